// groupdir_test.cpp — GpuMatchPlugin's group directory methods (protocol_amd/plugin/gpu_match_groupdir.cpp) and their C face
// (pm_plugin_groupdir_c.cpp) against tests/cpp/mock_engine.cpp + tests/cpp/mock_groupdir.cpp: the query each method sends, the
// counters-only query and the one sized call behind it, the NodeGroup objects with their classes and task ids, paging, the
// gauge's "present only" rule, a group whose member has no address, an engine refusal, the texts and their buffer sizing.
#include <cstdio>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "gpu_match_plugin.hpp"
#include "pm_plugin_c.h"
#include "pm_plugin_c_internal.hpp"

namespace mock_groupdir {
struct G {
  pm_gdir_row row;
  std::vector<uint32_t> members;
};
extern std::mutex mu;
extern bool live_on, rollout_on;
extern uint32_t n_cfgs;
extern std::vector<G> groups;
extern std::vector<std::string> calls;
}  // namespace mock_groupdir

using namespace orchestrator;

static int g_failed = 0;
#define CHECK(cond)                                                                      \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      std::fprintf(stderr, "  CHECK failed at %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                                        \
    }                                                                                    \
  } while (0)

static const int N = 8;
static std::string addr(int k) {
  char s[48];
  std::snprintf(s, sizeof(s), "0x%040x", 0x900 + k * 7);
  return s;
}
static Task task(int k) {
  Task t;
  char id[40];
  std::snprintf(id, sizeof(id), "00000000-0000-4000-8000-%012x", 0x1000 + k);
  t.id = id;
  t.name = "task-" + std::to_string(k);
  t.image = "image";
  t.created_at = 100 - k;
  return t;
}
static uint32_t row(const GpuMatchPlugin& p, int k) { return p.row_of(Address(addr(k))).value_or(PM_NONE); }

static mock_groupdir::G group(uint64_t id, uint32_t slot, uint32_t cfg, uint32_t task, uint8_t health, uint8_t rollout,
                              std::vector<uint32_t> members) {
  mock_groupdir::G g{};
  g.row.group_id = id, g.row.slot = slot, g.row.config = cfg, g.row.size = uint32_t(members.size()), g.row.task = task;
  g.row.health = health, g.row.rollout = rollout;
  g.row.by_status[health == PM_GH_SOUND ? PM_NS_HEALTHY : health == PM_GH_LOST ? PM_NS_EJECTED : PM_NS_UNHEALTHY] = g.row.size;
  if (task != PM_NONE) (rollout == PM_GR_CONVERGED ? g.row.converged : g.row.silent) = g.row.size;
  g.members = std::move(members);
  return g;
}

// N nodes, three configurations, two tasks; the mock's groups by the plugin's row numbers:
//   slot 0  id 0x100  "pair"  nodes 0, 1  task 0  sound     converged
//   slot 1  id 0xff   "solo"  node 2      no task degraded  no_task
//   slot 2  id 0x2    "pair"  nodes 4, 3  task 1  lost      rolling     (member order 4, 3: the engine's, kept)
// no group of "spare"; text order "100" < "2" < "ff"
static std::shared_ptr<GpuMatchPlugin> make_plugin(bool stranger = false) {
  std::vector<NodeGroupConfiguration> cfgs = {{"pair", 2, 2, std::nullopt}, {"solo", 1, 1, std::nullopt}, {"spare", 1, 4, std::nullopt}};
  auto p = std::make_shared<GpuMatchPlugin>(cfgs, 0, nullptr, std::vector<std::shared_ptr<WebhookPlugin>>{});
  p->clock = [] { return int64_t(777); };
  std::vector<OrchestratorNode> snap;
  for (int k = 0; k < N; ++k) {
    OrchestratorNode n;
    n.address = Address(addr(k));
    n.status = NodeStatus::Healthy;
    n.p2p_id = "p2p-" + std::to_string(k);
    snap.push_back(n);
  }
  p->sync_nodes(snap);
  p->sync_tasks({task(0), task(1)});
  std::lock_guard<std::mutex> lk(mock_groupdir::mu);
  mock_groupdir::live_on = mock_groupdir::rollout_on = true;
  mock_groupdir::n_cfgs = 3;
  mock_groupdir::calls.clear();
  mock_groupdir::groups = {group(0x100, 0, 0, 0, PM_GH_SOUND, PM_GR_CONVERGED, {row(*p, 0), row(*p, 1)}),
                           group(0xff, 1, 1, PM_NONE, PM_GH_DEGRADED, PM_GR_NO_TASK, {row(*p, 2)}),
                           group(0x2, 2, 0, 1, PM_GH_LOST, PM_GR_ROLLING, {row(*p, 4), stranger ? uint32_t(N + 3) : row(*p, 3)})};
  return p;
}
static std::vector<std::string> take_calls() {
  std::lock_guard<std::mutex> lk(mock_groupdir::mu);
  std::vector<std::string> c;
  c.swap(mock_groupdir::calls);
  return c;
}
static std::vector<std::string> ids(const std::vector<GpuMatchPlugin::ListedNodeGroup>& g) {
  std::vector<std::string> out;
  for (const auto& x : g) out.push_back(x.group.id);
  return out;
}
static const std::string ALL = "cfg=ffffffffffffffff holds=0 size=0-4294967295 health=7 rollout=7";

static void the_listing_and_the_queries() {
  auto p = make_plugin();
  const GpuMatchPlugin::GroupListing l = p->list_groups(GpuMatchPlugin::GroupFilter());
  // the counters-only query (limit 0, no buffers: no sort on the device), then ONE call with room for the window and the list's
  // members
  CHECK((take_calls() == std::vector<std::string>{ALL + " order=1 off=0 lim=0 caps=0/0/0",
                                                  ALL + " order=1 off=0 lim=4294967295 caps=0/3/5"}));
  CHECK(l.total == 3 && l.totals.members_total == 5 && (ids(l.groups) == std::vector<std::string>{"100", "2", "ff"}));
  CHECK(l.totals.by_health[PM_GH_LOST] == 1 && l.totals.by_health[PM_GH_DEGRADED] == 1 && l.totals.by_health[PM_GH_SOUND] == 1);
  const auto& a = l.groups[0];
  CHECK((a.group.nodes == std::vector<std::string>{addr(0), addr(1)}) && a.group.configuration_name == "pair" && a.group.created_at == 777);
  CHECK(a.health == PM_GH_SOUND && a.rollout == PM_GR_CONVERGED && a.task_id && *a.task_id == task(0).id && a.row.converged == 2);
  const auto& b = l.groups[1];
  CHECK((b.group.nodes == std::vector<std::string>{addr(4), addr(3)}) && b.health == PM_GH_LOST && b.rollout == PM_GR_ROLLING);
  CHECK(b.task_id && *b.task_id == task(1).id && b.row.by_status[PM_NS_EJECTED] == 2 && b.row.silent == 2);
  const auto& c = l.groups[2];
  CHECK((c.group.nodes == std::vector<std::string>{addr(2)}) && c.group.configuration_name == "solo" && !c.task_id);
  CHECK(c.health == PM_GH_DEGRADED && c.rollout == PM_GR_NO_TASK);
  // a filter travels field by field
  GpuMatchPlugin::GroupFilter f;
  f.config_mask = 1, f.holds = PM_GDIR_WITH_TASK, f.size_min = 2, f.size_max = 9, f.health_mask = 5, f.rollout_mask = 6;
  const GpuMatchPlugin::GroupListing m = p->list_groups(f, PM_GDIR_BY_SIZE_DESC, 0, 10);
  CHECK((take_calls() == std::vector<std::string>{"cfg=1 holds=1 size=2-9 health=5 rollout=6 order=2 off=0 lim=0 caps=0/0/0",
                                                  "cfg=1 holds=1 size=2-9 health=5 rollout=6 order=2 off=0 lim=10 caps=0/2/4"}));
  CHECK(m.total == 2 && (ids(m.groups) == std::vector<std::string>{"100", "2"}));
  CHECK((ids(p->list_groups(GpuMatchPlugin::GroupFilter(), PM_GDIR_BY_SLOT).groups) == std::vector<std::string>{"100", "ff", "2"}));
}

static void pages() {
  auto p = make_plugin();
  std::vector<std::string> joined, nodes;
  for (uint32_t off = 0; off < 5; off += 2) {
    const GpuMatchPlugin::GroupListing l = p->list_groups(GpuMatchPlugin::GroupFilter(), PM_GDIR_BY_ID_TEXT, off, 2);
    CHECK(l.total == 3 && l.totals.members_total == 5 && l.groups.size() == (off == 0 ? 2u : off == 2 ? 1u : 0u));
    for (const auto& g : l.groups) {
      joined.push_back(g.group.id);
      nodes.insert(nodes.end(), g.group.nodes.begin(), g.group.nodes.end());  // (member_begin restarts with every window)
    }
  }
  CHECK((joined == std::vector<std::string>{"100", "2", "ff"}));
  CHECK((nodes == std::vector<std::string>{addr(0), addr(1), addr(4), addr(3), addr(2)}));
  take_calls();
  const GpuMatchPlugin::GroupListing none = p->list_groups(GpuMatchPlugin::GroupFilter(), PM_GDIR_BY_ID_TEXT, 3, 5);
  CHECK(none.total == 3 && none.groups.empty() && take_calls().size() == 1);  // offset = total: the counters, no second call
  const GpuMatchPlugin::GroupListing zero = p->list_groups(GpuMatchPlugin::GroupFilter(), PM_GDIR_BY_ID_TEXT, 0, 0);
  CHECK(zero.total == 3 && zero.groups.empty() && take_calls().size() == 1);
  const GpuMatchPlugin::GroupListing tail = p->list_groups(GpuMatchPlugin::GroupFilter(), PM_GDIR_BY_ID_TEXT, 2, 0xFFFFFFFFu);  // offset + limit would wrap
  CHECK((ids(tail.groups) == std::vector<std::string>{"ff"}));
}

static void the_gauge_and_the_degraded_groups() {
  auto p = make_plugin();
  CHECK((p->group_counts() == std::map<std::string, uint32_t>{{"pair", 2}, {"solo", 1}}));  // no "spare": a name no group carries is not set
  CHECK((take_calls() == std::vector<std::string>{ALL + " order=0 off=0 lim=0 caps=64/0/0"}));  // one counters-only call
  const std::vector<GpuMatchPlugin::ListedNodeGroup> d = p->degraded_groups();
  CHECK((take_calls() == std::vector<std::string>{"cfg=ffffffffffffffff holds=0 size=0-4294967295 health=3 rollout=7 order=1 off=0 lim=0 caps=0/0/0",
                                                  "cfg=ffffffffffffffff holds=0 size=0-4294967295 health=3 rollout=7 order=1 off=0 lim=4294967295 caps=0/2/3"}));
  CHECK((ids(d) == std::vector<std::string>{"2", "ff"}) && d[0].health == PM_GH_LOST && d[1].health == PM_GH_DEGRADED);
  {
    std::lock_guard<std::mutex> lk(mock_groupdir::mu);
    for (auto& g : mock_groupdir::groups) g.row.health = PM_GH_SOUND;
  }
  CHECK(p->degraded_groups().empty() && take_calls().size() == 1);  // every member recovered: the list is empty, one call
  {
    std::lock_guard<std::mutex> lk(mock_groupdir::mu);
    mock_groupdir::groups.clear();
  }
  CHECK(p->group_counts().empty());
}

template <typename F>
static bool throws_range(F&& f) {
  try {
    f();
  } catch (const std::out_of_range&) {
    return true;
  } catch (...) {
  }
  return false;
}
template <typename F>
static int engine_code(F&& f) {
  try {
    f();
  } catch (const EngineError& x) {
    return x.code();
  } catch (...) {
    return 1;
  }
  return 0;
}

static void what_the_plugin_refuses() {
  {  // the engine lists a member the node table has no address for
    auto p = make_plugin(true);
    CHECK(throws_range([&] { p->list_groups(GpuMatchPlugin::GroupFilter()); }) && throws_range([&] { p->degraded_groups(); }));
    CHECK(p->group_counts().at("pair") == 2);                                                 // the counters name no member
    CHECK(p->list_groups(GpuMatchPlugin::GroupFilter(), PM_GDIR_BY_ID_TEXT, 0, 1).groups.size() == 1);  // nor does a window that does not reach it
  }
  {  // a configuration or a task the plugin has not
    auto p = make_plugin();
    {
      std::lock_guard<std::mutex> lk(mock_groupdir::mu);
      mock_groupdir::groups[1].row.config = 3;
    }
    CHECK(throws_range([&] { p->list_groups(GpuMatchPlugin::GroupFilter()); }));
    {
      std::lock_guard<std::mutex> lk(mock_groupdir::mu);
      mock_groupdir::groups[1].row.config = 1, mock_groupdir::groups[0].row.task = 2;
    }
    CHECK(throws_range([&] { p->list_groups(GpuMatchPlugin::GroupFilter()); }));
  }
  {  // the engine's refusal travels as it is
    auto p = make_plugin();
    {
      std::lock_guard<std::mutex> lk(mock_groupdir::mu);
      mock_groupdir::live_on = false;
    }
    CHECK(engine_code([&] { p->degraded_groups(); }) == PM_ESTATE);
    CHECK(engine_code([&] { p->group_counts(); }) == 0);  // (the gauge asks for no class)
    CHECK(engine_code([&] { p->list_groups(GpuMatchPlugin::GroupFilter(), 7u); }) == PM_EINVAL);  // an unknown order
    GpuMatchPlugin::GroupFilter f;
    f.size_min = 3, f.size_max = 2;
    CHECK(engine_code([&] { p->list_groups(f); }) == PM_EINVAL);
  }
}

template <typename F>
static std::string text_of(F&& call) {
  size_t need = 0;
  if (call(nullptr, size_t(0), &need) != 0) return "<error>";
  std::string buf(need ? need : 1, '\0');
  size_t again = 0;
  if (call(buf.data(), buf.size(), &again) != 0 || again != need) return "<error>";
  buf.resize(need ? need - 1 : 0);
  return buf;
}

static void the_c_face() {
  pmx_plugin h;
  h.plugin = make_plugin();
  const std::string g100 = "100\tpair\t2\tsound\tconverged\t" + task(0).id + "\t777\t" + addr(0) + "," + addr(1) + "\n";
  const std::string g2 = "2\tpair\t2\tlost\trolling\t" + task(1).id + "\t777\t" + addr(4) + "," + addr(3) + "\n";
  const std::string gff = "ff\tsolo\t1\tdegraded\tno_task\t-\t777\t" + addr(2) + "\n";
  CHECK(text_of([&](char* o, size_t c, size_t* n) { return pmx_list_groups(&h, ~0ull, 0, 0, 0xFFFFFFFFu, 7, 7, 1, 0, 0xFFFFFFFFu, o, c, n); }) ==
        "total\t3\t5\n" + g100 + g2 + gff);
  CHECK(text_of([&](char* o, size_t c, size_t* n) { return pmx_list_groups(&h, ~0ull, 0, 0, 0xFFFFFFFFu, 7, 7, 0, 1, 1, o, c, n); }) ==
        "total\t3\t5\n" + gff);
  CHECK(text_of([&](char* o, size_t c, size_t* n) { return pmx_group_counts(&h, o, c, n); }) == "pair\t2\nsolo\t1\n");
  CHECK(text_of([&](char* o, size_t c, size_t* n) { return pmx_degraded_groups(&h, o, c, n); }) == g2 + gff);
  // sizing: a buffer one byte short is refused with the size it needs, nothing else changes
  size_t need = 0, need2 = 0;
  CHECK(pmx_group_counts(&h, nullptr, 0, &need) == 0 && need == std::string("pair\t2\nsolo\t1\n").size() + 1);
  std::string small(need - 1, '\0');
  CHECK(pmx_group_counts(&h, small.data(), small.size(), &need2) == -2 && need2 == need);
  CHECK(pmx_list_groups(&h, ~0ull, 0, 0, 1, 7, 7, 9, 0, 1, nullptr, 0, &need) == -1 && std::string(pmx_last_error()).size() > 0);  // an unknown order
  {
    std::lock_guard<std::mutex> lk(mock_groupdir::mu);
    mock_groupdir::live_on = mock_groupdir::rollout_on = false;
    for (auto& g : mock_groupdir::groups) g.row.health = uint8_t(PM_GH_NONE), g.row.rollout = uint8_t(PM_GR_NONE);
  }
  CHECK(pmx_degraded_groups(&h, nullptr, 0, &need) == -1);
  CHECK(text_of([&](char* o, size_t c, size_t* n) { return pmx_list_groups(&h, ~0ull, 0, 0, 0xFFFFFFFFu, 7, 7, 1, 2, 1, o, c, n); }) ==
        "total\t3\t5\nff\tsolo\t1\t-\t-\t-\t777\t" + addr(2) + "\n");  // both ledgers off: no class to name
}

int main() {
  the_listing_and_the_queries();
  pages();
  the_gauge_and_the_degraded_groups();
  what_the_plugin_refuses();
  the_c_face();
  std::printf("5 tests, %d failed checks\n", g_failed);
  return g_failed ? 1 : 0;
}
