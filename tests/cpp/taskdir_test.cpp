// taskdir_test.cpp — GpuMatchPlugin's task directory methods (protocol_amd/plugin/gpu_match_taskdir.cpp) and their C face
// (pm_plugin_taskdir_c.cpp) against tests/cpp/mock_engine.cpp + tests/cpp/mock_taskdir.cpp (and, for the statistics, the mocks of
// the node directory, the group directory and the rollout ledger): the query each method sends, the counters-only query and the
// one sized call behind it, ids and names by position, paging, the "present only" rule of the statistics, the "unknown" name, a
// task the plugin has not, an engine refusal, the texts and their buffer sizing.
#include <cstdio>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "gpu_match_plugin.hpp"
#include "pm_plugin_c.h"
#include "pm_plugin_c_internal.hpp"

namespace mock_taskdir {
extern std::mutex mu;
extern bool rollout_on;
extern uint32_t n_cfgs, orphan_uids, orphan_reporters;
extern std::vector<pm_tdir_row> tasks;
extern std::vector<std::string> calls;
}  // namespace mock_taskdir
namespace mock_directory {
extern std::mutex mu;
extern bool on;
extern std::vector<pm_dir_row> rows;
extern std::vector<uint32_t> ranks;
extern std::vector<std::string> calls;
}  // namespace mock_directory
namespace mock_groupdir {
struct G {
  pm_gdir_row row;
  std::vector<uint32_t> members;
};
extern std::mutex mu;
extern uint32_t n_cfgs;
extern std::vector<G> groups;
extern std::vector<std::string> calls;
}  // namespace mock_groupdir
namespace mock_rollout {
extern std::mutex mu;
extern uint32_t W;
extern std::map<uint32_t, std::pair<uint64_t, uint32_t>> rows;
extern std::vector<uint64_t> task_uids;
extern std::vector<std::string> calls;
}  // namespace mock_rollout

using namespace orchestrator;

static int g_failed = 0;
#define CHECK(cond)                                                                      \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      std::fprintf(stderr, "  CHECK failed at %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                                        \
    }                                                                                    \
  } while (0)

static const int N = 6;
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

static pm_tdir_row trow(int k, uint64_t mask, uint32_t allowed, uint32_t running, uint32_t workers, uint8_t serve, uint8_t rollout,
                        uint32_t rep_running, uint32_t rep_failed) {
  pm_tdir_row r{};
  r.uid = task_uid(task(k)), r.created_at = 100 - k, r.topo_mask = mask, r.task = uint32_t(k);
  r.groups_allowed = allowed, r.groups_running = running, r.workers_running = workers;
  r.groups_converged = rollout == PM_TKR_CONVERGED ? running : 0u, r.converged = rollout == PM_TKR_CONVERGED ? workers : 0u;
  r.reporters[PM_TS_RUNNING] = rep_running, r.reporters[PM_TS_FAILED] = rep_failed;
  r.serve = serve, r.rollout = rollout;
  return r;
}

// N nodes, three configurations ("pair", "solo", "spare"), four tasks; what the mock lists, by position:
//   0  unrestricted  3 groups allowed  held by 1 group of 2 workers  running  converged  2 report it running
//   1  pair          2 groups allowed  held by none                  waiting  unheld     1 reports it failed
//   2  spare         no group stands                                 starved  unheld
//   3  pair | solo   3 groups allowed  held by 2 groups, 3 workers   running  rolling    1 reports it running
// two reported ids name no task, three rows report them
static std::shared_ptr<GpuMatchPlugin> make_plugin() {
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
  p->sync_tasks({task(0), task(1), task(2), task(3)});
  std::lock_guard<std::mutex> lk(mock_taskdir::mu);
  mock_taskdir::rollout_on = true;
  mock_taskdir::n_cfgs = 3;
  mock_taskdir::orphan_uids = 2, mock_taskdir::orphan_reporters = 3;
  mock_taskdir::calls.clear();
  mock_taskdir::tasks = {trow(0, ~0ull, 3, 1, 2, PM_TKS_RUNNING, PM_TKR_CONVERGED, 2, 0), trow(1, 0b001, 2, 0, 0, PM_TKS_WAITING, PM_TKR_UNHELD, 0, 1),
                         trow(2, 0b100, 0, 0, 0, PM_TKS_STARVED, PM_TKR_UNHELD, 0, 0), trow(3, 0b011, 3, 2, 3, PM_TKS_RUNNING, PM_TKR_ROLLING, 1, 0)};
  return p;
}
static std::vector<std::string> take_calls() {
  std::lock_guard<std::mutex> lk(mock_taskdir::mu);
  std::vector<std::string> c;
  c.swap(mock_taskdir::calls);
  return c;
}
static std::vector<std::string> names(const std::vector<GpuMatchPlugin::ListedTask>& t) {
  std::vector<std::string> out;
  for (const auto& x : t) out.push_back(x.name);
  return out;
}
static const std::string ALL = "cfg=ffffffffffffffff serve=7 rollout=7 workers=0-4294967295";

static void the_listing_and_the_queries() {
  auto p = make_plugin();
  const GpuMatchPlugin::TaskListing l = p->list_tasks(GpuMatchPlugin::TaskFilter());
  // the counters-only query (limit 0, no buffers), then ONE call with room for the window
  CHECK((take_calls() == std::vector<std::string>{ALL + " order=0 off=0 lim=0 caps=0/0", ALL + " order=0 off=0 lim=4294967295 caps=0/4"}));
  CHECK(l.total == 4 && l.totals.tasks == 4 && (names(l.tasks) == std::vector<std::string>{"task-0", "task-1", "task-2", "task-3"}));
  CHECK(l.totals.by_serve[PM_TKS_RUNNING] == 2 && l.totals.by_serve[PM_TKS_WAITING] == 1 && l.totals.by_serve[PM_TKS_STARVED] == 1);
  CHECK(l.totals.by_rollout[PM_TKR_UNHELD] == 2 && l.totals.unrestricted == 1 && l.totals.workers_running == 5 && l.totals.reporters == 4);
  CHECK(l.totals.orphan_uids == 2 && l.totals.orphan_reporters == 3);
  const auto& a = l.tasks[0];
  CHECK(a.id == task(0).id && a.serve == PM_TKS_RUNNING && a.rollout == PM_TKR_CONVERGED && a.row.workers_running == 2 && a.row.converged == 2);
  const auto& d = l.tasks[3];
  CHECK(d.id == task(3).id && d.rollout == PM_TKR_ROLLING && d.row.groups_running == 2 && d.row.reporters[PM_TS_RUNNING] == 1);
  // a filter travels field by field
  GpuMatchPlugin::TaskFilter f;
  f.config_mask = 3, f.serve_mask = 1, f.rollout_mask = 6, f.workers_min = 1, f.workers_max = 9;
  const GpuMatchPlugin::TaskListing m = p->list_tasks(f, PM_TDIR_BY_WORKERS_DESC, 0, 10);
  CHECK((take_calls() == std::vector<std::string>{"cfg=3 serve=1 rollout=6 workers=1-9 order=2 off=0 lim=0 caps=0/0",
                                                  "cfg=3 serve=1 rollout=6 workers=1-9 order=2 off=0 lim=10 caps=0/2"}));
  CHECK(m.total == 2 && (names(m.tasks) == std::vector<std::string>{"task-3", "task-0"}));
  CHECK((names(p->list_tasks(GpuMatchPlugin::TaskFilter(), PM_TDIR_BY_OLDEST).tasks) == std::vector<std::string>{"task-3", "task-2", "task-1", "task-0"}));
  CHECK((names(p->list_tasks(GpuMatchPlugin::TaskFilter(), PM_TDIR_BY_REPORTERS_DESC).tasks) == std::vector<std::string>{"task-0", "task-1", "task-3", "task-2"}));
}

static void pages() {
  auto p = make_plugin();
  std::vector<std::string> joined;
  for (uint32_t off = 0; off < 6; off += 3) {
    const GpuMatchPlugin::TaskListing l = p->list_tasks(GpuMatchPlugin::TaskFilter(), PM_TDIR_BY_LIST, off, 3);
    CHECK(l.total == 4 && l.tasks.size() == (off == 0 ? 3u : 1u));
    for (const auto& t : l.tasks) joined.push_back(t.name);
  }
  CHECK((joined == std::vector<std::string>{"task-0", "task-1", "task-2", "task-3"}));
  take_calls();
  const GpuMatchPlugin::TaskListing none = p->list_tasks(GpuMatchPlugin::TaskFilter(), PM_TDIR_BY_LIST, 4, 5);
  CHECK(none.total == 4 && none.tasks.empty() && take_calls().size() == 1);  // offset = total: the counters, no second call
  const GpuMatchPlugin::TaskListing zero = p->list_tasks(GpuMatchPlugin::TaskFilter(), PM_TDIR_BY_LIST, 0, 0);
  CHECK(zero.total == 4 && zero.tasks.empty() && take_calls().size() == 1);
  const GpuMatchPlugin::TaskListing tail = p->list_tasks(GpuMatchPlugin::TaskFilter(), PM_TDIR_BY_LIST, 3, 0xFFFFFFFFu);  // offset + limit would wrap
  CHECK((names(tail.tasks) == std::vector<std::string>{"task-3"}));
}

static void the_counts_and_the_starved_tasks() {
  auto p = make_plugin();
  const GpuMatchPlugin::TaskCounts c = p->task_counts();
  CHECK((take_calls() == std::vector<std::string>{ALL + " order=0 off=0 lim=0 caps=64/0"}));  // one counters-only call
  CHECK(c.totals.tasks == 4 && c.totals.total == 4 && (c.by_config == std::map<std::string, uint32_t>{{"pair", 3}, {"solo", 2}, {"spare", 2}}));
  const std::vector<GpuMatchPlugin::ListedTask> s = p->starved_tasks();
  CHECK((take_calls() == std::vector<std::string>{"cfg=ffffffffffffffff serve=4 rollout=7 workers=0-4294967295 order=0 off=0 lim=0 caps=0/0",
                                                  "cfg=ffffffffffffffff serve=4 rollout=7 workers=0-4294967295 order=0 off=0 lim=4294967295 caps=0/1"}));
  CHECK((names(s) == std::vector<std::string>{"task-2"}) && s[0].serve == PM_TKS_STARVED && s[0].row.groups_allowed == 0);
  {
    std::lock_guard<std::mutex> lk(mock_taskdir::mu);
    mock_taskdir::tasks[2].serve = PM_TKS_WAITING;
    for (auto& t : mock_taskdir::tasks) t.topo_mask &= 0b011;  // nothing allows "spare" any more: the name is not set
  }
  CHECK(p->starved_tasks().empty() && take_calls().size() == 1);  // a group of "spare" formed: the list is empty, one call
  CHECK((p->task_counts().by_config == std::map<std::string, uint32_t>{{"pair", 3}, {"solo", 2}}));
}

static void the_statistics() {
  auto p = make_plugin();
  p->enable_rollout();
  {
    std::lock_guard<std::mutex> a(mock_directory::mu);
    std::lock_guard<std::mutex> b(mock_groupdir::mu);
    std::lock_guard<std::mutex> c(mock_rollout::mu);
    mock_directory::on = true;
    mock_directory::rows.assign(N, pm_dir_row{});
    mock_directory::ranks.assign(N, 0u);
    for (int k = 0; k < N; ++k) {
      mock_directory::rows[k].worker = uint32_t(k), mock_directory::rows[k].group_slot = PM_NONE;
      mock_directory::rows[k].status = uint8_t(k < 4 ? PM_NS_HEALTHY : PM_NS_DEAD), mock_directory::rows[k].cls = uint8_t(k < 4 ? PM_DC_HEALTHY : PM_DC_DEAD);
    }
    mock_groupdir::n_cfgs = 3;
    mock_groupdir::groups.clear();
    for (uint32_t s = 0; s < 3; ++s) {
      mock_groupdir::G g{};
      g.row.group_id = 0x10 + s, g.row.slot = s, g.row.config = s == 2 ? 1u : 0u, g.row.size = 1, g.row.task = PM_NONE;
      g.row.health = PM_GH_SOUND, g.row.rollout = PM_GR_NO_TASK;
      g.members = {s};
      mock_groupdir::groups.push_back(g);
    }
    mock_rollout::W = N;
    mock_rollout::task_uids = {task_uid(task(0)), task_uid(task(1)), task_uid(task(2)), task_uid(task(3))};
    mock_rollout::rows = {{0, {task_uid(task(0)), PM_TS_RUNNING}}, {1, {task_uid(task(0)), PM_TS_FAILED}}, {2, {task_uid(task(3)), PM_TS_RUNNING}},
                          {5, {0xABCDull, PM_TS_RUNNING}}};
  }
  const GpuMatchPlugin::OrchestratorStatistics s = p->orchestrator_statistics();
  // present only: no status no node has, no configuration no group has, no task nobody reports
  CHECK((s.nodes_by_status == std::map<std::string, uint32_t>{{"healthy", 4}, {"dead", 2}}));
  CHECK(s.tasks_count == 4);
  CHECK((s.groups_count == std::map<std::string, uint32_t>{{"pair", 2}, {"solo", 1}}));
  std::map<std::string, std::pair<std::string, uint32_t>> npt;
  for (const auto& n : s.nodes_per_task) npt[n.task_id] = {n.task_name, n.count};
  CHECK(npt.size() == 3 && npt.size() == s.nodes_per_task.size());
  CHECK((npt[task(0).id] == std::pair<std::string, uint32_t>{"task-0", 2}) && (npt[task(3).id] == std::pair<std::string, uint32_t>{"task-3", 1}));
  CHECK((npt["abcd"] == std::pair<std::string, uint32_t>{"unknown", 1}));  // an id the task list has not: its name is "unknown"
  // every part is a counters-only query
  CHECK((take_calls() == std::vector<std::string>{ALL + " order=0 off=0 lim=0 caps=64/0"}));
  {
    std::lock_guard<std::mutex> a(mock_directory::mu);
    std::lock_guard<std::mutex> b(mock_groupdir::mu);
    CHECK(mock_directory::calls.size() == 1 && mock_directory::calls[0].find("lim=0") != std::string::npos);
    CHECK(mock_groupdir::calls.size() == 1 && mock_groupdir::calls[0].find("lim=0") != std::string::npos);
    mock_directory::calls.clear(), mock_groupdir::calls.clear();
  }
  pmx_plugin h;
  h.plugin = p;
  size_t need = 0;
  CHECK(pmx_orchestrator_statistics(&h, nullptr, 0, &need) == 0);
  std::string buf(need, '\0');
  CHECK(pmx_orchestrator_statistics(&h, buf.data(), buf.size(), &need) == 0);
  buf.resize(need - 1);
  CHECK(buf == "nodes\tdead\t2\nnodes\thealthy\t4\ntasks_count\t4\nnodes_per_task\tabcd\tunknown\t1\nnodes_per_task\t" + task(0).id +
                   "\ttask-0\t2\nnodes_per_task\t" + task(3).id + "\ttask-3\t1\ngroups_count\tpair\t2\ngroups_count\tsolo\t1\n");
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
  {  // the engine lists a task the plugin's list has not
    auto p = make_plugin();
    {
      std::lock_guard<std::mutex> lk(mock_taskdir::mu);
      mock_taskdir::tasks.push_back(trow(4, 1, 0, 0, 0, PM_TKS_STARVED, PM_TKR_UNHELD, 0, 0));
    }
    CHECK(throws_range([&] { p->list_tasks(GpuMatchPlugin::TaskFilter()); }) && throws_range([&] { p->starved_tasks(); }));
    CHECK(p->task_counts().totals.tasks == 5);                                                     // the counters name no task
    CHECK(p->list_tasks(GpuMatchPlugin::TaskFilter(), PM_TDIR_BY_LIST, 0, 4).tasks.size() == 4);  // nor does a window that does not reach it
  }
  {  // a configuration the plugin has not
    auto p = make_plugin();
    {
      std::lock_guard<std::mutex> lk(mock_taskdir::mu);
      mock_taskdir::n_cfgs = 4;
    }
    CHECK(throws_range([&] { p->task_counts(); }));
  }
  {  // the engine's refusal travels as it is
    auto p = make_plugin();
    {
      std::lock_guard<std::mutex> lk(mock_taskdir::mu);
      mock_taskdir::rollout_on = false;
    }
    GpuMatchPlugin::TaskFilter f;
    f.rollout_mask = 1u << PM_TKR_ROLLING;
    CHECK(engine_code([&] { p->list_tasks(f); }) == PM_ESTATE);
    CHECK(engine_code([&] { p->list_tasks(GpuMatchPlugin::TaskFilter(), PM_TDIR_BY_REPORTERS_DESC); }) == PM_ESTATE);
    CHECK(engine_code([&] { p->task_counts(); }) == 0 && engine_code([&] { p->starved_tasks(); }) == 0);  // (they ask for no rollout class)
    CHECK(engine_code([&] { p->list_tasks(GpuMatchPlugin::TaskFilter(), 7u); }) == PM_EINVAL);            // an unknown order
    f = GpuMatchPlugin::TaskFilter();
    f.workers_min = 3, f.workers_max = 2;
    CHECK(engine_code([&] { p->list_tasks(f); }) == PM_EINVAL);
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
  const std::string t0 = task(0).id + "\ttask-0\trunning\tconverged\t3\t1\t2\t1\t2\t2\n";
  const std::string t1 = task(1).id + "\ttask-1\twaiting\tunheld\t2\t0\t0\t0\t0\t1\n";
  const std::string t2 = task(2).id + "\ttask-2\tstarved\tunheld\t0\t0\t0\t0\t0\t0\n";
  const std::string t3 = task(3).id + "\ttask-3\trunning\trolling\t3\t2\t3\t0\t0\t1\n";
  CHECK(text_of([&](char* o, size_t c, size_t* n) { return pmx_list_tasks(&h, ~0ull, 7, 7, 0, 0xFFFFFFFFu, 0, 0, 0xFFFFFFFFu, o, c, n); }) ==
        "total\t4\t4\n" + t0 + t1 + t2 + t3);
  CHECK(text_of([&](char* o, size_t c, size_t* n) { return pmx_list_tasks(&h, ~0ull, 1, 7, 0, 0xFFFFFFFFu, 2, 1, 1, o, c, n); }) == "total\t2\t4\n" + t0);
  const std::string counts = "tasks\t4\nserve\t2\t1\t1\nrollout\t2\t1\t1\nunrestricted\t1\nworkers_running\t5\nreporters\t4\norphans\t2\t3\n"
                             "pair\t3\nsolo\t2\nspare\t2\n";
  CHECK(text_of([&](char* o, size_t c, size_t* n) { return pmx_task_counts(&h, o, c, n); }) == counts);
  CHECK(text_of([&](char* o, size_t c, size_t* n) { return pmx_starved_tasks(&h, o, c, n); }) == t2);
  // sizing: a buffer one byte short is refused with the size it needs, nothing else changes
  size_t need = 0, need2 = 0;
  CHECK(pmx_task_counts(&h, nullptr, 0, &need) == 0 && need == counts.size() + 1);
  std::string small(need - 1, '\0');
  CHECK(pmx_task_counts(&h, small.data(), small.size(), &need2) == -2 && need2 == need);
  CHECK(pmx_list_tasks(&h, ~0ull, 7, 7, 0, 1, 9, 0, 1, nullptr, 0, &need) == -1 && std::string(pmx_last_error()).size() > 0);  // an unknown order
  {
    std::lock_guard<std::mutex> lk(mock_taskdir::mu);
    mock_taskdir::rollout_on = false;
    for (auto& t : mock_taskdir::tasks) t.rollout = uint8_t(PM_TKR_NONE);
  }
  CHECK(pmx_list_tasks(&h, ~0ull, 7, 2, 0, 0xFFFFFFFFu, 0, 0, 1, nullptr, 0, &need) == -1);
  CHECK(text_of([&](char* o, size_t c, size_t* n) { return pmx_list_tasks(&h, ~0ull, 7, 7, 0, 0xFFFFFFFFu, 0, 2, 1, o, c, n); }) ==
        "total\t4\t4\n" + task(2).id + "\ttask-2\tstarved\t-\t0\t0\t0\t0\t0\t0\n");  // rollout off: no class to name
}

int main() {
  the_listing_and_the_queries();
  pages();
  the_counts_and_the_starved_tasks();
  the_statistics();
  what_the_plugin_refuses();
  the_c_face();
  std::printf("6 tests, %d failed checks\n", g_failed);
  return g_failed ? 1 : 0;
}
