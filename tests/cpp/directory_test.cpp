// directory_test.cpp — GpuMatchPlugin's directory methods (protocol_amd/plugin/gpu_match_directory.cpp) and their C face
// (pm_plugin_directory_c.cpp) against tests/cpp/mock_engine.cpp + tests/cpp/mock_directory.cpp: the queries each method sends, the
// size query and the one call behind it, the listing with its group objects and counts, the gauge's names, the two status lists,
// paging, an engine row without an address, an engine refusal, the texts and their buffer sizing.
#include <cstdio>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "gpu_match_plugin.hpp"
#include "pm_plugin_c.h"
#include "pm_plugin_c_internal.hpp"

namespace mock_directory {
extern std::mutex mu;
extern bool on;
extern std::vector<pm_dir_row> rows;
extern std::vector<uint32_t> ranks;
extern std::vector<std::string> calls;
}  // namespace mock_directory

using namespace orchestrator;

static int g_failed = 0;
#define CHECK(cond)                                                                      \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      std::fprintf(stderr, "  CHECK failed at %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                                        \
    }                                                                                    \
  } while (0)

static const int N = 10;
// node k's status; classes: Healthy {2, 7}, Discovered {0, 5}, the middle {1, 3, 6, 8, 9}, Dead {4}
static const uint8_t STATUS[N] = {PM_NS_DISCOVERED, PM_NS_WAITING, PM_NS_HEALTHY,    PM_NS_UNHEALTHY, PM_NS_DEAD,
                                  PM_NS_DISCOVERED, PM_NS_EJECTED, PM_NS_HEALTHY,    PM_NS_BANNED,    PM_NS_LOWBALANCE};
static const int LISTING[N] = {2, 7, 0, 5, 1, 3, 6, 8, 9, 4};
static std::string addr(int k) {
  char s[48];
  std::snprintf(s, sizeof(s), "0x%040x", 0x900 + (N - k) * 7);  // (descending texts: the address order is the rows' reversed)
  return s;
}
static uint8_t cls_of(uint8_t st) {
  return st == PM_NS_HEALTHY ? PM_DC_HEALTHY : st == PM_NS_DISCOVERED ? PM_DC_DISCOVERED : st == PM_NS_DEAD ? PM_DC_DEAD : PM_DC_OTHER;
}
static uint32_t row(const GpuMatchPlugin& p, int k) { return p.row_of(Address(addr(k))).value_or(PM_NONE); }

// N nodes; the mock's rows by the plugin's row numbers: nodes 2 and 7 in group 0xabc ("pair", slot 0), node 3 alone in 0xdef
// ("solo", slot 1); node 2 reports RUNNING
static std::shared_ptr<GpuMatchPlugin> make_plugin(int extra_rows = 0) {
  std::vector<NodeGroupConfiguration> cfgs = {{"pair", 2, 2, std::nullopt}, {"solo", 1, 1, std::nullopt}};
  auto p = std::make_shared<GpuMatchPlugin>(cfgs, 0, nullptr, std::vector<std::shared_ptr<WebhookPlugin>>{});
  p->clock = [] { return int64_t(777); };
  std::vector<OrchestratorNode> snap;
  for (int k = 0; k < N; ++k) {
    OrchestratorNode n;
    n.address = Address(addr(k));
    n.status = NodeStatus(STATUS[k]);
    n.p2p_id = "p2p-" + std::to_string(k);
    snap.push_back(n);
  }
  p->sync_nodes(snap);
  std::lock_guard<std::mutex> lk(mock_directory::mu);
  mock_directory::on = true;
  mock_directory::calls.clear();
  mock_directory::rows.assign(size_t(N + extra_rows), pm_dir_row{});
  mock_directory::ranks.assign(size_t(N + extra_rows), 0u);
  for (int k = 0; k < N + extra_rows; ++k) {
    const uint32_t w = k < N ? row(*p, k) : uint32_t(k);
    pm_dir_row& r = mock_directory::rows[w];
    r.worker = w;
    r.status = k < N ? STATUS[k] : uint8_t(PM_NS_DISCOVERED);
    r.cls = cls_of(r.status);
    r.state = uint8_t(PM_TS_NONE);
    r.counter = uint32_t(100 + k);
    r.group_slot = PM_NONE, r.group_id = PM_NONE, r.task = PM_NONE;
    mock_directory::ranks[w] = uint32_t(N + extra_rows - k);
  }
  for (int k : {2, 7}) {
    pm_dir_row& r = mock_directory::rows[row(*p, k)];
    r.group_slot = 0, r.group_id = 0xabcull, r.group_size = 2, r.config = 0, r.task = 1;
  }
  pm_dir_row& solo = mock_directory::rows[row(*p, 3)];
  solo.group_slot = 1, solo.group_id = 0xdefull, solo.group_size = 1, solo.config = 1;
  mock_directory::rows[row(*p, 2)].state = PM_TS_RUNNING, mock_directory::rows[row(*p, 2)].uid = 0xa1ull;
  return p;
}
static std::vector<std::string> take_calls() {
  std::lock_guard<std::mutex> lk(mock_directory::mu);
  std::vector<std::string> c;
  c.swap(mock_directory::calls);
  return c;
}
static std::vector<std::string> addrs(const int* k, size_t n) {
  std::vector<std::string> out;
  for (size_t i = 0; i < n; ++i) out.push_back(addr(k[i]));
  return out;
}
static std::vector<std::string> listed(const GpuMatchPlugin::NodeListing& l) {
  std::vector<std::string> out;
  for (const auto& n : l.nodes) out.push_back(n.address);
  return out;
}

static void the_listing_its_counts_and_its_groups() {
  auto p = make_plugin();
  const uint32_t all = (1u << PM_NS_N) - 1u, live = all & ~(1u << PM_NS_DEAD);
  const GpuMatchPlugin::NodeListing l = p->list_nodes(false);
  // the size query (no buffer), then one call with room for exactly the window
  CHECK((take_calls() == std::vector<std::string>{"mask=" + std::to_string(live) + " mem=0 order=0 off=0 lim=4294967295 cap=0",
                                                  "mask=" + std::to_string(live) + " mem=0 order=0 off=0 lim=4294967295 cap=9"}));
  CHECK(l.total == 9 && listed(l) == addrs(LISTING, 9));
  CHECK((l.counts == std::map<std::string, uint32_t>{{"Discovered", 2}, {"WaitingForHeartbeat", 1}, {"Healthy", 2}, {"Unhealthy", 1},
                                                     {"Ejected", 1}, {"Banned", 1}, {"LowBalance", 1}}));  // (no "Dead": 0 is not named)
  CHECK(l.nodes[0].status == NodeStatus::Healthy && l.nodes[0].unhealthy_counter == 102 && l.nodes[0].task_state == PM_TS_RUNNING);
  CHECK(l.nodes[0].group && l.nodes[0].group->id == "abc" && l.nodes[0].group->size == 2 && l.nodes[0].group->topology_config == "pair" &&
        l.nodes[0].group->created_at == 777);
  CHECK(l.nodes[1].group && l.nodes[1].group->id == "abc" && l.nodes[1].task_state == PM_TS_NONE);
  CHECK(!l.nodes[2].group && l.nodes[2].status == NodeStatus::Discovered);
  CHECK(l.nodes[5].address == addr(3) && l.nodes[5].group && l.nodes[5].group->id == "def" && l.nodes[5].group->topology_config == "solo" &&
        l.nodes[5].group->size == 1);
  const GpuMatchPlugin::NodeListing d = p->list_nodes(true);
  CHECK(d.total == 10 && listed(d) == addrs(LISTING, 10) && d.counts.at("Dead") == 1 && d.nodes[9].status == NodeStatus::Dead);
  CHECK(take_calls().size() == 2);
  // by address: the texts descend with k, so every class comes out reversed
  const int by_addr[N] = {7, 2, 5, 0, 9, 8, 6, 3, 1, 4};
  CHECK(listed(p->list_nodes(true, PM_DIR_BY_ADDRESS)) == addrs(by_addr, N));
  CHECK(take_calls()[0] == "mask=" + std::to_string(all) + " mem=0 order=1 off=0 lim=4294967295 cap=0");
}

static void pages() {
  auto p = make_plugin();
  std::vector<std::string> joined;
  for (uint32_t off = 0; off < 12; off += 3) {
    const GpuMatchPlugin::NodeListing l = p->list_nodes(true, PM_DIR_BY_ROW, off, 3);
    CHECK(l.total == 10 && l.counts.size() == 8 && l.nodes.size() == (off < 9 ? 3u : off == 9 ? 1u : 0u));
    for (const auto& n : l.nodes) joined.push_back(n.address);
  }
  CHECK(joined == addrs(LISTING, N));
  take_calls();
  const GpuMatchPlugin::NodeListing none = p->list_nodes(true, PM_DIR_BY_ROW, 10, 5);  // offset = total: the counters, no second call
  CHECK(none.total == 10 && none.nodes.empty() && none.counts.size() == 8 && take_calls().size() == 1);
  const GpuMatchPlugin::NodeListing zero = p->list_nodes(false, PM_DIR_BY_ROW, 0, 0);
  CHECK(zero.total == 9 && zero.nodes.empty() && take_calls().size() == 1);
  const GpuMatchPlugin::NodeListing tail = p->list_nodes(true, PM_DIR_BY_ROW, 8, 0xFFFFFFFFu);  // offset + limit would wrap
  CHECK(listed(tail) == addrs(LISTING + 8, 2));
}

static void the_gauge_and_the_two_lists() {
  auto p = make_plugin();
  const uint32_t all = (1u << PM_NS_N) - 1u;
  CHECK((p->status_counts() == std::map<std::string, uint32_t>{{"discovered", 2}, {"waitingforheartbeat", 1}, {"healthy", 2},
                                                               {"unhealthy", 1}, {"dead", 1}, {"ejected", 1}, {"banned", 1},
                                                               {"lowbalance", 1}}));
  CHECK((take_calls() == std::vector<std::string>{"mask=" + std::to_string(all) + " mem=0 order=0 off=0 lim=0 cap=0"}));  // one call
  const int disc[2] = {0, 5}, dead[1] = {4};
  CHECK(p->uninvited_nodes() == addrs(disc, 2));
  CHECK((take_calls() == std::vector<std::string>{"mask=1 mem=0 order=0 off=0 lim=4294967295 cap=0",
                                                  "mask=1 mem=0 order=0 off=0 lim=4294967295 cap=2"}));
  CHECK(p->dead_nodes() == addrs(dead, 1));
  CHECK(take_calls()[1] == "mask=16 mem=0 order=0 off=0 lim=4294967295 cap=1");
  {
    std::lock_guard<std::mutex> lk(mock_directory::mu);
    for (pm_dir_row& r : mock_directory::rows) r.status = PM_NS_HEALTHY, r.cls = PM_DC_HEALTHY;
  }
  CHECK(p->uninvited_nodes().empty() && p->dead_nodes().empty());
  CHECK((p->status_counts() == std::map<std::string, uint32_t>{{"healthy", 10}}));
  CHECK(GpuMatchPlugin::status_name(PM_NS_WAITING) == std::string("WaitingForHeartbeat"));
  bool threw = false;
  try {
    GpuMatchPlugin::status_name(PM_NS_N);
  } catch (const std::out_of_range&) {
    threw = true;
  }
  CHECK(threw);
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

static void what_the_plugin_refuses() {
  {  // the engine lists a row the node table has no address for
    auto p = make_plugin(2);
    CHECK(throws_range([&] { p->list_nodes(true); }) && throws_range([&] { p->uninvited_nodes(); }));
    CHECK(p->dead_nodes().size() == 1);                       // (the rows behind the table are Discovered: not in this list)
    CHECK(p->status_counts().at("discovered") == 4);          // the counters name no row
    CHECK(p->list_nodes(true, PM_DIR_BY_ROW, 0, 2).nodes.size() == 2);  // nor does a window that does not reach them
  }
  {  // a configuration the plugin has not; a status that is none
    auto p = make_plugin();
    {
      std::lock_guard<std::mutex> lk(mock_directory::mu);
      mock_directory::rows[row(*p, 3)].config = 2;
    }
    CHECK(throws_range([&] { p->list_nodes(true); }));
  }
  {  // the engine's refusal travels as it is
    auto p = make_plugin();
    {
      std::lock_guard<std::mutex> lk(mock_directory::mu);
      mock_directory::on = false;
    }
    int code = 0;
    try {
      p->status_counts();
    } catch (const EngineError& x) {
      code = x.code();
    }
    CHECK(code == PM_ESTATE);
    code = 0;
    try {
      p->list_nodes(false, 7u);  // an unknown order: PM_EINVAL
    } catch (const EngineError& x) {
      code = x.code();
    }
    CHECK(code == PM_EINVAL);
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
  const std::string want = "total\t9\ncount\tBanned\t1\ncount\tDiscovered\t2\ncount\tEjected\t1\ncount\tHealthy\t2\ncount\tLowBalance\t1\n"
                           "count\tUnhealthy\t1\ncount\tWaitingForHeartbeat\t1\n" +
                           addr(2) + "\tHealthy\t102\t2\tabc\t2\tpair\n" + addr(7) + "\tHealthy\t107\t-\tabc\t2\tpair\n" +
                           addr(0) + "\tDiscovered\t100\t-\t-\t-\t-\n" + addr(5) + "\tDiscovered\t105\t-\t-\t-\t-\n" +
                           addr(1) + "\tWaitingForHeartbeat\t101\t-\t-\t-\t-\n" + addr(3) + "\tUnhealthy\t103\t-\tdef\t1\tsolo\n" +
                           addr(6) + "\tEjected\t106\t-\t-\t-\t-\n" + addr(8) + "\tBanned\t108\t-\t-\t-\t-\n" +
                           addr(9) + "\tLowBalance\t109\t-\t-\t-\t-\n";
  CHECK(text_of([&](char* o, size_t c, size_t* n) { return pmx_list_nodes(&h, 0, 0, 0, 0xFFFFFFFFu, o, c, n); }) == want);
  CHECK(text_of([&](char* o, size_t c, size_t* n) { return pmx_list_nodes(&h, 1, 1, 9, 5, o, c, n); }) ==
        "total\t10\ncount\tBanned\t1\ncount\tDead\t1\ncount\tDiscovered\t2\ncount\tEjected\t1\ncount\tHealthy\t2\ncount\tLowBalance\t1\n"
        "count\tUnhealthy\t1\ncount\tWaitingForHeartbeat\t1\n" + addr(4) + "\tDead\t104\t-\t-\t-\t-\n");
  CHECK(text_of([&](char* o, size_t c, size_t* n) { return pmx_status_counts(&h, o, c, n); }) ==
        "banned\t1\ndead\t1\ndiscovered\t2\nejected\t1\nhealthy\t2\nlowbalance\t1\nunhealthy\t1\nwaitingforheartbeat\t1\n");
  CHECK(text_of([&](char* o, size_t c, size_t* n) { return pmx_uninvited_nodes(&h, o, c, n); }) == addr(0) + "\n" + addr(5) + "\n");
  CHECK(text_of([&](char* o, size_t c, size_t* n) { return pmx_dead_nodes(&h, o, c, n); }) == addr(4) + "\n");
  // sizing: a buffer one byte short is refused with the size it needs, nothing else changes
  size_t need = 0, need2 = 0;
  CHECK(pmx_dead_nodes(&h, nullptr, 0, &need) == 0 && need == addr(4).size() + 2);
  std::string small(need - 1, '\0');
  CHECK(pmx_dead_nodes(&h, small.data(), small.size(), &need2) == -2 && need2 == need);
  CHECK(pmx_list_nodes(&h, 0, 9, 0, 1, nullptr, 0, &need) == -1 && std::string(pmx_last_error()).size() > 0);  // an unknown order
  {
    std::lock_guard<std::mutex> lk(mock_directory::mu);
    mock_directory::on = false;
  }
  CHECK(pmx_status_counts(&h, nullptr, 0, &need) == -1 && pmx_uninvited_nodes(&h, nullptr, 0, &need) == -1);
}

int main() {
  the_listing_its_counts_and_its_groups();
  pages();
  the_gauge_and_the_two_lists();
  what_the_plugin_refuses();
  the_c_face();
  std::printf("5 tests, %d failed checks\n", g_failed);
  return g_failed ? 1 : 0;
}
