// changes_test.cpp — GpuMatchPlugin::enable_change_feed / changed_nodes (protocol_amd/plugin/gpu_match_changes.cpp) and their C
// face pmx_enable_change_feed / pmx_changed_nodes (pm_plugin_changes_c.cpp) against tests/cpp/mock_engine.cpp +
// tests/cpp/mock_changes.cpp: the size query then the drain; a list that grows between the two calls leads to another call, never
// to a short read; the resync flag comes through once; worker rows come back as node addresses in row order; a row the node
// table does not hold is an error; an empty feed is an empty answer; an engine refusal is thrown as EngineError.
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "gpu_match_plugin.hpp"
#include "pm_plugin_c.h"
#include "pm_plugin_c_internal.hpp"

namespace mock_changes {
extern bool on, resync;
extern int32_t fail_with;
extern std::vector<pm_change_row> pending;
extern std::vector<std::vector<pm_change_row>> grow_behind_refusal;
extern uint32_t refused, drained, enables;
extern std::vector<uint32_t> caps;
}  // namespace mock_changes

using namespace orchestrator;

static int g_failed = 0;
#define CHECK(cond)                                                                      \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      std::fprintf(stderr, "  CHECK failed at %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                                        \
    }                                                                                    \
  } while (0)

static const int N = 23;
static std::string addr(int k) {
  char s[48];
  std::snprintf(s, sizeof(s), "0x%040x", 0x300 + k * 7);
  return s;
}
static OrchestratorNode node(int k) {
  OrchestratorNode n;
  n.address = Address(addr(k));
  n.status = NodeStatus::Healthy;
  n.p2p_id = "p2p-" + std::to_string(k);
  return n;
}

static std::shared_ptr<GpuMatchPlugin> make_plugin() {
  std::vector<NodeGroupConfiguration> cfgs = {{"pair", 2, 2, std::nullopt}, {"solo", 1, 1, std::nullopt}};
  auto p = std::make_shared<GpuMatchPlugin>(cfgs, 0, nullptr, std::vector<std::shared_ptr<WebhookPlugin>>{});
  std::vector<OrchestratorNode> snap;
  for (int k = 0; k < N; ++k) snap.push_back(node(k));
  p->sync_nodes(snap);
  mock_changes::on = mock_changes::resync = false;
  mock_changes::fail_with = PM_OK;
  mock_changes::pending.clear();
  mock_changes::grow_behind_refusal.clear();
  mock_changes::refused = mock_changes::drained = mock_changes::enables = 0;
  mock_changes::caps.clear();
  return p;
}
static std::string addr_of_row(const GpuMatchPlugin& p, uint32_t w) {
  for (int k = 0; k < N; ++k) {
    const std::optional<uint32_t> r = p.row_of(Address(addr(k)));
    CHECK(r.has_value());
    if (r.value_or(PM_NONE) == w) return addr(k);
  }
  CHECK(!"no node has this row");
  return "";
}

static void query_then_drain_and_the_resync_flag_once() {
  auto p = make_plugin();
  bool threw = false;
  try {  // the feed is off: the engine's PM_ESTATE
    p->changed_nodes();
  } catch (const EngineError& x) {
    threw = x.code() == PM_ESTATE;
  }
  CHECK(threw);
  p->enable_change_feed(true);
  CHECK(mock_changes::on && mock_changes::enables == 1);
  mock_changes::pending = {{2, PM_CHG_TASK}, {5, PM_CHG_GROUP | PM_CHG_RING}, {22, 7}};
  const GpuMatchPlugin::ChangedNodes r = p->changed_nodes();
  CHECK(mock_changes::caps.size() == 2 && mock_changes::caps[0] == 0 && mock_changes::caps[1] == 3);  // the query, the drain
  CHECK(mock_changes::refused == 1 && mock_changes::drained == 1);
  CHECK(r.resync && r.nodes.size() == 3);
  CHECK(r.nodes[0] == std::make_pair(addr_of_row(*p, 2), uint32_t(PM_CHG_TASK)));
  CHECK(r.nodes[1] == std::make_pair(addr_of_row(*p, 5), uint32_t(PM_CHG_GROUP | PM_CHG_RING)));
  CHECK(r.nodes[2] == std::make_pair(addr_of_row(*p, 22), 7u));
  // an empty feed: an empty answer, and the resync flag does not come twice
  const GpuMatchPlugin::ChangedNodes e = p->changed_nodes();
  CHECK(!e.resync && e.nodes.empty() && mock_changes::pending.empty());
  p->enable_change_feed(false);
  CHECK(!mock_changes::on && mock_changes::enables == 2);
}

static void a_list_that_grows_between_the_two_calls() {
  auto p = make_plugin();
  p->enable_change_feed(true);
  mock_changes::resync = false;
  mock_changes::pending = {{1, 1}, {3, 2}};
  mock_changes::grow_behind_refusal = {{{7, 4}}, {{9, 7}, {11, 1}}};  // behind the query, and behind the drain that was too small
  const GpuMatchPlugin::ChangedNodes r = p->changed_nodes();
  // the query says 2; the drain with room for 2 meets 3 and is refused; the one with room for 3 meets 5; the one for 5 drains
  CHECK((mock_changes::caps == std::vector<uint32_t>{0, 2, 3, 5}));
  CHECK(mock_changes::refused == 3 && mock_changes::drained == 1);
  CHECK(!r.resync && r.nodes.size() == 5);
  const uint32_t want_w[5] = {1, 3, 7, 9, 11}, want_b[5] = {1, 2, 4, 7, 1};
  for (size_t j = 0; j < r.nodes.size() && j < 5; ++j)
    CHECK(r.nodes[j] == std::make_pair(addr_of_row(*p, want_w[j]), want_b[j]));
  CHECK(mock_changes::pending.empty());
}

static void a_row_beyond_the_node_table_and_an_engine_refusal() {
  auto p = make_plugin();
  p->enable_change_feed(true);
  mock_changes::pending = {{4, 1}, {uint32_t(N), 2}};  // the node table has rows 0 .. N - 1
  bool threw = false;
  try {
    p->changed_nodes();
  } catch (const std::out_of_range&) {
    threw = true;
  }
  CHECK(threw);
  mock_changes::pending = {{PM_NONE, 7}};
  threw = false;
  try {
    p->changed_nodes();
  } catch (const std::out_of_range&) {
    threw = true;
  }
  CHECK(threw);
  mock_changes::fail_with = PM_ENODEV;
  threw = false;
  try {
    p->changed_nodes();
  } catch (const EngineError& x) {
    threw = x.code() == PM_ENODEV;
  }
  CHECK(threw);
}

static void the_c_face() {
  pmx_plugin h;
  h.plugin = make_plugin();
  size_t need = 0;
  CHECK(pmx_changed_nodes(&h, nullptr, 0, &need) == -1 && std::string(pmx_last_error()).size() > 0);  // the feed is off
  CHECK(pmx_enable_change_feed(&h, 1) == 0 && mock_changes::on);
  mock_changes::pending = {{0, 4}, {6, 3}};
  CHECK(pmx_changed_nodes(&h, nullptr, 0, &need) == 0 && need > 0);  // the size query drains once ...
  CHECK(mock_changes::drained == 1 && mock_changes::pending.empty());
  mock_changes::pending = {{8, 1}};                                  // (a tick in between: the next drain's)
  std::string small(need - 1, '\0'), buf(need, '\0');
  size_t need2 = 0;
  CHECK(pmx_changed_nodes(&h, small.data(), small.size(), &need2) == -2 && need2 == need);  // ... too small: still held ...
  CHECK(pmx_changed_nodes(&h, buf.data(), buf.size(), &need2) == 0 && need2 == need);       // ... and handed over
  CHECK(mock_changes::drained == 1);
  buf.resize(need - 1);
  CHECK(buf == "resync\t1\n" + addr_of_row(*h.plugin, 0) + "\t4\n" + addr_of_row(*h.plugin, 6) + "\t3\n");
  std::string next(256, '\0');
  CHECK(pmx_changed_nodes(&h, next.data(), next.size(), &need) == 0 && mock_changes::drained == 2);
  next.resize(need - 1);
  CHECK(next == "resync\t0\n" + addr_of_row(*h.plugin, 8) + "\t1\n");
  CHECK(pmx_changed_nodes(&h, next.data(), 256, &need) == 0 && std::string(next.c_str()) == "resync\t0\n");  // the empty feed
  mock_changes::pending = {{uint32_t(N) + 3u, 1}};
  CHECK(pmx_changed_nodes(&h, nullptr, 0, &need) == -1 && std::string(pmx_last_error()).find("node table") != std::string::npos);
  CHECK(pmx_enable_change_feed(&h, 0) == 0 && !mock_changes::on);
}

int main() {
  query_then_drain_and_the_resync_flag_once();
  a_list_that_grows_between_the_two_calls();
  a_row_beyond_the_node_table_and_an_engine_refusal();
  the_c_face();
  std::printf("4 tests, %d failed checks\n", g_failed);
  return g_failed ? 1 : 0;
}
