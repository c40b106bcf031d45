// liveness_test.cpp — GpuMatchPlugin::enable_liveness / beat / sweep_statuses (protocol_amd/plugin/gpu_match_liveness.cpp) and
// their C face (pm_plugin_liveness_c.cpp) against tests/cpp/mock_engine.cpp + tests/cpp/mock_liveness.cpp: the call sequence
// the plugin makes (one applying sweep, then the list; what handle_status_change adds once liveness is on), the beat column and
// the pool bits it hands over, the transitions it returns and the statuses the nodes end on; a row the node table does not
// hold and an engine refusal; beat from several threads racing sweep_statuses and sync_nodes.
#include <atomic>
#include <cstdio>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "gpu_match_plugin.hpp"
#include "pm_plugin_c.h"
#include "pm_plugin_c_internal.hpp"

namespace mock_liveness {
extern std::mutex mu;
extern bool on;
extern uint32_t m, enables;
extern std::atomic<uint32_t> W;
extern int32_t fail_with;
extern std::vector<uint8_t> status;
extern std::vector<uint32_t> counter;
extern std::vector<std::string> calls;
extern std::vector<uint64_t> last_pool;
extern uint32_t extra_row;
}  // namespace mock_liveness
extern "C" const char* pm_mock_calls(void);
extern "C" void pm_mock_reset_calls(void);

using namespace orchestrator;

static int g_failed = 0;
#define CHECK(cond)                                                                      \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      std::fprintf(stderr, "  CHECK failed at %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                                        \
    }                                                                                    \
  } while (0)

static const int N = 70;  // (more than one word of pool bits)
static const uint64_t T0 = 1760000000000ull, STEP = 15000;
static std::string addr(int k) {
  char s[48];
  std::snprintf(s, sizeof(s), "0x%040x", 0x500 + k * 3);
  return s;
}
static OrchestratorNode node(int k) {
  OrchestratorNode n;
  n.address = Address(addr(k));
  n.status = NodeStatus::Healthy;
  n.p2p_id = "p2p-" + std::to_string(k);
  return n;
}
static std::vector<OrchestratorNode> snapshot(int n) {
  std::vector<OrchestratorNode> snap;
  for (int k = 0; k < n; ++k) snap.push_back(node(k));
  return snap;
}

static std::shared_ptr<GpuMatchPlugin> make_plugin() {
  std::vector<NodeGroupConfiguration> cfgs = {{"pair", 2, 2, std::nullopt}, {"solo", 1, 1, std::nullopt}};
  auto p = std::make_shared<GpuMatchPlugin>(cfgs, 0, nullptr, std::vector<std::shared_ptr<WebhookPlugin>>{});
  p->sync_nodes(snapshot(N));
  std::lock_guard<std::mutex> lk(mock_liveness::mu);
  mock_liveness::on = false;
  mock_liveness::m = mock_liveness::enables = 0;
  mock_liveness::W = uint32_t(N);
  mock_liveness::fail_with = PM_OK;
  mock_liveness::status.clear(), mock_liveness::counter.clear(), mock_liveness::calls.clear(), mock_liveness::last_pool.clear();
  mock_liveness::extra_row = PM_NONE;
  return p;
}
static uint32_t row(const GpuMatchPlugin& p, int k) {
  const std::optional<uint32_t> r = p.row_of(Address(addr(k)));
  CHECK(r.has_value());
  return r.value_or(PM_NONE);
}
static std::vector<std::string> take_calls() {
  std::lock_guard<std::mutex> lk(mock_liveness::mu);
  std::vector<std::string> c;
  c.swap(mock_liveness::calls);
  return c;
}
static void beat_all_but(const GpuMatchPlugin& p, uint64_t now, const std::vector<int>& silent) {
  for (int k = 0; k < N; ++k) {
    bool quiet = false;
    for (int s : silent) quiet = quiet || s == k;
    if (!quiet) p.beat(Address(addr(k)), now);
  }
}

static void the_call_sequence_and_the_statuses_it_ends_on() {
  auto p = make_plugin();
  bool threw = false;
  try {  // liveness is off: the engine's PM_ESTATE
    p->sweep_statuses(T0);
  } catch (const EngineError& x) {
    threw = x.code() == PM_ESTATE;
  }
  CHECK(threw);
  p->beat(Address(addr(1)), T0);  // (harmless before enable_liveness, and for an address nobody knows)
  p->beat(Address("0x00000000000000000000000000000000000000ff"), T0);
  OrchestratorNode banned = node(4);
  banned.status = NodeStatus::Banned;
  p->handle_status_change(banned);  // liveness off: no liveness call
  CHECK(take_calls().empty());
  banned.status = NodeStatus::Healthy;
  p->handle_status_change(banned);

  p->enable_liveness(3);
  CHECK(mock_liveness::on && mock_liveness::m == 3 && mock_liveness::enables == 1);
  CHECK((take_calls() == std::vector<std::string>{"enable m=3"}));
  // interval 1: 7 and 66 are silent -> Unhealthy; one applying sweep, then the list with room for it
  uint64_t now = T0 + STEP;
  beat_all_but(*p, now - 10, {7, 66});
  pm_mock_reset_calls();
  std::vector<GpuMatchPlugin::StatusTransition> tr = p->sweep_statuses(now);
  CHECK((take_calls() == std::vector<std::string>{"sweep now=" + std::to_string(now) + " apply=1 pool=null", "transitions cap=2"}));
  CHECK(std::string(pm_mock_calls()).empty());  // (no engine call of the plugin's own: apply is the engine's business)
  CHECK(tr.size() == 2);
  if (tr.size() == 2) {
    const bool first7 = row(*p, 7) < row(*p, 66);  // row order
    CHECK(tr[0].address == addr(first7 ? 7 : 66) && tr[1].address == addr(first7 ? 66 : 7));
    CHECK(tr[0].old_status == NodeStatus::Healthy && tr[0].new_status == NodeStatus::Unhealthy);
  }
  // intervals 2 and 3: still silent; the counter reaches the threshold -> Dead
  now += STEP;
  beat_all_but(*p, now - 10, {7, 66});
  CHECK(p->sweep_statuses(now).empty());
  now += STEP;
  beat_all_but(*p, now - 10, {7, 66});
  tr = p->sweep_statuses(now);
  CHECK(tr.size() == 2 && tr[0].old_status == NodeStatus::Unhealthy && tr[0].new_status == NodeStatus::Dead);
  CHECK(mock_liveness::status[row(*p, 7)] == PM_NS_DEAD && mock_liveness::counter[row(*p, 7)] == 3);
  take_calls();
  // the host writes statuses of its own: the ban keeps the counter (a read, then the write), the invite clears it
  banned = node(7);
  banned.status = NodeStatus::Banned;
  p->handle_status_change(banned);
  const std::string w7 = std::to_string(row(*p, 7));
  CHECK((take_calls() == std::vector<std::string>{"get w=" + w7, "set w=" + w7 + " s=6 c=3"}));
  OrchestratorNode invited = node(66);
  invited.status = NodeStatus::WaitingForHeartbeat;
  p->handle_status_change(invited);
  const std::string w66 = std::to_string(row(*p, 66));
  CHECK((take_calls() == std::vector<std::string>{"set w=" + w66 + " s=1 c=0"}));
  // interval 4: everyone beats; 66 is out of the pool (its bit, and only its bit, is clear): Waiting -> Discovered; the
  // banned node stays banned
  now += STEP;
  beat_all_but(*p, now - 10, {});
  tr = p->sweep_statuses(now, {Address(addr(66)), Address("0x00000000000000000000000000000000000000ff")});
  CHECK(tr.size() == 1 && tr[0].address == addr(66) && tr[0].old_status == NodeStatus::WaitingForHeartbeat &&
        tr[0].new_status == NodeStatus::Discovered);
  CHECK(mock_liveness::last_pool.size() == 2);
  if (mock_liveness::last_pool.size() == 2) {
    const uint32_t w = row(*p, 66);
    uint64_t want[2] = {~uint64_t(0), ~uint64_t(0)};
    want[w >> 6] &= ~(uint64_t(1) << (w & 63u));
    CHECK(mock_liveness::last_pool[0] == want[0] && mock_liveness::last_pool[1] == want[1]);
  }
  CHECK(mock_liveness::status[row(*p, 7)] == PM_NS_BANNED && mock_liveness::counter[row(*p, 7)] == 0);
  // interval 5: in the pool again -> Healthy (the revival)
  now += STEP;
  beat_all_but(*p, now - 10, {});
  tr = p->sweep_statuses(now);
  CHECK(tr.size() == 1 && tr[0].address == addr(66) && tr[0].new_status == NodeStatus::Healthy);
  for (int k = 0; k < N; ++k) CHECK(mock_liveness::status[row(*p, k)] == (k == 7 ? PM_NS_BANNED : PM_NS_HEALTHY));
}

static void a_row_beyond_the_node_table_and_an_engine_refusal() {
  auto p = make_plugin();
  p->enable_liveness(3);
  beat_all_but(*p, T0, {});
  mock_liveness::extra_row = uint32_t(N) + 5u;
  bool threw = false;
  try {
    p->sweep_statuses(T0 + 1);
  } catch (const std::out_of_range&) {
    threw = true;
  }
  CHECK(threw);
  mock_liveness::fail_with = PM_ENODEV;
  threw = false;
  try {
    p->sweep_statuses(T0 + 2);
  } catch (const EngineError& x) {
    threw = x.code() == PM_ENODEV;
  }
  CHECK(threw);
}

static void the_c_face() {
  pmx_plugin h;
  h.plugin = make_plugin();
  size_t need = 0;
  CHECK(pmx_sweep_statuses(&h, T0, nullptr, 0, nullptr, 0, &need) == -1 && std::string(pmx_last_error()).size() > 0);  // off
  CHECK(pmx_enable_liveness(&h, 2) == 0 && mock_liveness::on && mock_liveness::m == 2);
  for (int k = 0; k < N; ++k)
    if (k != 9) CHECK(pmx_beat(&h, addr(k).c_str(), T0) == 0);
  take_calls();
  CHECK(pmx_sweep_statuses(&h, T0 + 5, nullptr, 0, nullptr, 0, &need) == 0 && need > 0);  // the size query sweeps once ...
  std::string small(need - 1, '\0'), buf(need, '\0');
  size_t need2 = 0;
  CHECK(pmx_sweep_statuses(&h, T0 + 5, nullptr, 0, small.data(), small.size(), &need2) == -2 && need2 == need);  // ... held ...
  CHECK(pmx_sweep_statuses(&h, T0 + 5, nullptr, 0, buf.data(), buf.size(), &need2) == 0);                        // ... handed over
  CHECK(take_calls().size() == 2);  // one sweep, one list
  buf.resize(need - 1);
  CHECK(buf == addr(9) + "\t2\t3\n");
  const std::string outside = addr(9);
  const char* out_of_pool[1] = {outside.c_str()};
  CHECK(pmx_beat(&h, addr(9).c_str(), T0 + 10) == 0);
  std::string next(256, '\0');
  CHECK(pmx_sweep_statuses(&h, T0 + 20, out_of_pool, 1, next.data(), next.size(), &need) == 0);
  CHECK(std::string(next.c_str()) == addr(9) + "\t3\t0\n");  // Unhealthy, a beat, not in the pool -> Discovered
}

static void beats_race_the_sweep_and_the_node_sync() {
  auto p = make_plugin();
  p->enable_liveness(3);
  const int GROWN = N + 60;
  std::atomic<bool> stop{false};
  std::atomic<uint64_t> clock{T0};
  std::vector<std::thread> beaters;
  for (int t = 0; t < 4; ++t)
    beaters.emplace_back([&, t] {
      uint32_t x = 12345u + uint32_t(t);
      while (!stop.load()) {
        x = x * 1664525u + 1013904223u;
        p->beat(Address(addr(int((x >> 8) % uint32_t(GROWN)))), clock.load());  // (some of them not in the table yet)
      }
    });
  std::thread syncer([&] {
    for (int n = N + 1; n <= GROWN; ++n) {
      p->sync_nodes(snapshot(n));
      mock_liveness::W = uint32_t(n);  // (behind the sync: never more rows than the node table holds)
    }
  });
  size_t listed = 0;
  for (int k = 0; k < 200; ++k) listed += p->sweep_statuses(clock.fetch_add(STEP) + STEP).size();
  syncer.join();
  stop = true;
  for (std::thread& b : beaters) b.join();
  CHECK(p->known_nodes() == size_t(GROWN) && mock_liveness::W.load() == uint32_t(GROWN));
  // a quiet end: everyone beats, two sweeps later every node is Healthy whatever the race left behind
  const uint64_t now = clock.load() + STEP;
  for (int k = 0; k < GROWN; ++k) p->beat(Address(addr(k)), now);
  p->sweep_statuses(now);
  CHECK(p->sweep_statuses(now + 1).empty());
  for (int k = 0; k < GROWN; ++k) CHECK(mock_liveness::status[row(*p, k)] == PM_NS_HEALTHY && mock_liveness::counter[row(*p, k)] == 0);
  std::printf("  (race: %zu transitions listed over 200 sweeps)\n", listed);
}

int main() {
  the_call_sequence_and_the_statuses_it_ends_on();
  a_row_beyond_the_node_table_and_an_engine_refusal();
  the_c_face();
  beats_race_the_sweep_and_the_node_sync();
  std::printf("4 tests, %d failed checks\n", g_failed);
  return g_failed ? 1 : 0;
}
