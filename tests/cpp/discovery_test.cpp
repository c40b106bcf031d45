// discovery_test.cpp — GpuMatchPlugin::set_endpoint / sync_discovery (protocol_amd/plugin/gpu_match_discovery.cpp) and their C
// face (pm_plugin_discovery_c.cpp) against tests/cpp/mock_engine.cpp + mock_liveness.cpp + mock_discovery.cpp: the interning (one
// id per "ip:port", "discovery ip : stored port" for endpoint_after, never more ids than the engine accepts), the column and the
// rows the plugin hands over, the stamps it supplies, the endpoint column after rewrites and put-backs, admitted nodes and their
// remembered endpoints, an engine refusal, and sync_discovery racing beat, handle_status_change and sweep_statuses.
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
namespace mock_discovery {
extern std::vector<uint32_t> last_column;
extern std::vector<pm_disc_row> last_rows;
extern uint32_t last_n_endpoints;
extern int32_t fail_with;
}  // namespace mock_discovery

using namespace orchestrator;
using Sighting = GpuMatchPlugin::DiscoverySighting;
using Kind = GpuMatchPlugin::DiscoveryOutcome::Kind;

static int g_failed = 0;
#define CHECK(cond)                                                                      \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      std::fprintf(stderr, "  CHECK failed at %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                                        \
    }                                                                                    \
  } while (0)

static const int N = 70;
static const uint64_t T0 = 1760000000000ull;
static std::string addr(int k) {
  char s[48];
  std::snprintf(s, sizeof(s), "0x%040x", 0x700 + k * 3);
  return s;
}
static std::string ip(int k) { return "10.0." + std::to_string(k / 200) + "." + std::to_string(k % 200); }
static OrchestratorNode node(int k, NodeStatus s = NodeStatus::Healthy) {
  OrchestratorNode n;
  n.address = Address(addr(k));
  n.status = s;
  n.p2p_id = "p2p-" + std::to_string(k);
  return n;
}
static std::vector<OrchestratorNode> snapshot(int n) {
  std::vector<OrchestratorNode> snap;
  for (int k = 0; k < n; ++k) snap.push_back(node(k));
  return snap;
}
static Sighting seen(int k, const std::string& at, uint16_t port = 8080) {
  Sighting s;
  s.address = Address(addr(k));
  s.ip_address = at;
  s.port = port;
  s.is_validated = s.is_provider_whitelisted = s.is_active = true;
  return s;
}

// N Healthy nodes, node k on ip(k):8080, liveness on
static std::shared_ptr<GpuMatchPlugin> make_plugin() {
  std::vector<NodeGroupConfiguration> cfgs = {{"pair", 2, 2, std::nullopt}, {"solo", 1, 1, std::nullopt}};
  auto p = std::make_shared<GpuMatchPlugin>(cfgs, 0, nullptr, std::vector<std::shared_ptr<WebhookPlugin>>{});
  p->clock = [] { return int64_t(T0 - 1000000); };
  p->sync_nodes(snapshot(N));
  {
    std::lock_guard<std::mutex> lk(mock_liveness::mu);
    mock_liveness::on = false;
    mock_liveness::m = mock_liveness::enables = 0;
    mock_liveness::W = uint32_t(N);
    mock_liveness::fail_with = mock_discovery::fail_with = PM_OK;
    mock_liveness::status.clear(), mock_liveness::counter.clear(), mock_liveness::calls.clear(), mock_liveness::last_pool.clear();
    mock_liveness::extra_row = PM_NONE;
  }
  p->enable_liveness(3);
  for (int k = 0; k < N; ++k) p->set_endpoint(Address(addr(k)), ip(k), 8080);
  return p;
}
static uint32_t row(const GpuMatchPlugin& p, int k) {
  const std::optional<uint32_t> r = p.row_of(Address(addr(k)));
  CHECK(r.has_value());
  return r.value_or(PM_NONE);
}
static void set_status(GpuMatchPlugin& p, int k, NodeStatus s) { p.handle_status_change(node(k, s)); }
static bool at(const GpuMatchPlugin& p, int k, const std::string& want_ip, uint16_t want_port) {
  const auto e = p.endpoint_of(Address(addr(k)));
  return e.has_value() && e->first == want_ip && e->second == want_port;
}

static void interning_and_what_the_engine_is_handed() {
  auto p = make_plugin();
  CHECK(at(*p, 3, ip(3), 8080) && !p->endpoint_of(Address(addr(N + 1))).has_value());
  set_status(*p, 5, NodeStatus::Dead);  // (stamps node 5 with the plugin's clock)
  CHECK(p->last_status_change_ms(Address(addr(5))) == T0 - 1000000 && p->last_status_change_ms(Address(addr(6))) == 0);
  std::vector<Sighting> list = {seen(3, ip(3)), seen(4, ip(3), 9090), seen(N + 1, ip(3)), seen(5, ip(5))};
  list[1].is_provider_whitelisted = false;
  list[1].location_new = true;
  list[3].last_updated_ms = T0 - 5;
  list[3].specs_differ = list[3].balance_zero = true;
  const auto out = p->sync_discovery(T0, list, 1);
  const auto& rows = mock_discovery::last_rows;
  const auto& col = mock_discovery::last_column;
  CHECK(rows.size() == 4 && col.size() == size_t(N) && mock_discovery::last_n_endpoints <= uint32_t(N) + 8u);
  CHECK(mock_liveness::calls.back() == "discovery now=" + std::to_string(T0) + " rows=4 max=1 apply=1");
  // one id per "ip:port": node 3 keeps its endpoint, node 4 is seen at ip(3):9090 and would hold ip(3):8080 (its stored port)
  CHECK(rows[0].row == row(*p, 3) && rows[0].endpoint == col[row(*p, 3)] && rows[0].endpoint_after == rows[0].endpoint);
  CHECK(rows[1].row == row(*p, 4) && rows[1].endpoint != rows[0].endpoint && rows[1].endpoint_after == rows[0].endpoint);
  CHECK(rows[1].flags == (PM_DF_VALIDATED | PM_DF_ACTIVE | PM_DF_LOCATION_NEW));
  CHECK(rows[2].row == PM_DISC_NEW && rows[2].endpoint == rows[0].endpoint && rows[2].flags == 7u);
  CHECK(rows[3].flags == (7u | PM_DF_SPECS_DIFFER | PM_DF_BALANCE_ZERO) && rows[3].last_change_ms == T0 - 1000000 &&
        rows[3].last_updated_ms == T0 - 5 && rows[0].last_change_ms == 0);
  for (int k = 0; k < N; ++k)
    for (int j = 0; j < k; ++j) CHECK(col[row(*p, k)] != col[row(*p, j)] && col[row(*p, k)] < mock_discovery::last_n_endpoints);
  // outcomes: 3 untouched; 4 Ejected, then put back Healthy on ip(3) (two Healthy nodes there now); the new node skipped (two
  // Healthy nodes on ip(3):8080 when its turn came: node 3, and node 4, which had just moved there); 5: Dead -> specs put-back -> Discovered ->
  // LowBalance
  CHECK(out.size() == 4 && out[0].kind == Kind::Synced && out[0].updates.empty() && out[0].healthy_same_endpoint == 0);
  CHECK(out[1].final_status == NodeStatus::Healthy && out[1].updates.size() == 1 && out[1].updates[0].second == NodeStatus::Ejected &&
        out[1].ip_rewritten && out[1].location_new && !out[1].stamped_now);
  CHECK(out[2].kind == Kind::Skipped && out[2].healthy_same_endpoint == 2 && out[2].address == addr(N + 1));
  CHECK(out[3].final_status == NodeStatus::LowBalance && out[3].updates.size() == 2 && out[3].specs_rewritten && out[3].stamped_now);
  CHECK(at(*p, 4, ip(3), 8080) && at(*p, 5, ip(5), 8080));
  CHECK(p->last_status_change_ms(Address(addr(4))) == 0 && p->last_status_change_ms(Address(addr(5))) == T0);
  CHECK(mock_liveness::status[row(*p, 4)] == PM_NS_HEALTHY && mock_liveness::status[row(*p, 5)] == PM_NS_LOWBALANCE);
}

static void the_endpoint_column_after_rewrites_and_put_backs() {
  auto p = make_plugin();
  set_status(*p, 8, NodeStatus::Dead);
  // 7: Healthy, ip moves, port differs too (not rewritten); 8: Dead, ip and specs change -> the old ip stays; 9: port only
  std::vector<Sighting> list = {seen(7, "172.16.0.7", 9999), seen(8, "172.16.0.8"), seen(9, ip(9), 8081)};
  list[1].specs_differ = true;
  list[1].last_updated_ms = T0;
  auto out = p->sync_discovery(T0 + 1, list, 1);
  CHECK(out[0].ip_rewritten && at(*p, 7, "172.16.0.7", 8080));
  CHECK(out[1].ip_rewritten && out[1].specs_rewritten && out[1].final_status == NodeStatus::Discovered && at(*p, 8, ip(8), 8080));
  CHECK(!out[2].ip_rewritten && at(*p, 9, ip(9), 8080));
  // the next pass counts 7 where it is now: a new node on its new endpoint is skipped, one on its old endpoint admitted
  out = p->sync_discovery(T0 + 2, {seen(N + 2, "172.16.0.7", 8080), seen(N + 3, ip(7), 8080)}, 1);
  CHECK(out[0].kind == Kind::Skipped && out[1].kind == Kind::Admitted);
  CHECK(mock_discovery::last_column[row(*p, 7)] == mock_discovery::last_rows[0].endpoint);
  // many moves: the ids of endpoints nobody holds any more never exceed what the engine accepts
  for (int k = 0; k < 400; ++k) {
    out = p->sync_discovery(T0 + 10 + uint64_t(k), {seen(7, "172.17." + std::to_string(k / 200) + "." + std::to_string(k % 200))}, 1);
    CHECK(out.size() == 1 && out[0].ip_rewritten && mock_discovery::last_n_endpoints <= uint32_t(N) + 2u);
  }
  CHECK(at(*p, 7, "172.17.1.199", 8080));
  out = p->sync_discovery(T0 + 999, {seen(N + 4, "172.17.1.199", 8080), seen(N + 5, ip(12), 8080)}, 1);
  CHECK(out[0].kind == Kind::Skipped && out[1].kind == Kind::Skipped);  // (the column survived the re-interning)
}

static void admitted_nodes_and_an_engine_refusal() {
  auto p = make_plugin();
  auto out = p->sync_discovery(T0, {seen(N, "192.168.1.100"), seen(N + 1, ip(2))}, 1);
  CHECK(out[0].kind == Kind::Admitted && out[1].kind == Kind::Skipped && p->known_nodes() == size_t(N));  // returned, not appended
  p->sync_nodes(snapshot(N + 1));  // the caller added the admitted node to its store
  mock_liveness::W = uint32_t(N + 1);
  {
    std::lock_guard<std::mutex> lk(mock_liveness::mu);
    mock_liveness::status.resize(N + 1, PM_NS_DISCOVERED), mock_liveness::counter.resize(N + 1, 0u);
  }
  out = p->sync_discovery(T0 + 1, {seen(N, "192.168.1.101")}, 1);  // the reference's second test: the ip moves, Discovered stays
  CHECK(at(*p, N, "192.168.1.101", 8080) && out[0].kind == Kind::Synced && out[0].final_status == NodeStatus::Discovered);
  CHECK(mock_discovery::last_rows[0].row == row(*p, N) && mock_discovery::last_column.size() == size_t(N + 1));
  // a node that left the store is new again, and counts for nobody
  std::vector<OrchestratorNode> without = snapshot(N + 1);
  without.erase(without.begin() + 2);
  p->sync_nodes(without);
  out = p->sync_discovery(T0 + 2, {seen(N + 1, ip(2)), seen(2, ip(2))}, 1);
  CHECK(out[0].kind == Kind::Admitted && out[1].kind == Kind::Admitted && mock_discovery::last_column[row(*p, 2)] == PM_EP_NONE);
  // a refusal: EngineError, nothing moved
  mock_discovery::fail_with = PM_EINVAL;
  bool threw = false;
  try {
    p->sync_discovery(T0 + 3, {seen(4, "172.16.0.4")}, 1);
  } catch (const EngineError& x) {
    threw = x.code() == PM_EINVAL;
  }
  CHECK(threw && at(*p, 4, ip(4), 8080));
  mock_discovery::fail_with = PM_OK;
  threw = false;
  try {  // a table row listed twice is the engine's PM_EINVAL
    p->sync_discovery(T0 + 4, {seen(4, ip(4)), seen(4, ip(4))}, 1);
  } catch (const EngineError& x) {
    threw = x.code() == PM_EINVAL;
  }
  CHECK(threw);
}

static void the_c_face() {
  pmx_plugin h;
  h.plugin = make_plugin();
  const std::string a4 = addr(4), a_new = addr(N + 7), moved = "172.16.0.4", taken = ip(6);
  CHECK(pmx_set_endpoint(&h, a4.c_str(), "10.9.9.9", 8088) == 0 && at(*h.plugin, 4, "10.9.9.9", 8088));
  pmx_sighting s[2] = {};
  s[0].address = a4.c_str(), s[0].ip_address = moved.c_str(), s[0].port = 8088;
  s[0].is_validated = 1, s[0].is_active = 1, s[0].balance_zero = 1;
  s[1].address = a_new.c_str(), s[1].ip_address = taken.c_str(), s[1].port = 8080;
  s[1].is_validated = s[1].is_provider_whitelisted = s[1].is_active = 1;
  size_t need = 0, need2 = 0;
  const size_t before = mock_liveness::calls.size();
  CHECK(pmx_sync_discovery(&h, T0, s, 2, 1, nullptr, 0, &need) == 0 && need > 0);  // the size query syncs once ...
  std::string small(need - 1, '\0'), buf(need, '\0');
  CHECK(pmx_sync_discovery(&h, T0, s, 2, 1, small.data(), small.size(), &need2) == -2 && need2 == need);  // ... held ...
  CHECK(pmx_sync_discovery(&h, T0, s, 2, 1, buf.data(), buf.size(), &need2) == 0);                        // ... handed over
  CHECK(mock_liveness::calls.size() == before + 1);
  buf.resize(need - 1);
  CHECK(buf == a4 + "\tsynced\t0\t2\t7\tin\t2>5,2>7\n" + a_new + "\tskipped\t1\n");
  mock_discovery::fail_with = PM_ESTATE;
  CHECK(pmx_sync_discovery(&h, T0, s, 2, 1, nullptr, 0, &need) == -1 && std::string(pmx_last_error()).size() > 0);
  mock_discovery::fail_with = PM_OK;
}

static void the_sync_races_beats_status_changes_and_the_sweep() {
  auto p = make_plugin();
  std::atomic<bool> stop{false};
  std::vector<std::thread> others;
  for (int t = 0; t < 3; ++t)
    others.emplace_back([&, t] {
      uint32_t x = 777u + uint32_t(t);
      while (!stop.load()) {
        x = x * 1664525u + 1013904223u;
        p->beat(Address(addr(int((x >> 8) % uint32_t(N)))), T0 + (x & 1023u));
        if (t == 0 && (x & 0xF000u) == 0) set_status(*p, int((x >> 8) % uint32_t(N)), (x & 1u) ? NodeStatus::Healthy : NodeStatus::Unhealthy);
        if (t == 1 && (x & 0xFF00u) == 0) p->sweep_statuses(T0 + (x & 1023u));
        if (t == 2 && (x & 0xFF00u) == 0) p->sync_nodes(snapshot(N));
      }
    });
  size_t updates = 0;
  for (int k = 0; k < 300; ++k) {
    std::vector<Sighting> list;
    for (int j = 0; j < 20; ++j) list.push_back(seen((k * 7 + j * 3) % N, ip((k + j) % 16)));
    list.push_back(seen(N + 10 + k, ip(k % 16)));
    list[k % 20].is_active = false;
    for (const auto& o : p->sync_discovery(T0 + 2000 + uint64_t(k), list, 2)) updates += o.updates.size();
  }
  stop = true;
  for (std::thread& t : others) t.join();
  CHECK(p->known_nodes() == size_t(N) && updates > 0);
  for (int k = 0; k < N; ++k) CHECK(p->endpoint_of(Address(addr(k))).has_value());
  std::printf("  (race: %zu updates over 300 syncs)\n", updates);
}

int main() {
  interning_and_what_the_engine_is_handed();
  the_endpoint_column_after_rewrites_and_put_backs();
  admitted_nodes_and_an_engine_refusal();
  the_c_face();
  the_sync_races_beats_status_changes_and_the_sweep();
  std::printf("5 tests, %d failed checks\n", g_failed);
  return g_failed ? 1 : 0;
}
