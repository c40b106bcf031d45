// spread_test.cpp — GpuMatchPlugin::group_spread / configuration_spread / force_regroup
// (protocol_amd/plugin/gpu_match_spread.cpp) against tests/cpp/mock_engine.cpp + tests/cpp/mock_spread.cpp: every group's row
// lands under its "{:x}" id text with node addresses for worker rows, every field of a configuration row under the
// configuration's name, force_regroup resolves the name (an unknown one is nullopt and asks the engine nothing), delivers the
// destroyed webhooks in id-text order, and an engine refusal is thrown as EngineError.
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "gpu_match_plugin.hpp"
#include "group_id_text.hpp"

namespace mock_spread {
struct Asked {
  uint32_t config, metric;
  double threshold_km;
};
extern uint32_t n_cfgs;
extern int32_t fail_with;
extern std::vector<Asked> regroups;
double diameter_of(uint64_t id);
}  // namespace mock_spread

using namespace orchestrator;

static int g_failed = 0;
#define CHECK(cond)                                                                      \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      std::fprintf(stderr, "  CHECK failed at %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                                        \
    }                                                                                    \
  } while (0)

struct Hook : WebhookPlugin {
  std::vector<std::string> created, destroyed;  // group id texts, in delivery order
  std::vector<std::string> destroyed_cfg;
  void send_group_created(const std::string& id, const std::string&, const std::vector<std::string>&) override { created.push_back(id); }
  void send_group_destroyed(const std::string& id, const std::string& name, const std::vector<std::string>&) override {
    destroyed.push_back(id);
    destroyed_cfg.push_back(name);
  }
};

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
static Task task(int k, int64_t created, const char* topology) {
  Task t;
  t.allowed_topologies = std::vector<std::string>{topology};
  char id[40];
  std::snprintf(id, sizeof(id), "00000000-0000-4000-8000-%012x", 0x3000 + k);
  t.id = id;
  t.name = "task-" + std::to_string(k);
  t.image = "image";
  t.created_at = created;
  return t;
}

struct Rig {
  std::shared_ptr<Hook> hook = std::make_shared<Hook>();
  std::unique_ptr<GpuMatchPlugin> plugin;
};
// 23 nodes, pairs and solos: the mock's tick forms one group per configuration and pass until nobody is free
static Rig make_rig() {
  Rig r;
  std::vector<NodeGroupConfiguration> cfgs = {{"pair", 2, 2, std::nullopt}, {"solo", 1, 1, std::nullopt}};
  r.plugin = std::make_unique<GpuMatchPlugin>(cfgs, 0, nullptr, std::vector<std::shared_ptr<WebhookPlugin>>{r.hook});
  std::vector<OrchestratorNode> snap;
  for (int k = 0; k < 23; ++k) snap.push_back(node(k));
  r.plugin->sync_nodes(snap);
  r.plugin->sync_tasks({task(1, 200, "pair"), task(0, 100, "solo")});
  mock_spread::n_cfgs = 2;
  mock_spread::fail_with = PM_OK;
  mock_spread::regroups.clear();
  r.plugin->tick();
  return r;
}
static uint64_t id_of(const std::string& text) {
  uint64_t v = 0;
  CHECK(parse_group_id(text, &v));
  return v;
}

static void group_rows_by_id_text() {
  Rig r = make_rig();
  const std::vector<NodeGroup> groups = r.plugin->get_all_groups();
  CHECK(groups.size() >= 10);
  const auto m = r.plugin->group_spread();
  CHECK(m.size() == groups.size());
  for (const NodeGroup& g : groups) {
    const auto it = m.find(g.id);
    CHECK(it != m.end());
    if (it == m.end()) continue;
    const GpuMatchPlugin::GroupSpread& s = it->second;
    CHECK(s.located == g.nodes.size());
    if (g.nodes.size() > 1) {
      CHECK(s.ring_hops == g.nodes.size());
      CHECK(s.far_a == g.nodes.front() && s.far_b == g.nodes.back() && s.hop_from == g.nodes[1]);  // addresses, group.nodes order
      CHECK(s.diameter_km == mock_spread::diameter_of(id_of(g.id)));
      CHECK(s.ring_km == 2.0 * s.diameter_km && s.longest_hop_km == 0.5 * s.diameter_km);
    } else {
      CHECK(s.ring_hops == 0 && s.far_a.empty() && s.far_b.empty() && s.hop_from.empty() && s.diameter_km == 0.0);
    }
  }
}

static void configuration_rows_by_name() {
  Rig r = make_rig();
  const auto rows = r.plugin->configuration_spread();
  CHECK(rows.size() == 2);
  const std::vector<std::string> names = {"pair", "solo"};
  for (uint32_t c = 0; c < rows.size() && c < 2; ++c) {
    const auto& o = rows[c];
    CHECK(o.name == names[c]);
    CHECK(o.groups == 100 + c && o.measured == 90 + c);
    for (uint32_t k = 0; k < PM_SPREAD_BUCKETS; ++k) CHECK(o.hist[k] == 10 * c + k);
    CHECK(o.max_diameter_km == 1000.5 + c && o.max_hop_km == 500.25 + c);
    CHECK(o.sum_diameter_m == 7000000000ull + c && o.sum_ring_m == 9000000000ull + c);
  }
}

static void force_regroup_by_name_and_webhook_order() {
  Rig r = make_rig();
  const std::vector<NodeGroup> before = r.plugin->get_all_groups();  // id-text order (mod.rs:1040)
  std::vector<std::string> pairs, solos;
  for (const NodeGroup& g : before) (g.configuration_name == "pair" ? pairs : solos).push_back(g.id);
  CHECK(pairs.size() >= 4 && !solos.empty());
  if (pairs.size() < 4 || solos.empty()) return;
  CHECK(std::is_sorted(pairs.begin(), pairs.end()));
  std::vector<uint64_t> numeric;
  for (const std::string& t : pairs) numeric.push_back(id_of(t));
  // an unknown name: the route's 404, the engine is not asked
  CHECK(!r.plugin->force_regroup("trio").has_value());
  CHECK(mock_spread::regroups.empty() && r.hook->destroyed.empty());
  // by diameter: the pairs at or above the median, in id-text order
  std::vector<double> d;
  for (uint64_t id : numeric) d.push_back(mock_spread::diameter_of(id));
  std::sort(d.begin(), d.end());
  const double thr = d[d.size() / 2];
  std::vector<std::string> want;
  for (const std::string& t : pairs)
    if (mock_spread::diameter_of(id_of(t)) >= thr) want.push_back(t);
  auto got = r.plugin->force_regroup("pair", PM_REGROUP_DIAMETER, thr);
  CHECK(got.has_value() && got->dissolved_groups == want.size() && got->affected_nodes == 2 * want.size());
  CHECK(mock_spread::regroups.size() == 1 && mock_spread::regroups[0].config == 0 &&
        mock_spread::regroups[0].metric == PM_REGROUP_DIAMETER && mock_spread::regroups[0].threshold_km == thr);
  CHECK(r.hook->destroyed == want);
  for (const std::string& name : r.hook->destroyed_cfg) CHECK(name == "pair");
  CHECK(r.plugin->get_all_groups().size() == before.size() - want.size());
  // the route as the reference has it: every group of the configuration
  r.hook->destroyed.clear();
  got = r.plugin->force_regroup("solo");
  CHECK(got.has_value() && got->dissolved_groups == solos.size() && got->affected_nodes == solos.size());
  CHECK(mock_spread::regroups.size() == 2 && mock_spread::regroups[1].config == 1 && mock_spread::regroups[1].metric == PM_REGROUP_ALL);
  CHECK(r.hook->destroyed == solos);
  for (const NodeGroup& g : r.plugin->get_all_groups()) CHECK(g.configuration_name == "pair");
  // nothing selected: no webhook
  r.hook->destroyed.clear();
  got = r.plugin->force_regroup("solo");
  CHECK(got.has_value() && got->dissolved_groups == 0 && got->affected_nodes == 0 && r.hook->destroyed.empty());
}

static void refusals_are_engine_errors() {
  Rig r = make_rig();
  int thrown = 0;
  try {
    r.plugin->force_regroup("pair", 7, 0.0);
  } catch (const EngineError& e) {
    thrown += e.code() == PM_EINVAL;
  }
  try {
    r.plugin->force_regroup("pair", PM_REGROUP_LONGEST_HOP, -1.0);
  } catch (const EngineError& e) {
    thrown += e.code() == PM_EINVAL;
  }
  CHECK(thrown == 2 && r.hook->destroyed.empty());
  mock_spread::fail_with = PM_ESTATE;
  try {
    r.plugin->group_spread();
  } catch (const EngineError& e) {
    thrown += e.code() == PM_ESTATE;
  }
  try {
    r.plugin->configuration_spread();
  } catch (const EngineError& e) {
    thrown += e.code() == PM_ESTATE;
  }
  try {
    r.plugin->force_regroup("pair");
  } catch (const EngineError& e) {
    thrown += e.code() == PM_ESTATE;
  }
  CHECK(thrown == 5);
  mock_spread::fail_with = PM_OK;
}

int main() {
  const std::pair<const char*, void (*)()> tests[] = {{"group_rows_by_id_text", group_rows_by_id_text},
                                                      {"configuration_rows_by_name", configuration_rows_by_name},
                                                      {"force_regroup_by_name_and_webhook_order", force_regroup_by_name_and_webhook_order},
                                                      {"refusals_are_engine_errors", refusals_are_engine_errors}};
  int n = 0;
  for (const auto& t : tests) {
    const int before = g_failed;
    t.second();
    std::printf("%s  %s\n", g_failed == before ? "ok" : "FAIL", t.first);
    ++n;
  }
  std::printf("%d tests, %d failed checks\n", n, g_failed);
  return g_failed ? 1 : 0;
}
