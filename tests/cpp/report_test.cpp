// report_test.cpp — GpuMatchPlugin::explain_node / configuration_report / task_report
// (protocol_amd/plugin/gpu_match_report.cpp) against tests/cpp/mock_engine.cpp + tests/cpp/mock_report.cpp: the node's row
// goes to the engine, reasons and states come back by name per configuration in constructor order, every field of a report
// row lands in its place under the configuration's name, task positions are keyed by the task ids of the plugin's list, and
// an engine refusal is thrown as EngineError.
#include <cstdio>
#include <string>
#include <vector>

#include "gpu_match_plugin.hpp"

namespace mock_report {
extern std::vector<uint32_t> explained;
extern uint32_t n_cfgs, n_tasks, state_answer;
extern int32_t fail_with;
}  // namespace mock_report

using namespace orchestrator;

static int g_failed = 0;
#define CHECK(cond)                                                                      \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      std::fprintf(stderr, "  CHECK failed at %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                                        \
    }                                                                                    \
  } while (0)

static std::string addr(int k) {
  char s[48];
  std::snprintf(s, sizeof(s), "0x%040x", 0x200 + k * 13);
  return s;
}
static OrchestratorNode node(int k) {
  OrchestratorNode n;
  n.address = Address(addr(k));
  n.status = NodeStatus::Healthy;
  n.p2p_id = "p2p-" + std::to_string(k);
  return n;
}
static Task task(int k, int64_t created) {
  Task t;
  char id[40];
  std::snprintf(id, sizeof(id), "00000000-0000-4000-8000-%012x", 0x2000 + k);
  t.id = id;
  t.name = "task-" + std::to_string(k);
  t.image = "image";
  t.created_at = created;
  return t;
}

static std::unique_ptr<GpuMatchPlugin> make_plugin() {
  std::vector<NodeGroupConfiguration> cfgs = {{"pair", 2, 2, std::nullopt}, {"solo", 1, 1, std::nullopt}, {"quad", 1, 4, std::nullopt}};
  auto p = std::make_unique<GpuMatchPlugin>(cfgs, 0, nullptr);
  std::vector<OrchestratorNode> snap;
  for (int k = 0; k < 6; ++k) snap.push_back(node(k));
  p->sync_nodes(snap);
  p->sync_tasks({task(2, 300), task(1, 200), task(0, 100)});
  mock_report::n_cfgs = 3;
  mock_report::n_tasks = 3;
  mock_report::fail_with = PM_OK;
  return p;
}

static void explains_a_node_by_name() {
  auto p = make_plugin();
  const std::vector<std::string> names = {"pair", "solo", "quad"};
  const char* const why[PM_WHY_N] = {"ok",       "no_specs",  "cpu",       "ram",     "storage",
                                     "gpu_none", "gpu_count", "gpu_model", "gpu_mem", "gpu_total"};
  for (int k : {4, 0}) {
    mock_report::explained.clear();
    mock_report::state_answer = k == 4 ? PM_WS_NO_P2P : PM_WS_IN_GROUP;
    const auto x = p->explain_node(addr(k));
    CHECK(x.has_value());
    if (!x) return;
    CHECK(mock_report::explained.size() == 1);
    if (mock_report::explained.size() != 1) return;
    const uint32_t row = mock_report::explained[0];
    CHECK(row < 6);
    CHECK(x->state == (k == 4 ? "no_p2p" : "in_group"));
    CHECK(x->configs.size() == 3);
    for (size_t c = 0; c < x->configs.size() && c < 3; ++c) {
      CHECK(x->configs[c].first == names[c]);
      CHECK(x->configs[c].second == why[(row + c) % PM_WHY_N]);
    }
  }
  // two different nodes are two different rows
  mock_report::explained.clear();
  p->explain_node(addr(1));
  p->explain_node(addr(2));
  CHECK(mock_report::explained.size() == 2 && mock_report::explained[0] != mock_report::explained[1]);
  // an unknown address is not an error and asks the engine nothing
  mock_report::explained.clear();
  CHECK(!p->explain_node(addr(99)).has_value());
  CHECK(mock_report::explained.empty());
  CHECK(std::string(GpuMatchPlugin::state_name(PM_WS_IDLE)) == "idle" &&
        std::string(GpuMatchPlugin::state_name(PM_WS_UNHEALTHY)) == "unhealthy");
  CHECK(std::string(GpuMatchPlugin::why_name(PM_WHY_GPU_TOTAL)) == "gpu_total");
}

static void reports_configurations_by_name() {
  auto p = make_plugin();
  const auto rows = p->configuration_report();
  CHECK(rows.size() == 3);
  const std::vector<std::string> names = {"pair", "solo", "quad"};
  for (uint32_t c = 0; c < rows.size() && c < 3; ++c) {
    const auto& r = rows[c];
    CHECK(r.name == names[c]);
    CHECK(r.enabled == ((c & 1u) != 0));
    CHECK(r.eligible_meets == 100 + c && r.idle_meets == 200 + c);
    CHECK(r.groups == 300 + c && r.members == 400 + c && r.groups_without_task == 500 + c && r.tasks_allowing == 600 + c);
    CHECK(r.why[0] == r.eligible_meets);
    for (uint32_t k = 1; k < PM_WHY_N; ++k) CHECK(r.why[k] == 1000 * c + k);
  }
}

static void reports_tasks_by_id_and_refusals() {
  auto p = make_plugin();
  const auto m = p->task_report();
  CHECK(m.size() == 3);
  // the plugin's list is get_all_tasks order (created_at descending): task 2, task 1, task 0
  const int order[3] = {2, 1, 0};
  for (uint32_t pos = 0; pos < 3; ++pos) {
    const auto it = m.find(task(order[pos], 0).id);
    CHECK(it != m.end());
    if (it == m.end()) continue;
    CHECK(it->second.groups_running == pos && it->second.workers_running == 10 * pos && it->second.groups_allowed == 100 * pos);
  }
  mock_report::fail_with = PM_ESTATE;
  int thrown = 0;
  try {
    p->task_report();
  } catch (const EngineError& e) {
    thrown += e.code() == PM_ESTATE;
  }
  try {
    p->configuration_report();
  } catch (const EngineError& e) {
    thrown += e.code() == PM_ESTATE;
  }
  try {
    p->explain_node(addr(1));
  } catch (const EngineError& e) {
    thrown += e.code() == PM_ESTATE;
  }
  CHECK(thrown == 3);
  mock_report::fail_with = PM_OK;
}

int main() {
  const std::pair<const char*, void (*)()> tests[] = {{"explains_a_node_by_name", explains_a_node_by_name},
                                                      {"reports_configurations_by_name", reports_configurations_by_name},
                                                      {"reports_tasks_by_id_and_refusals", reports_tasks_by_id_and_refusals}};
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
