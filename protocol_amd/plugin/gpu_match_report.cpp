// gpu_match_report.cpp — GpuMatchPlugin::explain_node / configuration_report / task_report (see gpu_match_plugin.hpp): the
// engine's diagnostics reports (pm_explain_workers, pm_config_report, pm_task_report) by node address, configuration name and
// task id.  The twin of the same three methods of rust/gpu_match_plugin.rs, statement for statement.  (A file of its own: the
// plugin's other methods are also linked against a mock engine that has none of these exports.)
#include <shared_mutex>

#include "gpu_match_plugin.hpp"

namespace orchestrator {

const char* GpuMatchPlugin::why_name(uint32_t code) {
  static const char* const names[PM_WHY_N] = {"ok",       "no_specs",  "cpu",       "ram",     "storage",
                                               "gpu_none", "gpu_count", "gpu_model", "gpu_mem", "gpu_total"};
  return code < PM_WHY_N ? names[code] : "unknown";
}

const char* GpuMatchPlugin::state_name(uint32_t state) {
  switch (state) {
    case PM_WS_IN_GROUP: return "in_group";
    case PM_WS_UNHEALTHY: return "unhealthy";
    case PM_WS_NO_P2P: return "no_p2p";
    case PM_WS_IDLE: return "idle";
    default: return "unknown";
  }
}

std::optional<GpuMatchPlugin::NodeExplanation> GpuMatchPlugin::explain_node(const std::string& address) const {
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);  // (LOCK ORDER: nodes, the engine)
  const std::optional<uint32_t> row = row_of_address_text(nodes_, address);
  if (!row) return std::nullopt;
  std::vector<uint8_t> why(config_names_.size());
  uint32_t state = 0;
  check(pm_explain_workers(engine_, &*row, 1, why.empty() ? nullptr : why.data(), &state));
  NodeExplanation out;
  out.state = state_name(state);
  for (size_t c = 0; c < why.size(); ++c) out.configs.emplace_back(config_names_[c], why_name(why[c]));
  return out;
}

std::vector<GpuMatchPlugin::ConfigurationReport> GpuMatchPlugin::configuration_report() const {
  std::vector<pm_config_report_row> rows(config_names_.size());
  uint32_t n = 0;
  check(pm_config_report(engine_, rows.empty() ? nullptr : rows.data(), uint32_t(rows.size()), &n));
  std::vector<ConfigurationReport> out;
  for (uint32_t c = 0; c < n && c < rows.size(); ++c) {
    const pm_config_report_row& r = rows[c];
    ConfigurationReport o;
    o.name = config_names_[c];
    o.enabled = r.enabled != 0;
    o.eligible_meets = r.eligible_meets;
    o.idle_meets = r.idle_meets;
    for (size_t k = 0; k < o.why.size(); ++k) o.why[k] = r.why[k];
    o.groups = r.groups;
    o.members = r.members;
    o.groups_without_task = r.groups_without_task;
    o.tasks_allowing = r.tasks_allowing;
    out.push_back(std::move(o));
  }
  return out;
}

std::unordered_map<std::string, GpuMatchPlugin::TaskReport> GpuMatchPlugin::task_report() const {
  std::shared_lock<std::shared_mutex> tasks(tasks_mu_);  // (the engine's positions index tasks_)
  const size_t T = tasks_.size();
  std::vector<uint32_t> running(T), workers(T), allowed(T);
  check(pm_task_report(engine_, T ? running.data() : nullptr, T ? workers.data() : nullptr, T ? allowed.data() : nullptr));
  std::unordered_map<std::string, TaskReport> out;
  out.reserve(T);
  for (size_t i = 0; i < T; ++i) out[tasks_[i].id] = TaskReport{running[i], workers[i], allowed[i]};
  return out;
}

}  // namespace orchestrator
