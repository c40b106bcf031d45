// pm_plugin_taskdir_c.cpp — see pm_plugin_c.h "task directory": the C face of GpuMatchPlugin's task directory methods.  (A file
// of its own: pm_plugin_c.cpp is also linked against a mock engine that has not this export.)
#include <string>
#include <vector>

#include "pm_plugin_c.h"
#include "pm_plugin_c_internal.hpp"

using namespace orchestrator;

namespace {
template <typename F>
int32_t guarded(F&& f) {
  try {
    return f();
  } catch (const std::exception& e) {
    pmx_detail::set_error(e.what());
    return -1;
  }
}
std::string task_lines(const std::vector<GpuMatchPlugin::ListedTask>& tasks) {
  static const char* const serve[PM_TKS_N] = {"running", "waiting", "starved"};
  static const char* const rollout[PM_TKR_N] = {"unheld", "converged", "rolling"};
  std::string text;
  for (const auto& t : tasks) {
    uint32_t reporters = 0;
    for (uint32_t s = 0; s < PM_TS_N; ++s) reporters += t.row.reporters[s];
    text += t.id + "\t" + t.name + "\t" + (t.serve < PM_TKS_N ? serve[t.serve] : "-") + "\t" +
            (t.rollout < PM_TKR_N ? rollout[t.rollout] : "-") + "\t" + std::to_string(t.row.groups_allowed) + "\t" +
            std::to_string(t.row.groups_running) + "\t" + std::to_string(t.row.workers_running) + "\t" +
            std::to_string(t.row.groups_converged) + "\t" + std::to_string(t.row.converged) + "\t" + std::to_string(reporters) + "\n";
  }
  return text;
}
}  // namespace

extern "C" {

int32_t pmx_list_tasks(pmx_plugin* p, uint64_t config_mask, uint32_t serve_mask, uint32_t rollout_mask, uint32_t workers_min,
                       uint32_t workers_max, uint32_t order, uint32_t offset, uint32_t limit, char* out, size_t cap, size_t* needed) {
  return guarded([&] {
    const GpuMatchPlugin::TaskFilter f{config_mask, serve_mask, rollout_mask, workers_min, workers_max};
    const GpuMatchPlugin::TaskListing l = p->plugin->list_tasks(f, order, offset, limit);
    const std::string text = "total\t" + std::to_string(l.total) + "\t" + std::to_string(l.totals.tasks) + "\n" + task_lines(l.tasks);
    return pmx_detail::give_text(text, out, cap, needed);
  });
}

int32_t pmx_task_counts(pmx_plugin* p, char* out, size_t cap, size_t* needed) {
  return guarded([&] {
    const GpuMatchPlugin::TaskCounts c = p->plugin->task_counts();
    const pm_tdir_totals& t = c.totals;
    std::string text = "tasks\t" + std::to_string(t.tasks) + "\nserve";
    for (uint32_t k = 0; k < PM_TKS_N; ++k) text += "\t" + std::to_string(t.by_serve[k]);
    text += "\nrollout";
    for (uint32_t k = 0; k < PM_TKR_N; ++k) text += "\t" + std::to_string(t.by_rollout[k]);
    text += "\nunrestricted\t" + std::to_string(t.unrestricted) + "\nworkers_running\t" + std::to_string(t.workers_running) +
            "\nreporters\t" + std::to_string(t.reporters) + "\norphans\t" + std::to_string(t.orphan_uids) + "\t" +
            std::to_string(t.orphan_reporters) + "\n";
    for (const auto& kv : c.by_config) text += kv.first + "\t" + std::to_string(kv.second) + "\n";
    return pmx_detail::give_text(text, out, cap, needed);
  });
}

int32_t pmx_starved_tasks(pmx_plugin* p, char* out, size_t cap, size_t* needed) {
  return guarded([&] { return pmx_detail::give_text(task_lines(p->plugin->starved_tasks()), out, cap, needed); });
}

int32_t pmx_orchestrator_statistics(pmx_plugin* p, char* out, size_t cap, size_t* needed) {
  return guarded([&] {
    const GpuMatchPlugin::OrchestratorStatistics s = p->plugin->orchestrator_statistics();
    std::string text;
    for (const auto& kv : s.nodes_by_status) text += "nodes\t" + kv.first + "\t" + std::to_string(kv.second) + "\n";
    text += "tasks_count\t" + std::to_string(s.tasks_count) + "\n";
    for (const auto& n : s.nodes_per_task) text += "nodes_per_task\t" + n.task_id + "\t" + n.task_name + "\t" + std::to_string(n.count) + "\n";
    for (const auto& kv : s.groups_count) text += "groups_count\t" + kv.first + "\t" + std::to_string(kv.second) + "\n";
    return pmx_detail::give_text(text, out, cap, needed);
  });
}

}  // extern "C"
