// gpu_match_taskdir.cpp — GpuMatchPlugin::list_tasks / task_counts / starved_tasks / orchestrator_statistics (see
// gpu_match_plugin.hpp): the engine's task directory (pm_task_directory) with the plugin's own ids and names.  The twin of the
// same methods of rust/gpu_match_plugin.rs, statement for statement.  (A file of its own: the plugin's other methods are also
// linked against a mock engine that has not this export.)
#include <algorithm>
#include <shared_mutex>
#include <stdexcept>

#include "gpu_match_plugin.hpp"

namespace orchestrator {

// one window of the task directory (the node and task locks are held: LOCK ORDER nodes, tasks, the engine).  The COUNTERS-ONLY
// query first (limit 0: no sort, no row): its total sizes the buffer — the window has min(limit, total - offset) rows — and ONE
// call behind it makes the order and the window.  by_config: PM_MAX_CONFIGS words or nullptr.
GpuMatchPlugin::TaskWindow GpuMatchPlugin::task_directory_locked(const pm_tdir_query& q, uint32_t* by_config) const {
  TaskWindow w;
  pm_tdir_query counters = q;
  counters.limit = 0u;
  uint32_t have = 0;
  check(pm_task_directory(engine_, &counters, &w.totals, by_config, by_config ? uint32_t(PM_MAX_CONFIGS) : 0u, nullptr, 0u, &have));
  have = q.offset >= w.totals.total ? 0u : std::min(q.limit, w.totals.total - q.offset);
  if (!have) return w;
  w.rows.resize(have);
  uint32_t got = 0;
  check(pm_task_directory(engine_, &q, &w.totals, by_config, by_config ? uint32_t(PM_MAX_CONFIGS) : 0u, w.rows.data(),
                          uint32_t(w.rows.size()), &got));
  if (got > w.rows.size()) throw std::out_of_range("task directory: the window grew between two calls");
  w.rows.resize(got);
  for (const pm_tdir_row& r : w.rows)
    if (r.task >= tasks_.size()) throw std::out_of_range("task directory: the engine names a task the plugin has not");
  return w;
}

std::vector<GpuMatchPlugin::ListedTask> GpuMatchPlugin::listed_tasks_locked(const TaskWindow& w) const {
  std::vector<ListedTask> out;
  out.reserve(w.rows.size());
  for (const pm_tdir_row& r : w.rows) {
    ListedTask t;
    t.id = tasks_[r.task].id;
    t.name = tasks_[r.task].name;
    t.serve = r.serve;
    t.rollout = r.rollout;
    t.row = r;
    out.push_back(std::move(t));
  }
  return out;
}

GpuMatchPlugin::TaskListing GpuMatchPlugin::list_tasks(const TaskFilter& f, uint32_t order, uint32_t offset, uint32_t limit) const {
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);
  std::shared_lock<std::shared_mutex> tasks(tasks_mu_);
  const pm_tdir_query q{f.config_mask, f.serve_mask, f.rollout_mask, f.workers_min, f.workers_max, order, offset, limit, 0u};
  const TaskWindow w = task_directory_locked(q, nullptr);
  TaskListing out;
  out.total = w.totals.total;
  out.totals = w.totals;
  out.tasks = listed_tasks_locked(w);
  return out;
}

GpuMatchPlugin::TaskCounts GpuMatchPlugin::task_counts() const {
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);
  std::shared_lock<std::shared_mutex> tasks(tasks_mu_);
  const pm_tdir_query q{~0ull, (1u << PM_TKS_N) - 1u, (1u << PM_TKR_N) - 1u, 0u, 0xFFFFFFFFu, PM_TDIR_BY_LIST, 0u, 0u, 0u};  // the counters alone
  uint32_t by_config[PM_MAX_CONFIGS] = {};
  const TaskWindow w = task_directory_locked(q, by_config);
  if (w.totals.n_cfgs > config_names_.size()) throw std::out_of_range("task directory: the engine counts a configuration the plugin has not");
  TaskCounts out;
  out.totals = w.totals;
  for (uint32_t c = 0; c < w.totals.n_cfgs; ++c)
    if (by_config[c]) out.by_config[config_names_[c]] += by_config[c];  // (a name no task allows is not set)
  return out;
}

std::vector<GpuMatchPlugin::ListedTask> GpuMatchPlugin::starved_tasks() const {
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);
  std::shared_lock<std::shared_mutex> tasks(tasks_mu_);
  const pm_tdir_query q{~0ull, 1u << PM_TKS_STARVED, (1u << PM_TKR_N) - 1u, 0u, 0xFFFFFFFFu, PM_TDIR_BY_LIST, 0u, 0xFFFFFFFFu, 0u};
  return listed_tasks_locked(task_directory_locked(q, nullptr));
}

GpuMatchPlugin::OrchestratorStatistics GpuMatchPlugin::orchestrator_statistics() {
  OrchestratorStatistics out;
  out.nodes_by_status = status_counts();         // sync_service.rs:209-225: the node directory's counters
  out.tasks_count = task_counts().totals.tasks;  // :228-241: the task directory's
  out.nodes_per_task = nodes_per_task();         // :243-267: the rollout task table (it flushes the queued reports first)
  out.groups_count = group_counts();             // :272-286: the group directory's
  return out;
}

}  // namespace orchestrator
