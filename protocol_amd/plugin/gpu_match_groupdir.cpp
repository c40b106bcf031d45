// gpu_match_groupdir.cpp — GpuMatchPlugin::list_groups / group_counts / degraded_groups (see gpu_match_plugin.hpp): the
// engine's group directory (pm_group_directory) as NodeGroup objects.  The twin of the same methods of
// rust/gpu_match_plugin.rs, statement for statement.  (A file of its own: the plugin's other methods are also linked against a
// mock engine that has not this export.)
#include <algorithm>
#include <shared_mutex>
#include <stdexcept>

#include "group_id_text.hpp"
#include "gpu_match_plugin.hpp"

namespace orchestrator {

// one window of the group directory (the node and task locks are held: LOCK ORDER nodes, tasks, the engine).  The
// COUNTERS-ONLY query first (limit 0: one synchronisation, no sort, no row): its totals size the buffers — the window has at most
// min(limit, total - offset) rows and the whole list's members — and ONE call behind it makes the order and the window; the
// engine's own size query (a NULL row buffer) would make the order twice.  by_config: PM_MAX_CONFIGS words or nullptr.
GpuMatchPlugin::GroupWindow GpuMatchPlugin::group_directory_locked(const pm_gdir_query& q, uint32_t* by_config) const {
  GroupWindow w;
  pm_gdir_query counters = q;
  counters.limit = 0u;
  uint32_t have = 0, have_members = 0;
  check(pm_group_directory(engine_, &counters, &w.totals, by_config, by_config ? uint32_t(PM_MAX_CONFIGS) : 0u, nullptr, 0u, &have,
                           nullptr, 0u, &have_members));
  have = q.offset >= w.totals.total ? 0u : std::min(q.limit, w.totals.total - q.offset);
  if (!have) return w;
  w.rows.resize(have);
  w.members.resize(w.totals.members_total ? w.totals.members_total : 1u);
  uint32_t got = 0, got_members = 0;
  check(pm_group_directory(engine_, &q, &w.totals, by_config, by_config ? uint32_t(PM_MAX_CONFIGS) : 0u, w.rows.data(),
                           uint32_t(w.rows.size()), &got, w.members.data(), uint32_t(w.members.size()), &got_members));
  if (got > w.rows.size() || got_members > w.members.size()) throw std::out_of_range("group directory: the window grew between two calls");
  w.rows.resize(got);
  w.members.resize(got_members);
  for (const pm_gdir_row& r : w.rows) {
    if (r.config >= config_names_.size()) throw std::out_of_range("group directory: the engine names a configuration the plugin has not");
    if (r.task != PM_NONE && r.task >= tasks_.size()) throw std::out_of_range("group directory: the engine names a task the plugin has not");
    if (uint64_t(r.member_begin) + r.size > w.members.size()) throw std::out_of_range("group directory: a row's members lie outside the window's");
  }
  for (const uint32_t m : w.members)
    if (m >= nodes_.address_strings.size()) throw std::out_of_range("group directory: the engine lists a member the plugin has no address of");
  return w;
}

std::vector<GpuMatchPlugin::ListedNodeGroup> GpuMatchPlugin::listed_groups_locked(const GroupWindow& w) const {
  std::vector<ListedNodeGroup> out;
  out.reserve(w.rows.size());
  for (const pm_gdir_row& r : w.rows) {
    ListedNodeGroup g;
    g.group.id = hex_lower(r.group_id);
    g.group.nodes.reserve(r.size);
    for (uint32_t k = 0; k < r.size; ++k) g.group.nodes.push_back(nodes_.address_strings[w.members[r.member_begin + k]]);
    g.group.configuration_name = config_names_[r.config];
    {
      std::lock_guard<std::mutex> lk(group_meta_mu_);
      const auto it = group_created_at_.find(r.group_id);
      g.group.created_at = it != group_created_at_.end() ? it->second : (clock ? clock() : 0);  // (formed, creation not reported yet)
    }
    g.health = r.health;
    g.rollout = r.rollout;
    if (r.task != PM_NONE) g.task_id = tasks_[r.task].id;
    g.row = r;
    out.push_back(std::move(g));
  }
  return out;
}

GpuMatchPlugin::GroupListing GpuMatchPlugin::list_groups(const GroupFilter& f, uint32_t order, uint32_t offset, uint32_t limit) const {
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);
  std::shared_lock<std::shared_mutex> tasks(tasks_mu_);
  const pm_gdir_query q{f.config_mask, f.holds, f.size_min, f.size_max, f.health_mask, f.rollout_mask, order, offset, limit};
  const GroupWindow w = group_directory_locked(q, nullptr);
  GroupListing out;
  out.total = w.totals.total;
  out.totals = w.totals;
  out.groups = listed_groups_locked(w);
  return out;
}

std::map<std::string, uint32_t> GpuMatchPlugin::group_counts() const {
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);
  std::shared_lock<std::shared_mutex> tasks(tasks_mu_);
  const pm_gdir_query q{~0ull, PM_GDIR_ANY, 0u, 0xFFFFFFFFu, (1u << PM_GH_N) - 1u, (1u << PM_GR_N) - 1u, PM_GDIR_BY_SLOT, 0u, 0u};  // the counters alone
  uint32_t by_config[PM_MAX_CONFIGS] = {};
  const GroupWindow w = group_directory_locked(q, by_config);
  if (w.totals.n_cfgs > config_names_.size()) throw std::out_of_range("group directory: the engine counts a configuration the plugin has not");
  std::map<std::string, uint32_t> out;
  for (uint32_t c = 0; c < w.totals.n_cfgs; ++c)
    if (by_config[c]) out[config_names_[c]] += by_config[c];  // (a name no group carries gets no gauge: sync_service.rs:275-282)
  return out;
}

std::vector<GpuMatchPlugin::ListedNodeGroup> GpuMatchPlugin::degraded_groups() const {
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);
  std::shared_lock<std::shared_mutex> tasks(tasks_mu_);
  const pm_gdir_query q{~0ull, PM_GDIR_ANY, 0u, 0xFFFFFFFFu, (1u << PM_GH_LOST) | (1u << PM_GH_DEGRADED), (1u << PM_GR_N) - 1u,
                        PM_GDIR_BY_ID_TEXT, 0u, 0xFFFFFFFFu};
  return listed_groups_locked(group_directory_locked(q, nullptr));
}

}  // namespace orchestrator
