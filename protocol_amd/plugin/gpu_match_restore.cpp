// gpu_match_restore.cpp — GpuMatchPlugin::restore_groups / group_tasks / group_id_state (see gpu_match_plugin.hpp): taking
// over the groups a store already holds, at a restart or when a pool moves from NodeGroupsPlugin to this plugin.  The twin of
// the same three methods of rust/gpu_match_plugin.rs, statement for statement.  (A file of its own: the plugin's other
// methods are also linked against a mock engine that has no pm_adopt_groups.)
#include <algorithm>
#include <random>
#include <shared_mutex>
#include <unordered_set>

#include "gpu_match_plugin.hpp"
#include "group_id_text.hpp"

namespace orchestrator {

GpuMatchPlugin::RestoreReport GpuMatchPlugin::restore_groups(const std::vector<NodeGroup>& groups,
                                                             const std::unordered_map<std::string, std::string>& group_tasks,
                                                             std::optional<uint64_t> id_state) {
  if (ticked_.load() || !nodes_synced_.load() || !tasks_synced_.load())
    throw EngineError(PM_ESTATE, "pm_engine error " + std::to_string(PM_ESTATE) + ": restore_groups: after sync_nodes and sync_tasks, before the first tick");
  if (!id_state && (multi_gpu || dist_world_ > 1))
    throw std::invalid_argument("restore_groups: the ranks of a multi-GPU pool must draw the same ids: pass id_state");
  RestoreReport report;
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);  // (LOCK ORDER: nodes, tasks, the engine)
  std::shared_lock<std::shared_mutex> tasks(tasks_mu_);
  std::unordered_map<std::string, uint32_t> task_position;  // task id text -> position in tasks_ (the engine's task index)
  for (size_t i = 0; i < tasks_.size(); ++i) task_position.emplace(tasks_[i].id, uint32_t(i));
  std::vector<pm_group> records;
  std::vector<uint32_t> members;
  std::vector<std::pair<uint64_t, int64_t>> created;
  std::unordered_set<uint64_t> ids;
  std::vector<bool> taken(nodes_.rows.size(), false);
  for (const NodeGroup& g : groups) {
    const auto drop = [&](const std::string& why) { report.dropped.emplace_back(g.id, why); };
    uint64_t id = 0;
    if (!parse_group_id(g.id, &id)) {
      drop("the id is not the {:x} text of a u64");
      continue;
    }
    const auto cfg = std::find(config_names_.begin(), config_names_.end(), g.configuration_name);
    if (cfg == config_names_.end()) {
      drop("unknown configuration " + g.configuration_name);
      continue;
    }
    std::vector<uint32_t> rows;
    std::string why;
    for (const std::string& a : g.nodes) {
      const std::optional<uint32_t> row = row_of_address_text(nodes_, a);
      if (!row) {
        why = "node " + a + " is not in the node table";
        break;
      }
      if (taken[*row] || std::find(rows.begin(), rows.end(), *row) != rows.end()) {
        why = "node " + a + " is already in an earlier group";
        break;
      }
      rows.push_back(*row);
    }
    if (!why.empty()) {
      drop(why);
      continue;
    }
    const size_t max_size = templates_[size_t(cfg - config_names_.begin())].max_group_size;
    if (rows.empty() || rows.size() > max_size) {
      drop(rows.empty() ? std::string("the group has no nodes")
                        : std::to_string(rows.size()) + " nodes, more than max_group_size " + std::to_string(max_size));
      continue;
    }
    if (!ids.insert(id).second) {
      drop("the id of an earlier group");
      continue;
    }
    pm_group rec{};
    rec.id = id;
    rec.config = uint32_t(cfg - config_names_.begin());
    rec.n_members = uint32_t(rows.size());
    rec.member_begin = uint32_t(members.size());
    rec.task = PM_NONE;
    if (const auto t = group_tasks.find(g.id); t != group_tasks.end()) {  // get_current_group_task (mod.rs:436-469)
      const auto at = task_position.find(t->second);
      if (at != task_position.end()) rec.task = at->second;
      else report.task_cleared.push_back(g.id);
    }
    for (uint32_t r : rows) taken[r] = true;
    members.insert(members.end(), rows.begin(), rows.end());
    records.push_back(rec);
    created.emplace_back(id, g.created_at);
  }
  uint64_t state = 0;
  if (id_state) {
    state = *id_state;
  } else {
    std::random_device rd;  // (generate_group_id draws from rand::rng(), mod.rs:1489-1493)
    state = (uint64_t(rd()) << 32) ^ uint64_t(rd());
  }
  check(pm_adopt_groups(engine_, records.empty() ? nullptr : records.data(), uint32_t(records.size()),
                        members.empty() ? nullptr : members.data(), uint32_t(members.size()), state));
  {
    std::lock_guard<std::mutex> lk(group_meta_mu_);
    for (const auto& kv : created) group_created_at_[kv.first] = kv.second;
  }
  check(pm_match(engine_, nullptr, nullptr));  // heartbeats are served from the adopted groups from here on
  return report;
}

std::unordered_map<std::string, std::string> GpuMatchPlugin::group_tasks() const {
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);
  std::shared_lock<std::shared_mutex> tasks(tasks_mu_);  // (task positions are positions in tasks_)
  const GroupSnapshot snap = snapshot_groups(false);
  std::unordered_map<std::string, std::string> out;
  for (const pm_group& g : snap.groups)
    if (g.task != PM_NONE && g.task < tasks_.size()) out.emplace(hex_lower(g.id), tasks_[g.task].id);
  return out;
}

uint64_t GpuMatchPlugin::group_id_state() const {
  uint64_t state = 0;
  check(pm_group_id_state(engine_, &state));
  return state;
}

}  // namespace orchestrator
