// gpu_match_directory.cpp — GpuMatchPlugin::list_nodes / status_counts / uninvited_nodes / dead_nodes (see
// gpu_match_plugin.hpp): the engine's node directory (pm_directory) by node address.  The twin of the same methods of
// rust/gpu_match_plugin.rs, statement for statement.  (A file of its own: the plugin's other methods are also linked against a
// mock engine that has not this export.)
#include <algorithm>
#include <shared_mutex>
#include <stdexcept>

#include "group_id_text.hpp"
#include "gpu_match_plugin.hpp"

namespace orchestrator {

const char* GpuMatchPlugin::status_name(uint32_t status) {
  static const char* const names[PM_NS_N] = {"Discovered", "WaitingForHeartbeat", "Healthy", "Unhealthy",
                                             "Dead",       "Ejected",             "Banned",  "LowBalance"};
  if (status >= PM_NS_N) throw std::out_of_range("directory: not a node status");
  return names[status];
}

// one window of the directory (the node lock is held: LOCK ORDER nodes, the engine); the size query first, as every list
std::vector<pm_dir_row> GpuMatchPlugin::directory_locked(const pm_dir_query& q, uint32_t* total, uint32_t* counts) const {
  uint32_t have = 0;
  const int32_t rc = pm_directory(engine_, &q, total, counts, nullptr, 0u, &have);  // PM_ERANGE unless the window is empty
  if (rc != PM_ERANGE) check(rc);
  std::vector<pm_dir_row> rows(have ? have : 1u);
  if (!have) return rows.clear(), rows;
  uint32_t got = 0;
  check(pm_directory(engine_, &q, total, counts, rows.data(), uint32_t(rows.size()), &got));
  if (got > rows.size()) throw std::out_of_range("directory: the window grew between two calls");
  rows.resize(got);
  for (const pm_dir_row& r : rows)
    if (r.worker >= nodes_.rows.size() || r.status >= PM_NS_N)
      throw std::out_of_range("directory: the engine lists a row the plugin does not know");
  return rows;
}

GpuMatchPlugin::NodeListing GpuMatchPlugin::list_nodes(bool include_dead, uint32_t order, uint32_t offset, uint32_t limit) const {
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);
  const uint32_t all = (1u << PM_NS_N) - 1u;
  const pm_dir_query q{include_dead ? all : all & ~(1u << PM_NS_DEAD), PM_DIR_ANY, order, offset, limit};
  uint32_t counts[PM_NS_N] = {};
  NodeListing out;
  const std::vector<pm_dir_row> rows = directory_locked(q, &out.total, counts);
  for (uint32_t s = 0; s < PM_NS_N; ++s)
    if (counts[s]) out.counts[status_name(s)] = counts[s];  // (the route names the statuses it met: nodes.rs:47-59)
  out.nodes.reserve(rows.size());
  for (const pm_dir_row& r : rows) {
    ListedNode n;
    n.address = nodes_.address_strings[r.worker];
    n.status = NodeStatus(r.status);
    n.unhealthy_counter = r.counter;
    n.task_state = r.state;
    if (r.group_slot != PM_NONE) {  // nodes.rs:82-89: id, size, created_at, topology_config
      if (r.config >= config_names_.size()) throw std::out_of_range("directory: the engine names a configuration the plugin has not");
      ListedGroup g;
      g.id = hex_lower(r.group_id);
      g.size = r.group_size;
      g.topology_config = config_names_[r.config];
      {
        std::lock_guard<std::mutex> lk(group_meta_mu_);
        const auto it = group_created_at_.find(r.group_id);
        g.created_at = it != group_created_at_.end() ? it->second : (clock ? clock() : 0);  // (formed, creation not reported yet)
      }
      n.group = std::move(g);
    }
    out.nodes.push_back(std::move(n));
  }
  return out;
}

std::map<std::string, uint32_t> GpuMatchPlugin::status_counts() const {
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);
  const pm_dir_query q{(1u << PM_NS_N) - 1u, PM_DIR_ANY, PM_DIR_BY_ROW, 0u, 0u};  // the counters alone
  uint32_t total = 0, counts[PM_NS_N] = {};
  (void)directory_locked(q, &total, counts);
  std::map<std::string, uint32_t> out;
  for (uint32_t s = 0; s < PM_NS_N; ++s) {
    if (!counts[s]) continue;  // (a status no node has gets no gauge: sync_service.rs:218-225)
    std::string name = status_name(s);
    std::transform(name.begin(), name.end(), name.begin(), [](unsigned char c) { return char(c >= 'A' && c <= 'Z' ? c + 32 : c); });
    out[name] = counts[s];
  }
  return out;
}

std::vector<std::string> GpuMatchPlugin::nodes_of_status_locked(uint32_t status) const {
  const pm_dir_query q{1u << status, PM_DIR_ANY, PM_DIR_BY_ROW, 0u, 0xFFFFFFFFu};
  uint32_t total = 0;
  std::vector<std::string> out;
  for (const pm_dir_row& r : directory_locked(q, &total, nullptr)) out.push_back(nodes_.address_strings[r.worker]);
  return out;
}

std::vector<std::string> GpuMatchPlugin::uninvited_nodes() const {
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);
  return nodes_of_status_locked(PM_NS_DISCOVERED);
}

std::vector<std::string> GpuMatchPlugin::dead_nodes() const {
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);
  return nodes_of_status_locked(PM_NS_DEAD);
}

}  // namespace orchestrator
