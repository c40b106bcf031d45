// gpu_match_spread.cpp — GpuMatchPlugin::group_spread / configuration_spread / force_regroup (see gpu_match_plugin.hpp): the
// engine's group geography reports (pm_group_spread, pm_config_spread) by group id text and configuration name, and
// pm_force_regroup by configuration name.  The twin of the same three methods of rust/gpu_match_plugin.rs, statement for
// statement.  (A file of its own: the plugin's other methods are also linked against a mock engine that has none of these
// exports.)
#include <shared_mutex>

#include "gpu_match_plugin.hpp"
#include "group_id_text.hpp"

namespace orchestrator {

std::unordered_map<std::string, GpuMatchPlugin::GroupSpread> GpuMatchPlugin::group_spread() const {
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);  // (LOCK ORDER: nodes, the engine)
  // the ids in slot order, then the rows in the same order; another thread's call in between changes the count (a
  // dissolution, a tick): ask again
  for (int attempt = 0; attempt < 8; ++attempt) {
    const GroupSnapshot snap = snapshot_groups(false);
    std::vector<pm_group_spread_row> rows(snap.groups.size());
    uint32_t n = 0;
    const int32_t rc = pm_group_spread(engine_, rows.empty() ? nullptr : rows.data(), uint32_t(rows.size()), &n);
    if (rc == PM_ERANGE && n != rows.size()) continue;
    check(rc);
    if (n != rows.size()) continue;
    const auto addr = [&](uint32_t w) { return w == PM_NONE ? std::string() : nodes_.address_strings[w]; };
    std::unordered_map<std::string, GroupSpread> out;
    out.reserve(n);
    for (uint32_t g = 0; g < n; ++g) {
      const pm_group_spread_row& r = rows[g];
      GroupSpread o;
      o.located = r.located;
      o.ring_hops = r.ring_hops;
      o.far_a = addr(r.far_a);
      o.far_b = addr(r.far_b);
      o.hop_from = addr(r.hop_from);
      o.diameter_km = r.diameter_km;
      o.ring_km = r.ring_km;
      o.longest_hop_km = r.longest_hop_km;
      out.emplace(hex_lower(snap.groups[g].id), std::move(o));
    }
    return out;
  }
  throw EngineError(PM_ESTATE, "group_spread: the group list kept changing under the report");
}

std::vector<GpuMatchPlugin::ConfigurationSpread> GpuMatchPlugin::configuration_spread() const {
  std::vector<pm_config_spread_row> rows(config_names_.size());
  uint32_t n = 0;
  check(pm_config_spread(engine_, rows.empty() ? nullptr : rows.data(), uint32_t(rows.size()), &n));
  std::vector<ConfigurationSpread> out;
  for (uint32_t c = 0; c < n && c < rows.size(); ++c) {
    const pm_config_spread_row& r = rows[c];
    ConfigurationSpread o;
    o.name = config_names_[c];
    o.groups = r.groups;
    o.measured = r.measured;
    for (size_t k = 0; k < o.hist.size(); ++k) o.hist[k] = r.hist[k];
    o.max_diameter_km = r.max_diameter_km;
    o.max_hop_km = r.max_hop_km;
    o.sum_diameter_m = r.sum_diameter_m;
    o.sum_ring_m = r.sum_ring_m;
    out.push_back(std::move(o));
  }
  return out;
}

std::optional<GpuMatchPlugin::ForceRegroupResult> GpuMatchPlugin::force_regroup(const std::string& configuration_name,
                                                                                uint32_t metric, double threshold_km) {
  uint32_t config = PM_NONE;
  for (size_t c = 0; c < config_names_.size() && config == PM_NONE; ++c)
    if (config_names_[c] == configuration_name) config = uint32_t(c);
  if (config == PM_NONE) return std::nullopt;  // "Configuration not found" (groups.rs: 404)
  ForceRegroupResult out;
  check(pm_force_regroup(engine_, config, metric, threshold_km, &out.dissolved_groups, &out.affected_nodes));
  if (out.dissolved_groups) emit_group_webhooks();  // send_group_destroyed per group, mod.rs:1469-1481
  return out;
}

}  // namespace orchestrator
