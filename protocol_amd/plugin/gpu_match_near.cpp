// gpu_match_near.cpp — GpuMatchPlugin::nearest_nodes (see gpu_match_plugin.hpp): the engine's nearest-candidates query
// (pm_nearest_workers) by node address and configuration name.  The twin of the same method of rust/gpu_match_plugin.rs,
// statement for statement.  (A file of its own: the plugin's other methods are also linked against a mock engine that has
// not this export.)
#include <shared_mutex>
#include <stdexcept>

#include "gpu_match_plugin.hpp"

namespace orchestrator {

std::optional<GpuMatchPlugin::NearestNodes> GpuMatchPlugin::nearest_nodes(const std::optional<std::string>& address,
                                                                          const std::string& configuration_name, uint32_t pool,
                                                                          uint32_t k) const {
  uint32_t config = PM_NONE;
  for (size_t c = 0; c < config_names_.size() && config == PM_NONE; ++c)
    if (config_names_[c] == configuration_name) config = uint32_t(c);
  if (config == PM_NONE) throw std::invalid_argument("nearest_nodes: no configuration is named '" + configuration_name + "'");
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);  // (LOCK ORDER: nodes, the engine)
  pm_near_query q{PM_NEAR_SEED, config};
  if (address) {
    const std::optional<uint32_t> row = row_of_address_text(nodes_, *address);
    if (!row) return std::nullopt;
    q.origin = *row;
  }
  pm_near_row r{};
  std::vector<uint32_t> workers(k ? k : 1u);  // (k == 0 is the engine's to refuse)
  std::vector<double> km(workers.size());
  check(pm_nearest_workers(engine_, &q, 1, pool, k, &r, workers.data(), km.data()));
  NearestNodes out;
  if (r.origin != PM_NONE) out.origin = nodes_.address_strings[r.origin];
  out.candidates = r.candidates;
  out.located = r.located;
  out.nodes.reserve(r.n);
  for (uint32_t j = 0; j < r.n && j < workers.size(); ++j) out.nodes.emplace_back(nodes_.address_strings[workers[j]], km[j]);
  return out;
}

}  // namespace orchestrator
