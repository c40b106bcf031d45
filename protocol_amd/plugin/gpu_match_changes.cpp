// gpu_match_changes.cpp — GpuMatchPlugin::enable_change_feed / changed_nodes (see gpu_match_plugin.hpp): the engine's assignment
// change feed (pm_enable_assignment_changes / pm_drain_assignment_changes) by node address.  The twin of the same methods of
// rust/gpu_match_plugin.rs, statement for statement.  (A file of its own: the plugin's other methods are also linked against a
// mock engine that has not these exports.)
#include <shared_mutex>
#include <stdexcept>

#include "gpu_match_plugin.hpp"

namespace orchestrator {

void GpuMatchPlugin::enable_change_feed(bool on) const { check(pm_enable_assignment_changes(engine_, on ? 1u : 0u)); }

GpuMatchPlugin::ChangedNodes GpuMatchPlugin::changed_nodes() const {
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);  // (LOCK ORDER: nodes, the engine)
  std::vector<pm_change_row> rows;
  uint32_t n = 0, flags = 0;
  int32_t rc = pm_drain_assignment_changes(engine_, nullptr, 0, &n, &flags);  // the size query
  while (rc == PM_ERANGE) {  // (a publish between two calls lengthens the list: ask again with the new size, never read short)
    rows.resize(n ? n : 1u);
    rc = pm_drain_assignment_changes(engine_, rows.data(), uint32_t(rows.size()), &n, &flags);
  }
  check(rc);
  if (n > rows.size()) throw std::out_of_range("changed_nodes: the engine reports more rows than it was given room for");
  for (uint32_t j = 0; j < n; ++j)
    if (rows[j].worker >= nodes_.address_strings.size())
      throw std::out_of_range("changed_nodes: the engine lists a row the node table does not hold");
  ChangedNodes out;
  out.resync = (flags & PM_CHANGES_RESYNC) != 0u;
  out.nodes.reserve(n);
  for (uint32_t j = 0; j < n; ++j) out.nodes.emplace_back(nodes_.address_strings[rows[j].worker], rows[j].what);
  return out;
}

}  // namespace orchestrator
