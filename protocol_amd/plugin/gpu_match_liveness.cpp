// gpu_match_liveness.cpp — GpuMatchPlugin::enable_liveness / beat / sweep_statuses (see gpu_match_plugin.hpp): the engine's
// liveness sweep (pm_liveness_*) by node address.  The twin of the same methods of rust/gpu_match_plugin.rs, statement for
// statement.  (A file of its own: the plugin's other methods are also linked against a mock engine that has not these exports.)
#include <shared_mutex>
#include <stdexcept>

#include "gpu_match_plugin.hpp"

namespace orchestrator {

void GpuMatchPlugin::enable_liveness(uint32_t missing_heartbeat_threshold) {
  std::unique_lock<std::shared_mutex> nodes(nodes_mu_);  // (LOCK ORDER: nodes, the engine)
  check(pm_liveness_enable(engine_, 1u, missing_heartbeat_threshold));
  liveness_note_ = &GpuMatchPlugin::liveness_note;
}

// handle_status_change's write to the ledger (the exclusive node lock is held): the discovery monitor's Dead / Ejected /
// Discovered / LowBalance (discovery/monitor.rs:262-389) and the ban route (api/routes/nodes.rs:365) leave the unhealthy
// counter alone, the invite (node/invite.rs:168-176) sets WaitingForHeartbeat and clears it
void GpuMatchPlugin::liveness_note(const GpuMatchPlugin& self, uint32_t row, NodeStatus status) {
  const uint8_t s = uint8_t(status);
  uint32_t counter = 0;
  if (status != NodeStatus::WaitingForHeartbeat) self.check(pm_liveness_get(self.engine_, &row, 1u, nullptr, &counter));
  self.check(pm_liveness_set(self.engine_, &row, &s, &counter, 1u));
}

void GpuMatchPlugin::beat(const Address& address, uint64_t now_ms) const {
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);
  const auto it = nodes_.index.find(address);
  if (it == nodes_.index.end() || it->second >= beats_cap_) return;
  beats_[it->second].store(now_ms, std::memory_order_relaxed);
}

std::vector<GpuMatchPlugin::StatusTransition> GpuMatchPlugin::sweep_statuses(uint64_t now_ms, const std::vector<Address>& out_of_pool) {
  std::vector<StatusTransition> out;
  bool any_dead = false;
  {
    std::unique_lock<std::shared_mutex> nodes(nodes_mu_);  // (LOCK ORDER: nodes, the engine; the rows' flags are written below)
    NodeTable& t = nodes_;
    const size_t W = t.rows.size();
    std::vector<uint64_t> beats(W), pool;
    for (size_t w = 0; w < W; ++w) beats[w] = w < beats_cap_ ? beats_[w].load(std::memory_order_relaxed) : 0;
    if (!out_of_pool.empty()) {
      pool.assign((W + 63) / 64, ~uint64_t(0));
      for (const Address& a : out_of_pool) {
        const auto it = t.index.find(a);
        if (it != t.index.end()) pool[it->second >> 6] &= ~(uint64_t(1) << (it->second & 63u));
      }
    }
    uint32_t n = 0;
    // (admission on: the later of the device's beat column and this one, so beat() and admitted heartbeats both count)
    check((sweep_call_ ? sweep_call_ : pm_liveness_sweep)(engine_, now_ms, W ? beats.data() : nullptr, pool.empty() ? nullptr : pool.data(), 1u, &n,
                                                          nullptr));
    std::vector<pm_live_row> rows(n ? n : 1u);
    uint32_t got = 0;
    check(pm_liveness_transitions(engine_, rows.data(), uint32_t(rows.size()), &got));
    if (got != n) throw std::out_of_range("sweep_statuses: the list is not the sweep's");
    for (uint32_t j = 0; j < n; ++j)
      if (rows[j].worker >= W || rows[j].old_status >= PM_NS_N || rows[j].new_status >= PM_NS_N)
        throw std::out_of_range("sweep_statuses: the engine lists a row the node table does not hold");
    out.reserve(n);
    for (uint32_t j = 0; j < n; ++j) {
      const pm_live_row& r = rows[j];
      uint32_t flags = t.rows[r.worker].flags & ~uint32_t(PM_W_HEALTHY);  // (what the engine's apply gave the row)
      if (r.new_status == PM_NS_HEALTHY) flags |= PM_W_HEALTHY;
      t.rows[r.worker].flags = flags;
      note_stamp_locked(r.worker, now_ms);
      any_dead = any_dead || r.new_status == PM_NS_DEAD;
      out.push_back(StatusTransition{t.address_strings[r.worker], NodeStatus(r.old_status), NodeStatus(r.new_status)});
    }
  }
  if (any_dead) emit_group_webhooks();  // whole groups were dissolved (status_update_impl.rs:17-29)
  return out;
}

}  // namespace orchestrator
