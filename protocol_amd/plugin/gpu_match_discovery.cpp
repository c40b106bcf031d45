// gpu_match_discovery.cpp — GpuMatchPlugin::set_endpoint / sync_discovery (see gpu_match_plugin.hpp): the engine's discovery
// sync (pm_discovery_sync) by node address.  The twin of the same methods of rust/gpu_match_plugin.rs, statement for statement.
// (A file of its own: the plugin's other methods are also linked against a mock engine that has not this export.)
#include <shared_mutex>
#include <stdexcept>

#include "gpu_match_plugin.hpp"

namespace orchestrator {

uint32_t GpuMatchPlugin::intern_endpoint_locked(const std::string& ip, uint16_t port) {
  EndpointColumn& c = endpoints_;
  return c.intern.emplace(ip + ":" + std::to_string(port), uint32_t(c.intern.size())).first->second;
}

// the column covers every row; the endpoints remembered for addresses that have a row by now move into it
void GpuMatchPlugin::fit_endpoints_locked() {
  EndpointColumn& c = endpoints_;
  const size_t W = nodes_.rows.size();
  if (c.ip.size() < W) {
    c.ip.resize(W);
    c.port.resize(W, 0);
    c.id.resize(W, PM_EP_NONE);
  }
  if (stamps_.size() < W) stamps_.resize(W, 0);
  for (auto it = c.pending.begin(); it != c.pending.end();) {
    const auto row = nodes_.index.find(it->first);
    if (row == nodes_.index.end()) {
      ++it;
      continue;
    }
    c.ip[row->second] = it->second.first;
    c.port[row->second] = it->second.second;
    c.id[row->second] = intern_endpoint_locked(it->second.first, it->second.second);
    it = c.pending.erase(it);
  }
}

void GpuMatchPlugin::set_endpoint(const Address& address, const std::string& ip_address, uint16_t port) {
  std::unique_lock<std::shared_mutex> nodes(nodes_mu_);
  endpoints_.pending[address] = std::make_pair(ip_address, port);
  fit_endpoints_locked();
}

std::optional<std::pair<std::string, uint16_t>> GpuMatchPlugin::endpoint_of(const Address& address) const {
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);
  const auto it = nodes_.index.find(address);
  if (it == nodes_.index.end() || it->second >= endpoints_.ip.size() || endpoints_.ip[it->second].empty()) return std::nullopt;
  return std::make_pair(endpoints_.ip[it->second], endpoints_.port[it->second]);
}

uint64_t GpuMatchPlugin::last_status_change_ms(const Address& address) const {
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);
  const auto it = nodes_.index.find(address);
  return it == nodes_.index.end() || it->second >= stamps_.size() ? 0 : stamps_[it->second];
}

std::vector<GpuMatchPlugin::DiscoveryOutcome> GpuMatchPlugin::sync_discovery(uint64_t now_ms, const std::vector<DiscoverySighting>& sightings,
                                                                             uint32_t max_same_endpoint) {
  std::vector<DiscoveryOutcome> out;
  bool any_dead = false;
  {
    std::unique_lock<std::shared_mutex> nodes(nodes_mu_);  // (LOCK ORDER: nodes, the engine; flags, stamps and endpoints are written below)
    NodeTable& t = nodes_;
    EndpointColumn& c = endpoints_;
    const size_t W = t.rows.size(), D = sightings.size();
    fit_endpoints_locked();
    std::vector<pm_disc_row> rows(D);
    std::vector<uint32_t> column(W);
    for (int pass = 0;; ++pass) {
      for (size_t j = 0; j < D; ++j) {
        const DiscoverySighting& s = sightings[j];
        pm_disc_row& r = rows[j];
        r = pm_disc_row{};
        r.endpoint = intern_endpoint_locked(s.ip_address, s.port);
        r.flags = (s.is_validated ? uint32_t(PM_DF_VALIDATED) : 0u) | (s.is_provider_whitelisted ? uint32_t(PM_DF_WHITELISTED) : 0u) |
                  (s.is_active ? uint32_t(PM_DF_ACTIVE) : 0u) | (s.balance_zero ? uint32_t(PM_DF_BALANCE_ZERO) : 0u);
        r.last_updated_ms = s.last_updated_ms;
        const auto it = t.index.find(s.address);
        if (it == t.index.end() || !t.present[it->second]) {  // get_node is Ok(None) (a tombstoned row left the store)
          r.row = PM_DISC_NEW;
          continue;
        }
        const uint32_t w = it->second;
        r.row = w;
        // "discovery ip : STORED port" (a row whose endpoint nobody told has no stored port: the sighting's)
        r.endpoint_after = intern_endpoint_locked(s.ip_address, c.ip[w].empty() ? s.port : c.port[w]);
        r.flags |= (s.location_new ? uint32_t(PM_DF_LOCATION_NEW) : 0u) | (s.specs_differ ? uint32_t(PM_DF_SPECS_DIFFER) : 0u);
        r.last_change_ms = stamps_[w];
      }
      if (c.intern.size() <= W + 2 * D || pass) break;
      // ids of endpoints nobody holds any more have piled up past what the engine accepts: intern the column afresh
      c.intern.clear();
      for (size_t w = 0; w < W; ++w) c.id[w] = c.ip[w].empty() ? PM_EP_NONE : intern_endpoint_locked(c.ip[w], c.port[w]);
    }
    for (size_t w = 0; w < W; ++w) column[w] = t.present[w] ? c.id[w] : PM_EP_NONE;  // (a node that left the store is no "other node")
    std::vector<pm_disc_result> res(D ? D : 1u);
    check(pm_discovery_sync(engine_, now_ms, W ? column.data() : nullptr, uint32_t(c.intern.size()), max_same_endpoint,
                            D ? rows.data() : nullptr, uint32_t(D), 1u, res.data(), nullptr));
    for (size_t j = 0; j < D; ++j)
      if (rows[j].row != PM_DISC_NEW && (res[j].old_status >= PM_NS_N || res[j].final_status >= PM_NS_N || res[j].n_updates > 3u))
        throw std::out_of_range("sync_discovery: a result that is no node status");
    out.reserve(D);
    for (size_t j = 0; j < D; ++j) {
      const DiscoverySighting& s = sightings[j];
      const pm_disc_result& r = res[j];
      DiscoveryOutcome o;
      o.address = s.address.to_string();
      o.healthy_same_endpoint = r.healthy_same_endpoint;
      if (rows[j].row == PM_DISC_NEW) {
        o.kind = (r.ops & PM_DO_ADMIT) ? DiscoveryOutcome::Kind::Admitted : DiscoveryOutcome::Kind::Skipped;
        if (r.ops & PM_DO_ADMIT) c.pending[s.address] = std::make_pair(s.ip_address, s.port);
        out.push_back(std::move(o));
        continue;
      }
      const uint32_t w = rows[j].row;
      o.old_status = NodeStatus(r.old_status);
      o.final_status = NodeStatus(r.final_status);
      for (uint32_t u = 0; u < r.n_updates; ++u) {
        o.updates.emplace_back(NodeStatus(r.upd_old[u]), NodeStatus(r.upd_new[u]));
        any_dead = any_dead || r.upd_new[u] == PM_NS_DEAD || r.upd_new[u] == PM_NS_LOWBALANCE;
      }
      o.ip_rewritten = r.ops & PM_DO_IP_REWRITE;
      o.location_new = r.ops & PM_DO_LOCATION;
      o.specs_rewritten = r.ops & PM_DO_SPECS_REWRITE;
      o.stamped_now = r.ops & PM_DO_STAMP_NOW;
      if (o.ip_rewritten && !o.specs_rewritten) {  // (the specs put-back restores the old ip)
        if (c.ip[w].empty()) c.port[w] = s.port;
        c.ip[w] = s.ip_address;
        c.id[w] = rows[j].endpoint_after;
      }
      if (r.n_updates) {  // (what the engine's apply gave the row)
        uint32_t flags = t.rows[w].flags & ~uint32_t(PM_W_HEALTHY);
        if (r.final_status == PM_NS_HEALTHY) flags |= PM_W_HEALTHY;
        t.rows[w].flags = flags;
      }
      if (o.stamped_now) stamps_[w] = now_ms;
      out.push_back(std::move(o));
    }
  }
  if (any_dead) emit_group_webhooks();  // whole groups were dissolved (status_update_impl.rs:16-29)
  return out;
}

}  // namespace orchestrator
