// pm_plugin_discovery_c.cpp — see pm_plugin_c.h "discovery sync": the C face of GpuMatchPlugin::set_endpoint / sync_discovery.
// (A file of its own: pm_plugin_c.cpp is also linked against a mock engine that has not this export.)
#include <string>
#include <vector>

#include "pm_plugin_c.h"
#include "pm_plugin_c_internal.hpp"

using namespace orchestrator;

extern "C" {

int32_t pmx_set_endpoint(pmx_plugin* p, const char* address, const char* ip_address, uint16_t port) {
  try {
    p->plugin->set_endpoint(Address(address), ip_address, port);
    return 0;
  } catch (const std::exception& e) {
    pmx_detail::set_error(e.what());
    return -1;
  }
}

int32_t pmx_sync_discovery(pmx_plugin* p, uint64_t now_ms, const pmx_sighting* sightings, uint32_t n, uint32_t max_same_endpoint,
                           char* out, size_t cap, size_t* needed) {
  try {
    // (a sync commits: its text is held until a call's buffer has taken it — the size query and the call behind it hand over
    // ONE sync)
    if (!p->discovery_text_pending) {
      std::vector<GpuMatchPlugin::DiscoverySighting> list(n);
      for (uint32_t k = 0; k < n; ++k) {
        const pmx_sighting& s = sightings[k];
        GpuMatchPlugin::DiscoverySighting& d = list[k];
        d.address = Address(s.address);
        d.ip_address = s.ip_address;
        d.port = s.port;
        d.is_validated = s.is_validated != 0;
        d.is_provider_whitelisted = s.is_provider_whitelisted != 0;
        d.is_active = s.is_active != 0;
        d.location_new = s.location_new != 0;
        d.specs_differ = s.specs_differ != 0;
        d.balance_zero = s.balance_zero != 0;
        d.last_updated_ms = s.last_updated_ms;
      }
      std::string text;
      for (const auto& o : p->plugin->sync_discovery(now_ms, list, max_same_endpoint)) {
        using Kind = GpuMatchPlugin::DiscoveryOutcome::Kind;
        text += o.address + "\t" + (o.kind == Kind::Admitted ? "admitted" : o.kind == Kind::Skipped ? "skipped" : "synced") + "\t" +
                std::to_string(o.healthy_same_endpoint);
        if (o.kind == Kind::Synced) {
          text += "\t" + std::to_string(uint32_t(o.old_status)) + "\t" + std::to_string(uint32_t(o.final_status)) + "\t";
          text += std::string(o.ip_rewritten ? "i" : "") + (o.location_new ? "l" : "") + (o.specs_rewritten ? "s" : "") + (o.stamped_now ? "n" : "");
          text += "\t";
          for (size_t u = 0; u < o.updates.size(); ++u)
            text += (u ? "," : "") + std::to_string(uint32_t(o.updates[u].first)) + ">" + std::to_string(uint32_t(o.updates[u].second));
        }
        text += "\n";
      }
      p->discovery_text = text;
      p->discovery_text_pending = true;
    }
    const int32_t rc = pmx_detail::give_text(p->discovery_text, out, cap, needed);
    if (rc == 0 && out) p->discovery_text_pending = false;
    return rc;
  } catch (const std::exception& e) {
    pmx_detail::set_error(e.what());
    return -1;
  }
}

}  // extern "C"
