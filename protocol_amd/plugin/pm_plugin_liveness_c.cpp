// pm_plugin_liveness_c.cpp — see pm_plugin_c.h "liveness": the C face of GpuMatchPlugin::enable_liveness / beat /
// sweep_statuses.  (A file of its own: pm_plugin_c.cpp is also linked against a mock engine that has not these exports.)
#include <string>
#include <vector>

#include "pm_plugin_c.h"
#include "pm_plugin_c_internal.hpp"

using namespace orchestrator;

extern "C" {

int32_t pmx_enable_liveness(pmx_plugin* p, uint32_t missing_heartbeat_threshold) {
  try {
    p->plugin->enable_liveness(missing_heartbeat_threshold);
    return 0;
  } catch (const std::exception& e) {
    pmx_detail::set_error(e.what());
    return -1;
  }
}

int32_t pmx_beat(pmx_plugin* p, const char* address, uint64_t now_ms) {
  try {
    p->plugin->beat(Address(address), now_ms);
    return 0;
  } catch (const std::exception& e) {
    pmx_detail::set_error(e.what());
    return -1;
  }
}

int32_t pmx_sweep_statuses(pmx_plugin* p, uint64_t now_ms, const char* const* out_of_pool, uint32_t n_out_of_pool, char* out,
                           size_t cap, size_t* needed) {
  try {
    // (a sweep commits: its text is held until a call's buffer has taken it — the size query and the call behind it hand over
    // ONE sweep)
    if (!p->sweep_text_pending) {
      std::vector<Address> outside;
      for (uint32_t k = 0; k < n_out_of_pool; ++k) outside.emplace_back(out_of_pool[k]);
      std::string text;
      for (const auto& t : p->plugin->sweep_statuses(now_ms, outside))
        text += t.address + "\t" + std::to_string(uint32_t(t.old_status)) + "\t" + std::to_string(uint32_t(t.new_status)) + "\n";
      p->sweep_text = text;
      p->sweep_text_pending = true;
    }
    const int32_t rc = pmx_detail::give_text(p->sweep_text, out, cap, needed);
    if (rc == 0 && out) p->sweep_text_pending = false;
    return rc;
  } catch (const std::exception& e) {
    pmx_detail::set_error(e.what());
    return -1;
  }
}

}  // extern "C"
