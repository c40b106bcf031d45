// pm_plugin_near_c.cpp — see pm_plugin_c.h "nearest candidates": the C face of GpuMatchPlugin::nearest_nodes.  (A file of its
// own: pm_plugin_c.cpp is also linked against a mock engine that has not this export.)
#include <cfloat>
#include <cstdio>
#include <string>

#include "pm_plugin_c.h"
#include "pm_plugin_c_internal.hpp"

using namespace orchestrator;

extern "C" {

int32_t pmx_nearest_nodes(pmx_plugin* p, const char* address, const char* configuration_name, uint32_t pool, uint32_t k,
                          int32_t* found, char* out, size_t cap, size_t* needed) {
  try {
    const std::optional<GpuMatchPlugin::NearestNodes> r = p->plugin->nearest_nodes(
        address ? std::optional<std::string>(address) : std::nullopt, configuration_name ? configuration_name : "", pool, k);
    if (found) *found = r ? 1 : 0;
    std::string text;
    if (r) {
      text = "origin\t" + (r->origin.empty() ? std::string("-") : r->origin) + "\t" + std::to_string(r->candidates) + "\t" +
             std::to_string(r->located) + "\n";
      for (const auto& n : r->nodes) {
        char buf[40] = "-";
        if (n.second != DBL_MAX) std::snprintf(buf, sizeof buf, "%.17g", n.second);  // (round-trips a double)
        text += n.first + "\t" + buf + "\n";
      }
    }
    return pmx_detail::give_text(text, out, cap, needed);
  } catch (const std::exception& e) {
    pmx_detail::set_error(e.what());
    return -1;
  }
}

}  // extern "C"
