// pm_plugin_spread_c.cpp — see pm_plugin_c.h "group geography": the C face of GpuMatchPlugin::group_spread,
// configuration_spread and force_regroup.  (A file of its own: pm_plugin_c.cpp is also linked against a mock engine that
// has none of these exports.)
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "pm_plugin_c.h"
#include "pm_plugin_c_internal.hpp"

using namespace orchestrator;

namespace {
std::string f64_text(double v) {  // round-trips a double
  char buf[40];
  std::snprintf(buf, sizeof buf, "%.17g", v);
  return buf;
}
std::string or_dash(const std::string& s) { return s.empty() ? "-" : s; }
}  // namespace

extern "C" {

int32_t pmx_group_spread(pmx_plugin* p, char* out, size_t cap, size_t* needed) {
  try {
    const auto m = p->plugin->group_spread();
    std::vector<std::pair<std::string, GpuMatchPlugin::GroupSpread>> sorted(m.begin(), m.end());
    std::sort(sorted.begin(), sorted.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    std::string text;
    for (const auto& kv : sorted) {
      const GpuMatchPlugin::GroupSpread& r = kv.second;
      text += kv.first + "\t" + std::to_string(r.located) + "\t" + std::to_string(r.ring_hops) + "\t" + or_dash(r.far_a) + "\t" +
              or_dash(r.far_b) + "\t" + or_dash(r.hop_from) + "\t" + f64_text(r.diameter_km) + "\t" + f64_text(r.ring_km) + "\t" +
              f64_text(r.longest_hop_km) + "\n";
    }
    return pmx_detail::give_text(text, out, cap, needed);
  } catch (const std::exception& e) {
    pmx_detail::set_error(e.what());
    return -1;
  }
}

int32_t pmx_configuration_spread(pmx_plugin* p, char* out, size_t cap, size_t* needed) {
  try {
    std::string text;
    for (const GpuMatchPlugin::ConfigurationSpread& r : p->plugin->configuration_spread()) {
      text += r.name + "\t" + std::to_string(r.groups) + "\t" + std::to_string(r.measured);
      for (uint32_t v : r.hist) text += "\t" + std::to_string(v);
      text += "\t" + f64_text(r.max_diameter_km) + "\t" + f64_text(r.max_hop_km) + "\t" + std::to_string(r.sum_diameter_m) +
              "\t" + std::to_string(r.sum_ring_m) + "\n";
    }
    return pmx_detail::give_text(text, out, cap, needed);
  } catch (const std::exception& e) {
    pmx_detail::set_error(e.what());
    return -1;
  }
}

int32_t pmx_force_regroup(pmx_plugin* p, const char* configuration_name, uint32_t metric, double threshold_km, int32_t* found,
                          uint32_t* dissolved_groups, uint32_t* affected_nodes) {
  try {
    const std::optional<GpuMatchPlugin::ForceRegroupResult> r =
        p->plugin->force_regroup(configuration_name ? configuration_name : "", metric, threshold_km);
    if (found) *found = r ? 1 : 0;
    if (dissolved_groups) *dissolved_groups = r ? r->dissolved_groups : 0u;
    if (affected_nodes) *affected_nodes = r ? r->affected_nodes : 0u;
    return 0;
  } catch (const std::exception& e) {
    pmx_detail::set_error(e.what());
    return -1;
  }
}

}  // extern "C"
