// pm_plugin_probe_c.cpp — see pm_plugin_c.h "probing configurations": the C face of GpuMatchPlugin::probe_configurations and
// configuration_overlap.  (A file of its own: pm_plugin_c.cpp is also linked against a mock engine that has not these exports.)
#include <string>

#include "pm_plugin_c.h"
#include "pm_plugin_c_internal.hpp"

using namespace orchestrator;

extern "C" {

int32_t pmx_probe_configurations(pmx_plugin* p, const pmx_config* probes, uint32_t n, char* out, size_t cap, size_t* needed) {
  if (n && !probes) {
    pmx_detail::set_error("null argument");
    return -1;
  }
  try {
    std::vector<NodeGroupConfiguration> t;
    for (uint32_t i = 0; i < n; ++i) {
      NodeGroupConfiguration c{probes[i].name ? probes[i].name : "", probes[i].min_group_size, probes[i].max_group_size, std::nullopt};
      if (probes[i].compute_requirements) c.compute_requirements = std::string(probes[i].compute_requirements);
      t.push_back(c);
    }
    std::string text;
    for (const GpuMatchPlugin::ProbeResult& r : p->plugin->probe_configurations(t)) {
      text += r.name;
      for (uint32_t v : {r.eligible_meets, r.idle_meets, r.idle_located, r.idle_exclusive, r.groups_max, r.groups_exclusive})
        text += "\t" + std::to_string(v);
      for (uint32_t v : r.why) text += "\t" + std::to_string(v);
      for (const auto& o : r.overlap) text += "\t" + o.first + "=" + std::to_string(o.second);
      text += "\n";
    }
    return pmx_detail::give_text(text, out, cap, needed);
  } catch (const std::exception& e) {
    pmx_detail::set_error(e.what());
    return -1;
  }
}

int32_t pmx_configuration_overlap(pmx_plugin* p, char* out, size_t cap, size_t* needed) {
  try {
    const GpuMatchPlugin::ConfigurationOverlap o = p->plugin->configuration_overlap();
    const size_t C = o.names.size();
    std::string text;
    for (size_t a = 0; a < C; ++a) {
      text += o.names[a];
      for (size_t b = 0; b < C; ++b) text += "\t" + std::to_string(o.idle[a * C + b]);
      text += "\n";
    }
    return pmx_detail::give_text(text, out, cap, needed);
  } catch (const std::exception& e) {
    pmx_detail::set_error(e.what());
    return -1;
  }
}

}  // extern "C"
