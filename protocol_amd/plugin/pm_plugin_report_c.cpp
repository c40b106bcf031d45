// pm_plugin_report_c.cpp — see pm_plugin_c.h "diagnostics": the C face of GpuMatchPlugin::explain_node,
// configuration_report and task_report.  (A file of its own: pm_plugin_c.cpp is also linked against a mock engine that has
// none of the report exports.)
#include <algorithm>
#include <string>
#include <vector>

#include "pm_plugin_c.h"
#include "pm_plugin_c_internal.hpp"

using namespace orchestrator;

extern "C" {

int32_t pmx_explain_node(pmx_plugin* p, const char* address, char* out, size_t cap, size_t* needed) {
  try {
    const std::optional<GpuMatchPlugin::NodeExplanation> x = p->plugin->explain_node(address ? address : "");
    std::string text;
    if (x) {
      text = "state\t" + x->state + "\n";
      for (const auto& c : x->configs) text += c.first + "\t" + c.second + "\n";
    }
    return pmx_detail::give_text(text, out, cap, needed);
  } catch (const std::exception& e) {
    pmx_detail::set_error(e.what());
    return -1;
  }
}

int32_t pmx_configuration_report(pmx_plugin* p, char* out, size_t cap, size_t* needed) {
  try {
    std::string text;
    for (const GpuMatchPlugin::ConfigurationReport& r : p->plugin->configuration_report()) {
      text += r.name + "\t" + (r.enabled ? "1" : "0");
      for (uint32_t v : {r.eligible_meets, r.idle_meets, r.groups, r.members, r.groups_without_task, r.tasks_allowing})
        text += "\t" + std::to_string(v);
      for (uint32_t v : r.why) text += "\t" + std::to_string(v);
      text += "\n";
    }
    return pmx_detail::give_text(text, out, cap, needed);
  } catch (const std::exception& e) {
    pmx_detail::set_error(e.what());
    return -1;
  }
}

int32_t pmx_task_report(pmx_plugin* p, char* out, size_t cap, size_t* needed) {
  try {
    const auto m = p->plugin->task_report();
    std::vector<std::pair<std::string, GpuMatchPlugin::TaskReport>> sorted(m.begin(), m.end());
    std::sort(sorted.begin(), sorted.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    std::string text;
    for (const auto& kv : sorted)
      text += kv.first + "\t" + std::to_string(kv.second.groups_running) + "\t" + std::to_string(kv.second.workers_running) +
              "\t" + std::to_string(kv.second.groups_allowed) + "\n";
    return pmx_detail::give_text(text, out, cap, needed);
  } catch (const std::exception& e) {
    pmx_detail::set_error(e.what());
    return -1;
  }
}

}  // extern "C"
