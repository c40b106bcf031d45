// pm_plugin_directory_c.cpp — see pm_plugin_c.h "node directory": the C face of GpuMatchPlugin's directory methods.  (A file of
// its own: pm_plugin_c.cpp is also linked against a mock engine that has not this export.)
#include <string>
#include <vector>

#include "pm_plugin_c.h"
#include "pm_plugin_c_internal.hpp"

using namespace orchestrator;

namespace {
template <typename F>
int32_t guarded(F&& f) {
  try {
    return f();
  } catch (const std::exception& e) {
    pmx_detail::set_error(e.what());
    return -1;
  }
}
std::string lines(const std::vector<std::string>& v) {
  std::string out;
  for (const std::string& s : v) out += s + "\n";
  return out;
}
}  // namespace

extern "C" {

int32_t pmx_list_nodes(pmx_plugin* p, uint32_t include_dead, uint32_t order, uint32_t offset, uint32_t limit, char* out, size_t cap,
                       size_t* needed) {
  return guarded([&] {
    const GpuMatchPlugin::NodeListing l = p->plugin->list_nodes(include_dead != 0, order, offset, limit);
    std::string text = "total\t" + std::to_string(l.total) + "\n";
    for (const auto& kv : l.counts) text += "count\t" + kv.first + "\t" + std::to_string(kv.second) + "\n";
    for (const auto& n : l.nodes)
      text += n.address + "\t" + GpuMatchPlugin::status_name(uint32_t(n.status)) + "\t" + std::to_string(n.unhealthy_counter) + "\t" +
              (n.task_state == PM_TS_NONE ? "-" : std::to_string(n.task_state)) + "\t" + (n.group ? n.group->id : "-") + "\t" +
              (n.group ? std::to_string(n.group->size) : "-") + "\t" + (n.group ? n.group->topology_config : "-") + "\n";
    return pmx_detail::give_text(text, out, cap, needed);
  });
}

int32_t pmx_status_counts(pmx_plugin* p, char* out, size_t cap, size_t* needed) {
  return guarded([&] {
    std::string text;
    for (const auto& kv : p->plugin->status_counts()) text += kv.first + "\t" + std::to_string(kv.second) + "\n";
    return pmx_detail::give_text(text, out, cap, needed);
  });
}

int32_t pmx_uninvited_nodes(pmx_plugin* p, char* out, size_t cap, size_t* needed) {
  return guarded([&] { return pmx_detail::give_text(lines(p->plugin->uninvited_nodes()), out, cap, needed); });
}

int32_t pmx_dead_nodes(pmx_plugin* p, char* out, size_t cap, size_t* needed) {
  return guarded([&] { return pmx_detail::give_text(lines(p->plugin->dead_nodes()), out, cap, needed); });
}

}  // extern "C"
