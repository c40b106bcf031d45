// pm_plugin_changes_c.cpp — see pm_plugin_c.h "change feed": the C face of GpuMatchPlugin::enable_change_feed / changed_nodes.
// (A file of its own: pm_plugin_c.cpp is also linked against a mock engine that has not these exports.)
#include <string>

#include "pm_plugin_c.h"
#include "pm_plugin_c_internal.hpp"

using namespace orchestrator;

extern "C" {

int32_t pmx_enable_change_feed(pmx_plugin* p, int32_t on) {
  try {
    p->plugin->enable_change_feed(on != 0);
    return 0;
  } catch (const std::exception& e) {
    pmx_detail::set_error(e.what());
    return -1;
  }
}

int32_t pmx_changed_nodes(pmx_plugin* p, char* out, size_t cap, size_t* needed) {
  try {
    // (the drain empties the feed: its text is held until a call's buffer has taken it — the size query and the call behind it
    // hand over ONE drain)
    if (!p->changed_text_pending) {
      const GpuMatchPlugin::ChangedNodes r = p->plugin->changed_nodes();
      std::string text = std::string("resync\t") + (r.resync ? "1" : "0") + "\n";
      for (const auto& n : r.nodes) text += n.first + "\t" + std::to_string(n.second) + "\n";
      p->changed_text = text;
      p->changed_text_pending = true;
    }
    const int32_t rc = pmx_detail::give_text(p->changed_text, out, cap, needed);
    if (rc == 0 && out) p->changed_text_pending = false;
    return rc;
  } catch (const std::exception& e) {
    pmx_detail::set_error(e.what());
    return -1;
  }
}

}  // extern "C"
