// pm_plugin_groupdir_c.cpp — see pm_plugin_c.h "group directory": the C face of GpuMatchPlugin's group directory methods.  (A
// file of its own: pm_plugin_c.cpp is also linked against a mock engine that has not this export.)
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
std::string group_lines(const std::vector<GpuMatchPlugin::ListedNodeGroup>& groups) {
  static const char* const health[PM_GH_N] = {"lost", "degraded", "sound"};
  static const char* const rollout[PM_GR_N] = {"no_task", "converged", "rolling"};
  std::string text;
  for (const auto& g : groups) {
    text += g.group.id + "\t" + g.group.configuration_name + "\t" + std::to_string(g.group.nodes.size()) + "\t" +
            (g.health < PM_GH_N ? health[g.health] : "-") + "\t" + (g.rollout < PM_GR_N ? rollout[g.rollout] : "-") + "\t" +
            (g.task_id ? *g.task_id : "-") + "\t" + std::to_string(g.group.created_at) + "\t";
    for (size_t k = 0; k < g.group.nodes.size(); ++k) text += (k ? "," : "") + g.group.nodes[k];
    text += "\n";
  }
  return text;
}
}  // namespace

extern "C" {

int32_t pmx_list_groups(pmx_plugin* p, uint64_t config_mask, uint32_t holds, uint32_t size_min, uint32_t size_max, uint32_t health_mask,
                        uint32_t rollout_mask, uint32_t order, uint32_t offset, uint32_t limit, char* out, size_t cap, size_t* needed) {
  return guarded([&] {
    const GpuMatchPlugin::GroupFilter f{config_mask, holds, size_min, size_max, health_mask, rollout_mask};
    const GpuMatchPlugin::GroupListing l = p->plugin->list_groups(f, order, offset, limit);
    const std::string text = "total\t" + std::to_string(l.total) + "\t" + std::to_string(l.totals.members_total) + "\n" + group_lines(l.groups);
    return pmx_detail::give_text(text, out, cap, needed);
  });
}

int32_t pmx_group_counts(pmx_plugin* p, char* out, size_t cap, size_t* needed) {
  return guarded([&] {
    std::string text;
    for (const auto& kv : p->plugin->group_counts()) text += kv.first + "\t" + std::to_string(kv.second) + "\n";
    return pmx_detail::give_text(text, out, cap, needed);
  });
}

int32_t pmx_degraded_groups(pmx_plugin* p, char* out, size_t cap, size_t* needed) {
  return guarded([&] { return pmx_detail::give_text(group_lines(p->plugin->degraded_groups()), out, cap, needed); });
}

}  // extern "C"
