// pm_plugin_rollout_c.cpp — see pm_plugin_c.h "rollout": the C face of GpuMatchPlugin's rollout methods.  (A file of its own:
// pm_plugin_c.cpp is also linked against a mock engine that has not these exports.)
#include <optional>
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
std::optional<std::string> opt(const char* s) { return s ? std::optional<std::string>(s) : std::nullopt; }
template <typename T>
std::string words(const T* p, size_t n) {
  std::string out;
  for (size_t k = 0; k < n; ++k) out += "\t" + std::to_string(p[k]);
  return out;
}
}  // namespace

extern "C" {

int32_t pmx_enable_rollout(pmx_plugin* p) {
  return guarded([&] { return p->plugin->enable_rollout(), 0; });
}

int32_t pmx_report_task(pmx_plugin* p, const char* address, const char* task_id, const char* task_state) {
  return guarded([&] { return p->plugin->report_task(Address(address), opt(task_id), opt(task_state)), 0; });
}

int32_t pmx_flush_rollout(pmx_plugin* p) {
  return guarded([&] { return p->plugin->flush_rollout(), 0; });
}

int32_t pmx_nodes_per_task(pmx_plugin* p, char* out, size_t cap, size_t* needed) {
  return guarded([&] {
    std::string text;
    for (const auto& t : p->plugin->nodes_per_task()) text += t.task_id + "\t" + t.task_name + "\t" + std::to_string(t.count) + "\n";
    return pmx_detail::give_text(text, out, cap, needed);
  });
}

int32_t pmx_rollout_summary(pmx_plugin* p, pm_ro_summary* out) {
  return guarded([&] {
    if (!out) throw std::invalid_argument("null argument");
    *out = p->plugin->rollout_summary();
    return 0;
  });
}

int32_t pmx_task_rollout(pmx_plugin* p, char* out, size_t cap, size_t* needed) {
  return guarded([&] {
    std::string text;
    for (const auto& t : p->plugin->task_rollout())
      text += t.task_id + "\t" + t.task_name + "\t" + (t.row.task == PM_NONE ? "-" : std::to_string(t.row.task)) + "\t" +
              std::to_string(t.row.groups) + "\t" + std::to_string(t.row.groups_converged) + "\t" + std::to_string(t.row.assigned) +
              "\t" + std::to_string(t.row.converged) + words(t.row.reporters, PM_TS_N) + "\n";
    return pmx_detail::give_text(text, out, cap, needed);
  });
}

int32_t pmx_group_rollout(pmx_plugin* p, char* out, size_t cap, size_t* needed) {
  return guarded([&] {
    std::string text;
    for (const auto& g : p->plugin->group_rollout())
      text += g.group_id + "\t" + g.configuration_name + "\t" + g.task_id + "\t" + std::to_string(g.row.size) +
              words(g.row.same, PM_TS_N) + "\t" + std::to_string(g.row.other) + "\t" + std::to_string(g.row.silent) + "\n";
    return pmx_detail::give_text(text, out, cap, needed);
  });
}

int32_t pmx_rollout_nodes(pmx_plugin* p, uint32_t class_mask, char* out, size_t cap, size_t* needed) {
  return guarded([&] {
    std::string text;
    for (const auto& n : p->plugin->rollout_nodes(class_mask))
      text += n.address + "\t" + std::to_string(n.cls) + "\t" + (n.task_id ? std::to_string(n.state) : "-") + "\t" +
              (n.task_id ? *n.task_id : "-") + "\n";
    return pmx_detail::give_text(text, out, cap, needed);
  });
}

}  // extern "C"
