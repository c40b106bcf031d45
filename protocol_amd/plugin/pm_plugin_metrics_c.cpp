// pm_plugin_metrics_c.cpp — see pm_plugin_c.h "metrics": the C face of GpuMatchPlugin's metrics methods.  (A file of its own:
// pm_plugin_c.cpp is also linked against a mock engine that has not these exports.)
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "pm_plugin_c.h"
#include "pm_plugin_c_internal.hpp"

using namespace orchestrator;

namespace {
std::vector<GpuMatchPlugin::MetricEntry> entries_of(const char* const* task_ids, const char* const* labels, const double* values,
                                                    uint32_t n) {
  std::vector<GpuMatchPlugin::MetricEntry> out;
  for (uint32_t k = 0; k < n; ++k) out.push_back(GpuMatchPlugin::MetricEntry{task_ids[k], labels[k], values[k]});
  return out;
}
std::string hex_double(double v) {  // "%a": every bit of the value
  char buf[64];
  std::snprintf(buf, sizeof(buf), "%a", v);
  return buf;
}
template <typename F>
int32_t guarded(F&& f) {
  try {
    return f();
  } catch (const std::exception& e) {
    pmx_detail::set_error(e.what());
    return -1;
  }
}
}  // namespace

extern "C" {

int32_t pmx_enable_metrics(pmx_plugin* p) {
  return guarded([&] { return p->plugin->enable_metrics(), 0; });
}

int32_t pmx_beat_metrics(pmx_plugin* p, const char* address, const char* const* task_ids, const char* const* labels,
                         const double* values, uint32_t n) {
  return guarded([&] { return p->plugin->beat_metrics(Address(address), entries_of(task_ids, labels, values, n)), 0; });
}

int32_t pmx_store_metrics(pmx_plugin* p, const char* address, const char* const* task_ids, const char* const* labels,
                          const double* values, uint32_t n) {
  return guarded([&] { return p->plugin->store_metrics(Address(address), entries_of(task_ids, labels, values, n)), 0; });
}

int32_t pmx_store_manual_metric(pmx_plugin* p, const char* label, double value) {
  return guarded([&] { return p->plugin->store_manual_metric(label, value), 0; });
}

int32_t pmx_delete_metric(pmx_plugin* p, const char* task_id, const char* label, const char* address) {
  return guarded([&] { return p->plugin->delete_metric(task_id, label, Address(address)), 0; });
}

int32_t pmx_clear_metrics(pmx_plugin* p, const char* address) {
  return guarded([&] { return p->plugin->clear_metrics(Address(address)), 0; });
}

int32_t pmx_flush_metrics(pmx_plugin* p) {
  return guarded([&] { return p->plugin->flush_metrics(), 0; });
}

int32_t pmx_aggregate_metrics(pmx_plugin* p, const char* task_id, char* out, size_t cap, size_t* needed) {
  return guarded([&] {
    std::string text;
    for (const auto& kv : task_id ? p->plugin->aggregate_metrics_for_task(task_id) : p->plugin->aggregate_metrics_for_all_tasks())
      text += kv.first + "\t" + hex_double(kv.second) + "\n";
    return pmx_detail::give_text(text, out, cap, needed);
  });
}

int32_t pmx_metrics_for_node(pmx_plugin* p, const char* address, char* out, size_t cap, size_t* needed) {
  return guarded([&] {
    std::string text;
    for (const auto& task : p->plugin->metrics_for_node(Address(address)))
      for (const auto& kv : task.second) text += task.first + "\t" + kv.first + "\t" + hex_double(kv.second) + "\n";
    return pmx_detail::give_text(text, out, cap, needed);
  });
}

int32_t pmx_synced_metrics(pmx_plugin* p, const char* const* task_ids, const char* const* task_names, uint32_t n_tasks, char* out,
                           size_t cap, size_t* needed) {
  return guarded([&] {
    std::map<std::string, std::string> names;
    for (uint32_t k = 0; k < n_tasks; ++k) names[task_ids[k]] = task_names[k];
    std::string text;
    for (const auto& m : p->plugin->synced_metrics(names))
      text += m.address + "\t" + m.task_id + "\t" + m.task_name + "\t" + m.label + "\t" + hex_double(m.value) + "\t" +
              (m.group_id ? *m.group_id : "-") + "\t" + (m.group_config_name ? *m.group_config_name : "-") + "\n";
    return pmx_detail::give_text(text, out, cap, needed);
  });
}

}  // extern "C"
