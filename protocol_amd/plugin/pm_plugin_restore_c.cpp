// pm_plugin_restore_c.cpp — see pm_plugin_c.h "restart and switch-over": the C face of GpuMatchPlugin::restore_groups,
// group_tasks and group_id_state.  (A file of its own: pm_plugin_c.cpp is also linked against a mock engine that has no
// pm_adopt_groups.)
#include <algorithm>
#include <string>
#include <vector>

#include "pm_plugin_c.h"
#include "pm_plugin_c_internal.hpp"

using namespace orchestrator;

namespace {

// the tab-separated fields of one line, with pm_plugin_c.cpp's escapes (\\ \t \n) undone
std::vector<std::string> fields(const std::string& line) {
  std::vector<std::string> out(1);
  for (size_t i = 0; i < line.size(); ++i) {
    const char c = line[i];
    if (c == '\t') {
      out.emplace_back();
    } else if (c == '\\' && i + 1 < line.size()) {
      const char n = line[++i];
      out.back() += n == 't' ? '\t' : n == 'n' ? '\n' : n;
    } else {
      out.back() += c;
    }
  }
  return out;
}

std::vector<std::vector<std::string>> lines(const char* text) {
  std::vector<std::vector<std::string>> out;
  const std::string s = text ? text : "";
  size_t at = 0;
  while (at < s.size()) {
    size_t end = s.find('\n', at);
    if (end == std::string::npos) end = s.size();
    if (end > at) out.push_back(fields(s.substr(at, end - at)));
    at = end + 1;
  }
  return out;
}

}  // namespace

extern "C" {

int32_t pmx_restore_groups(pmx_plugin* p, const char* groups, const char* group_tasks, uint32_t has_id_state, uint64_t id_state) {
  try {
    std::vector<NodeGroup> gs;
    for (const std::vector<std::string>& f : lines(groups)) {
      if (f.size() < 3) throw std::invalid_argument("pmx_restore_groups: a group line has fewer than three fields");
      NodeGroup g;
      g.id = f[0];
      g.configuration_name = f[1];
      g.created_at = std::stoll(f[2]);
      g.nodes.assign(f.begin() + 3, f.end());
      gs.push_back(std::move(g));
    }
    std::unordered_map<std::string, std::string> tasks;
    for (const std::vector<std::string>& f : lines(group_tasks)) {
      if (f.size() != 2) throw std::invalid_argument("pmx_restore_groups: a group_task line is not <group id>\\t<task id>");
      tasks[f[0]] = f[1];
    }
    const GpuMatchPlugin::RestoreReport r =
        p->plugin->restore_groups(gs, tasks, has_id_state ? std::optional<uint64_t>(id_state) : std::nullopt);
    std::string text;
    for (const auto& d : r.dropped) text += "dropped\t" + d.first + "\t" + d.second + "\n";
    for (const std::string& id : r.task_cleared) text += "task_cleared\t" + id + "\n";
    p->restore_report = text;
    return 0;
  } catch (const std::exception& e) {
    pmx_detail::set_error(e.what());
    return -1;
  }
}

int32_t pmx_take_restore_report(pmx_plugin* p, char* out, size_t cap, size_t* needed) {
  return pmx_detail::give_text(p->restore_report, out, cap, needed);
}

int32_t pmx_group_tasks(pmx_plugin* p, char* out, size_t cap, size_t* needed) {
  try {
    const std::unordered_map<std::string, std::string> m = p->plugin->group_tasks();
    std::vector<std::pair<std::string, std::string>> sorted(m.begin(), m.end());
    std::sort(sorted.begin(), sorted.end());
    std::string text;
    for (const auto& kv : sorted) text += kv.first + "\t" + kv.second + "\n";
    return pmx_detail::give_text(text, out, cap, needed);
  } catch (const std::exception& e) {
    pmx_detail::set_error(e.what());
    return -1;
  }
}

int32_t pmx_group_id_state(pmx_plugin* p, uint64_t* state) {
  if (!state) {
    pmx_detail::set_error("null argument");
    return -1;
  }
  try {
    *state = p->plugin->group_id_state();
    return 0;
  } catch (const std::exception& e) {
    pmx_detail::set_error(e.what());
    return -1;
  }
}

void pmx_set_multi_gpu(pmx_plugin* p, uint32_t on) { p->plugin->multi_gpu = on != 0; }

}  // extern "C"
