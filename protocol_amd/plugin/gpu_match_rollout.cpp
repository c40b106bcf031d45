// gpu_match_rollout.cpp — GpuMatchPlugin::enable_rollout / report_task / flush_rollout and the reads over them (see
// gpu_match_plugin.hpp): the engine's rollout ledger (pm_rollout_*) by node address and task id text.  The twin of the same
// methods of rust/gpu_match_plugin.rs, statement for statement.  (A file of its own: the plugin's other methods are also linked
// against a mock engine that has not these exports.)
#include <algorithm>
#include <shared_mutex>
#include <stdexcept>

#include "group_id_text.hpp"
#include "gpu_match_plugin.hpp"

namespace orchestrator {

namespace {
bool is_hex(char c) { return (c >= '0' && c <= '9') || (c >= 'a' && c <= 'f') || (c >= 'A' && c <= 'F'); }
// the hyphenated form task.id.to_string() gives (8-4-4-4-12), or the 32 digits alone
bool is_uuid_text(const std::string& s) {
  if (s.size() == 32) return std::all_of(s.begin(), s.end(), is_hex);
  if (s.size() != 36) return false;
  for (size_t i = 0; i < 36; ++i) {
    const bool dash = i == 8 || i == 13 || i == 18 || i == 23;
    if (dash ? s[i] != '-' : !is_hex(s[i])) return false;
  }
  return true;
}
}  // namespace

uint64_t GpuMatchPlugin::reported_task_uid(const std::string& task_id) {
  if (is_uuid_text(task_id)) {
    Task t;
    t.id = task_id;
    return task_uid(t);
  }
  uint64_t h = 0xCBF29CE484222325ull;  // FNV-1a, 64 bits
  for (unsigned char c : task_id) h = (h ^ c) * 0x100000001B3ull;
  return h;
}

void GpuMatchPlugin::enable_rollout() {
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);  // (LOCK ORDER: nodes, tasks, rollout, the engine)
  std::lock_guard<std::mutex> lk(rollout_mu_);
  check(pm_rollout_enable(engine_, 1u));
  rollout_ = RolloutQueue{};
}

void GpuMatchPlugin::report_task(const Address& address, const std::optional<std::string>& task_id,
                                 const std::optional<std::string>& task_state) {
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);
  const auto it = nodes_.index.find(address);
  if (it == nodes_.index.end()) return;
  std::lock_guard<std::mutex> lk(rollout_mu_);
  if (task_id && task_state) {  // (Some(task), Some(state), _): node_store.rs:357
    const uint64_t uid = reported_task_uid(*task_id);
    rollout_.texts.emplace(uid, *task_id);  // (the first text of an id stays: a collision is one id, see the header)
    rollout_.reports.push_back(pm_ro_report{it->second, pm_host_task_state(task_state->c_str()), uid});
  } else {  // _ => the three fields are deleted (:369-372)
    rollout_.reports.push_back(pm_ro_report{it->second, PM_TS_NONE, 0ull});
  }
}

void GpuMatchPlugin::flush_rollout_locked() {
  if (rollout_.reports.empty()) return;
  const int32_t rc = pm_rollout_ingest(engine_, rollout_.reports.data(), uint32_t(rollout_.reports.size()));
  rollout_.reports.clear();  // (a refused batch is dropped, not sent again and again)
  check(rc);
}

void GpuMatchPlugin::flush_rollout() {
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);
  std::lock_guard<std::mutex> lk(rollout_mu_);
  flush_rollout_locked();
}

size_t GpuMatchPlugin::queued_task_reports() const {
  std::lock_guard<std::mutex> lk(rollout_mu_);
  return rollout_.reports.size();
}

std::pair<std::vector<uint64_t>, std::vector<uint8_t>> GpuMatchPlugin::reported_tasks(const std::vector<uint32_t>& rows) {
  std::vector<uint64_t> uid(rows.size());
  std::vector<uint8_t> state(rows.size());
  check(pm_rollout_get(engine_, rows.data(), uint32_t(rows.size()), uid.data(), state.data()));
  return {std::move(uid), std::move(state)};
}

size_t GpuMatchPlugin::remembered_task_texts() const {
  std::lock_guard<std::mutex> lk(rollout_mu_);
  return rollout_.texts.size();
}

// the task report; the texts of ids it no longer lists go (a listed id keeps its text also while the task list carries it: a task
// deleted under its reporters renders with the text they sent)
std::vector<pm_ro_task_row> GpuMatchPlugin::rollout_task_rows_locked() {
  uint32_t have = 0;
  const int32_t rc = pm_rollout_tasks(engine_, nullptr, 0u, &have);  // the size query: PM_ERANGE unless there is nothing
  if (rc != PM_ERANGE) check(rc);
  std::vector<pm_ro_task_row> out(have ? have : 1u);
  uint32_t got = 0;
  check(pm_rollout_tasks(engine_, out.data(), uint32_t(out.size()), &got));
  if (got > out.size()) throw std::out_of_range("rollout: the task report grew between two calls");
  out.resize(got);
  std::unordered_map<uint64_t, std::string> kept;
  for (const pm_ro_task_row& r : out) {
    if (r.task != PM_NONE && r.task >= tasks_.size()) throw std::out_of_range("rollout: the engine names a task the plugin has not");
    const auto it = rollout_.texts.find(r.uid);
    if (it != rollout_.texts.end()) kept.emplace(it->first, std::move(it->second));
  }
  rollout_.texts.swap(kept);
  return out;
}

std::string GpuMatchPlugin::rollout_text_locked(uint64_t uid, uint32_t task) const {
  if (task != PM_NONE && task < tasks_.size()) return tasks_[task].id;
  const auto it = rollout_.texts.find(uid);
  return it == rollout_.texts.end() ? hex_lower(uid) : it->second;
}

std::vector<GpuMatchPlugin::TaskRollout> GpuMatchPlugin::task_rollout() {
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);
  std::shared_lock<std::shared_mutex> tasks(tasks_mu_);
  std::lock_guard<std::mutex> lk(rollout_mu_);
  flush_rollout_locked();
  std::vector<TaskRollout> out;
  for (const pm_ro_task_row& r : rollout_task_rows_locked()) {
    TaskRollout t;
    t.task_id = rollout_text_locked(r.uid, r.task);
    t.task_name = r.task != PM_NONE ? tasks_[r.task].name : "unknown";
    t.row = r;
    out.push_back(std::move(t));
  }
  return out;
}

std::vector<GpuMatchPlugin::NodesPerTask> GpuMatchPlugin::nodes_per_task() {
  std::vector<NodesPerTask> out;
  for (const TaskRollout& t : task_rollout()) {
    uint32_t count = 0;
    for (uint32_t s = 0; s < PM_TS_N; ++s) count += t.row.reporters[s];
    if (count) out.push_back(NodesPerTask{t.task_id, t.task_name, count});  // (only tasks with nodes: sync_service.rs:251-256)
  }
  return out;
}

pm_ro_summary GpuMatchPlugin::rollout_summary() {
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);
  std::lock_guard<std::mutex> lk(rollout_mu_);
  flush_rollout_locked();
  pm_ro_summary out{};
  check(pm_rollout_summary(engine_, &out));
  return out;
}

std::vector<GpuMatchPlugin::GroupRollout> GpuMatchPlugin::group_rollout() {
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);
  std::shared_lock<std::shared_mutex> tasks(tasks_mu_);
  std::lock_guard<std::mutex> lk(rollout_mu_);
  flush_rollout_locked();
  uint32_t have = 0;
  const int32_t rc = pm_rollout_groups(engine_, nullptr, 0u, &have);
  if (rc != PM_ERANGE) check(rc);
  std::vector<pm_ro_group_row> rows(have ? have : 1u);
  uint32_t got = 0;
  check(pm_rollout_groups(engine_, rows.data(), uint32_t(rows.size()), &got));
  if (got > rows.size()) throw std::out_of_range("rollout: the group report grew between two calls");
  rows.resize(got);
  std::vector<GroupRollout> out;
  for (const pm_ro_group_row& r : rows) {
    if (r.config >= config_names_.size() || r.task >= tasks_.size())
      throw std::out_of_range("rollout: the engine names a configuration or a task the plugin has not");
    out.push_back(GroupRollout{hex_lower(r.group_id), config_names_[r.config], tasks_[r.task].id, r});
  }
  return out;
}

std::vector<GpuMatchPlugin::NodeRollout> GpuMatchPlugin::rollout_nodes(uint32_t class_mask) {
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);
  std::shared_lock<std::shared_mutex> tasks(tasks_mu_);
  std::lock_guard<std::mutex> lk(rollout_mu_);
  flush_rollout_locked();
  uint32_t have = 0;
  const int32_t rc = pm_rollout_workers(engine_, class_mask, nullptr, 0u, &have);
  if (rc != PM_ERANGE) check(rc);
  std::vector<pm_ro_worker_row> rows(have ? have : 1u);
  uint32_t got = 0;
  check(pm_rollout_workers(engine_, class_mask, rows.data(), uint32_t(rows.size()), &got));
  if (got > rows.size()) throw std::out_of_range("rollout: the node list grew between two calls");
  rows.resize(got);
  // the texts of the reported ids: the task list's where it carries the id (the first row that does), else the remembered one
  std::unordered_map<uint64_t, uint32_t> first;
  for (uint32_t k = uint32_t(tasks_.size()); k-- > 0;) first[task_uid(tasks_[k])] = k;
  std::vector<NodeRollout> out;
  for (const pm_ro_worker_row& r : rows) {
    if (r.worker >= nodes_.rows.size()) throw std::out_of_range("rollout: the engine lists a row the plugin does not know");
    NodeRollout n;
    n.address = nodes_.address_strings[r.worker];
    n.cls = r.cls;
    n.state = r.state;
    if (r.state != PM_TS_NONE) {
      const auto it = r.uid == ~0ull ? first.end() : first.find(r.uid);
      n.task_id = rollout_text_locked(r.uid, it == first.end() ? uint32_t(PM_NONE) : it->second);
    }
    out.push_back(std::move(n));
  }
  return out;
}

}  // namespace orchestrator
