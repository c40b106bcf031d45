// mock_rollout.cpp — TEST INFRASTRUCTURE: the rollout exports of include/pm_engine.h (pm_rollout_enable / _ingest / _get /
// _summary / _tasks / _groups / _workers), which tests/cpp/mock_engine.cpp does not define.  A sequential ledger that follows the
// header (the reports applied one after another, the reads by brute force), a log of every call, and the last batch as it
// arrived.  The join's other side is what the test says (mock_rollout::groups, mock_rollout::task_uids).
#include <cstdint>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "pm_engine.h"

namespace mock_rollout {
struct Group {
  uint64_t id;
  uint32_t config, task;  // task: position in task_uids or PM_NONE
  std::vector<uint32_t> members;
};
std::mutex mu;
bool on = false;
uint32_t W = 0;
int32_t fail_ingest_with = PM_OK;                      // != PM_OK: the next ingest returns it (once)
std::map<uint32_t, std::pair<uint64_t, uint32_t>> rows;  // worker -> (uid, state)
std::vector<Group> groups;                             // in pm_get_groups order
std::vector<uint64_t> task_uids;                       // the current list
std::vector<std::string> calls;                        // "enable 1", "ingest n=..", "summary", "tasks", "groups", "workers mask=.."
std::vector<pm_ro_report> last_reports;

static uint32_t position_of(uint64_t uid) {
  if (uid == ~0ull) return PM_NONE;
  for (size_t k = 0; k < task_uids.size(); ++k)
    if (task_uids[k] == uid) return uint32_t(k);
  return PM_NONE;
}
static int slot_of(uint32_t w) {
  for (size_t s = 0; s < groups.size(); ++s)
    for (uint32_t m : groups[s].members)
      if (m == w) return int(s);
  return -1;
}
static uint32_t class_of(uint32_t w) {
  const int s = slot_of(w);
  const auto it = rows.find(w);
  if (s < 0 || groups[size_t(s)].task == PM_NONE) return it == rows.end() ? PM_RO_IDLE : PM_RO_STRAY;
  if (it == rows.end()) return PM_RO_SILENT;
  const uint64_t claimed = task_uids[groups[size_t(s)].task];
  if (it->second.first != claimed || claimed == ~0ull) return PM_RO_OTHER;
  return it->second.second == PM_TS_RUNNING ? PM_RO_CONVERGED : PM_RO_BEHIND;
}
static pm_ro_group_row group_row(uint32_t s) {
  const Group& g = groups[s];
  pm_ro_group_row r{};
  r.group_id = g.id, r.slot = s, r.config = g.config, r.task = g.task, r.size = uint32_t(g.members.size());
  for (uint32_t w : g.members) {
    const uint32_t c = class_of(w);
    if (c == PM_RO_SILENT) ++r.silent;
    else if (c == PM_RO_OTHER) ++r.other;
    else ++r.same[rows.at(w).second];
  }
  return r;
}
static std::vector<pm_ro_task_row> task_rows() {
  std::set<uint64_t> ids;
  for (const auto& kv : rows) ids.insert(kv.second.first);
  for (const Group& g : groups)
    if (g.task != PM_NONE) ids.insert(task_uids[g.task]);
  std::vector<pm_ro_task_row> out;
  for (uint64_t uid : ids) {
    pm_ro_task_row r{};
    r.uid = uid, r.task = position_of(uid);
    for (const auto& kv : rows)
      if (kv.second.first == uid) ++r.reporters[kv.second.second];
    for (uint32_t s = 0; s < groups.size(); ++s) {
      if (groups[s].task == PM_NONE || task_uids[groups[s].task] != uid) continue;
      const pm_ro_group_row g = group_row(s);
      ++r.groups, r.assigned += g.size, r.converged += g.same[PM_TS_RUNNING];
      r.groups_converged += g.same[PM_TS_RUNNING] == g.size;
    }
    out.push_back(r);
  }
  return out;
}
}  // namespace mock_rollout

extern "C" {

int32_t pm_rollout_enable(pm_engine*, uint32_t on) {
  using namespace mock_rollout;
  std::lock_guard<std::mutex> lk(mu);
  mock_rollout::on = on != 0;
  rows.clear();
  calls.push_back("enable " + std::to_string(on));
  return PM_OK;
}

int32_t pm_rollout_ingest(pm_engine*, const pm_ro_report* reports, uint32_t n) {
  using namespace mock_rollout;
  std::lock_guard<std::mutex> lk(mu);
  calls.push_back("ingest n=" + std::to_string(n));
  last_reports.assign(reports, reports + (reports ? n : 0u));
  if (fail_ingest_with != PM_OK) {
    const int32_t rc = fail_ingest_with;
    fail_ingest_with = PM_OK;
    return rc;
  }
  if (!on) return PM_ESTATE;
  for (uint32_t i = 0; i < n; ++i) {
    if (reports[i].state >= PM_TS_N && reports[i].state != PM_TS_NONE) return PM_EINVAL;
    if (reports[i].worker >= W) return PM_ERANGE;
  }
  for (uint32_t i = 0; i < n; ++i) {
    if (reports[i].state == PM_TS_NONE) rows.erase(reports[i].worker);
    else rows[reports[i].worker] = {reports[i].uid, reports[i].state};
  }
  return PM_OK;
}

int32_t pm_rollout_get(pm_engine*, const uint32_t* idx, uint32_t n, uint64_t* uid, uint8_t* state) {
  using namespace mock_rollout;
  std::lock_guard<std::mutex> lk(mu);
  if (!on) return PM_ESTATE;
  for (uint32_t k = 0; k < n; ++k) {
    if (idx[k] >= W) return PM_ERANGE;
    const auto it = rows.find(idx[k]);
    if (uid) uid[k] = it == rows.end() ? 0ull : it->second.first;
    if (state) state[k] = it == rows.end() ? uint8_t(PM_TS_NONE) : uint8_t(it->second.second);
  }
  return PM_OK;
}

int32_t pm_rollout_summary(pm_engine*, pm_ro_summary* out) {
  using namespace mock_rollout;
  std::lock_guard<std::mutex> lk(mu);
  if (!on) return PM_ESTATE;
  if (!out) return PM_EINVAL;
  calls.push_back("summary");
  *out = pm_ro_summary{};
  for (uint32_t w = 0; w < W; ++w) {
    ++out->by_class[class_of(w)];
    const auto it = rows.find(w);
    ++out->by_state[it == rows.end() ? uint32_t(PM_TS_N) : it->second.second];
  }
  for (uint32_t s = 0; s < groups.size(); ++s) {
    if (groups[s].task == PM_NONE) continue;
    const pm_ro_group_row g = group_row(s);
    ++out->groups_with_task;
    out->groups_converged += g.same[PM_TS_RUNNING] == g.size;
  }
  out->distinct_uids = uint32_t(task_rows().size());
  return PM_OK;
}

int32_t pm_rollout_tasks(pm_engine*, pm_ro_task_row* out, uint32_t cap, uint32_t* n) {
  using namespace mock_rollout;
  std::lock_guard<std::mutex> lk(mu);
  if (!on) return PM_ESTATE;
  if (!n) return PM_EINVAL;
  calls.push_back("tasks");
  const std::vector<pm_ro_task_row> list = task_rows();
  *n = uint32_t(list.size());
  if (!list.empty() && (!out || cap < list.size())) return PM_ERANGE;
  for (size_t i = 0; i < list.size(); ++i) out[i] = list[i];
  return PM_OK;
}

int32_t pm_rollout_groups(pm_engine*, pm_ro_group_row* out, uint32_t cap, uint32_t* n) {
  using namespace mock_rollout;
  std::lock_guard<std::mutex> lk(mu);
  if (!on) return PM_ESTATE;
  if (!n) return PM_EINVAL;
  calls.push_back("groups");
  std::vector<pm_ro_group_row> list;
  for (uint32_t s = 0; s < groups.size(); ++s)
    if (groups[s].task != PM_NONE) list.push_back(group_row(s));
  *n = uint32_t(list.size());
  if (!list.empty() && (!out || cap < list.size())) return PM_ERANGE;
  for (size_t i = 0; i < list.size(); ++i) out[i] = list[i];
  return PM_OK;
}

int32_t pm_rollout_workers(pm_engine*, uint32_t class_mask, pm_ro_worker_row* out, uint32_t cap, uint32_t* n) {
  using namespace mock_rollout;
  std::lock_guard<std::mutex> lk(mu);
  if (!on) return PM_ESTATE;
  if (!n || !class_mask || (class_mask >> PM_RO_N)) return PM_EINVAL;
  calls.push_back("workers mask=" + std::to_string(class_mask));
  std::vector<pm_ro_worker_row> list;
  for (uint32_t w = 0; w < W; ++w) {
    const uint32_t c = class_of(w);
    if (!((class_mask >> c) & 1u)) continue;
    pm_ro_worker_row r{};
    const int s = slot_of(w);
    const auto it = rows.find(w);
    r.worker = w, r.group_slot = s < 0 ? uint32_t(PM_NONE) : uint32_t(s), r.cls = uint8_t(c);
    r.uid = it == rows.end() ? 0ull : it->second.first;
    r.state = it == rows.end() ? uint8_t(PM_TS_NONE) : uint8_t(it->second.second);
    list.push_back(r);
  }
  *n = uint32_t(list.size());
  if (!list.empty() && (!out || cap < list.size())) return PM_ERANGE;
  for (size_t i = 0; i < list.size(); ++i) out[i] = list[i];
  return PM_OK;
}

}  // extern "C"
