// mock_taskdir.cpp — TEST INFRASTRUCTURE: the task directory's export of include/pm_engine.h (pm_task_directory), which
// tests/cpp/mock_engine.cpp does not define.  The tasks are what the test says (mock_taskdir::tasks: a pm_tdir_row a live task in
// list order with its classes and columns; the orphans beside them); the call filters, orders and cuts them by brute force as
// the header says, and logs every query.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <mutex>
#include <string>
#include <vector>

#include "pm_engine.h"

namespace mock_taskdir {
std::mutex mu;
bool rollout_on = true;  // a rollout filter other than "all", or the order by reporters, over a ledger that is off: PM_ESTATE
uint32_t n_cfgs = 0, orphan_uids = 0, orphan_reporters = 0;
std::vector<pm_tdir_row> tasks;  // by position
std::vector<std::string> calls;  // "cfg=.. serve=.. rollout=.. workers=..-.. order=.. off=.. lim=.. caps=<cfgs>/<rows>"
}  // namespace mock_taskdir

static uint32_t reporters_of(const pm_tdir_row& r) {
  uint32_t n = 0;
  for (uint32_t s = 0; s < PM_TS_N; ++s) n += r.reporters[s];
  return n;
}

extern "C" {

int32_t pm_task_directory(pm_engine*, const pm_tdir_query* q, pm_tdir_totals* totals, uint32_t* by_config, uint32_t cap_cfgs,
                          pm_tdir_row* rows, uint32_t cap_rows, uint32_t* n_rows) {
  using namespace mock_taskdir;
  std::lock_guard<std::mutex> lk(mu);
  if (!q || !totals || !n_rows) return PM_EINVAL;
  if (!q->config_mask || !q->serve_mask || (q->serve_mask >> PM_TKS_N) || !q->rollout_mask || (q->rollout_mask >> PM_TKR_N) ||
      q->order > PM_TDIR_BY_REPORTERS_DESC || q->workers_min > q->workers_max)
    return PM_EINVAL;
  if (!rollout_on && (q->rollout_mask != 7u || q->order == PM_TDIR_BY_REPORTERS_DESC)) return PM_ESTATE;
  char cfg[20];
  std::snprintf(cfg, sizeof(cfg), "%llx", (unsigned long long)q->config_mask);
  calls.push_back(std::string("cfg=") + cfg + " serve=" + std::to_string(q->serve_mask) + " rollout=" + std::to_string(q->rollout_mask) +
                  " workers=" + std::to_string(q->workers_min) + "-" + std::to_string(q->workers_max) + " order=" +
                  std::to_string(q->order) + " off=" + std::to_string(q->offset) + " lim=" + std::to_string(q->limit) + " caps=" +
                  std::to_string(cap_cfgs) + "/" + std::to_string(cap_rows));
  const uint64_t valid = n_cfgs >= 64 ? ~0ull : (1ull << n_cfgs) - 1ull;
  std::vector<uint32_t> list;
  *totals = pm_tdir_totals{};
  totals->tasks = uint32_t(tasks.size());
  totals->n_cfgs = n_cfgs;
  totals->orphan_uids = rollout_on ? orphan_uids : 0u;
  totals->orphan_reporters = rollout_on ? orphan_reporters : 0u;
  std::vector<uint32_t> cfg_count(n_cfgs, 0u);
  for (uint32_t t = 0; t < tasks.size(); ++t) {
    const pm_tdir_row& r = tasks[t];
    if (q->config_mask != ~0ull && !(r.topo_mask & valid & q->config_mask)) continue;
    if (!((q->serve_mask >> r.serve) & 1u)) continue;
    if (rollout_on && !((q->rollout_mask >> r.rollout) & 1u)) continue;
    if (r.workers_running < q->workers_min || r.workers_running > q->workers_max) continue;
    list.push_back(t);
    totals->total++;
    totals->by_serve[r.serve]++;
    if (rollout_on) totals->by_rollout[r.rollout]++;
    totals->unrestricted += r.topo_mask == ~0ull;
    totals->workers_running += r.workers_running;
    totals->reporters += reporters_of(r);
    for (uint32_t c = 0; c < n_cfgs; ++c) cfg_count[c] += uint32_t((r.topo_mask >> c) & 1ull);
  }
  if (q->order == PM_TDIR_BY_OLDEST) std::reverse(list.begin(), list.end());
  if (q->order == PM_TDIR_BY_WORKERS_DESC)
    std::stable_sort(list.begin(), list.end(), [&](uint32_t a, uint32_t b) { return tasks[a].workers_running > tasks[b].workers_running; });
  if (q->order == PM_TDIR_BY_REPORTERS_DESC)
    std::stable_sort(list.begin(), list.end(), [&](uint32_t a, uint32_t b) { return reporters_of(tasks[a]) > reporters_of(tasks[b]); });
  const uint32_t n = q->offset >= list.size() ? 0u : std::min(q->limit, uint32_t(list.size()) - q->offset);
  *n_rows = n;
  if (by_config && cap_cfgs < n_cfgs) return PM_ERANGE;
  if (by_config) std::copy(cfg_count.begin(), cfg_count.end(), by_config);
  if (n && (!rows || cap_rows < n)) return PM_ERANGE;
  for (uint32_t k = 0; k < n; ++k) {
    rows[k] = tasks[list[q->offset + k]];
    rows[k].task = list[q->offset + k];
  }
  return PM_OK;
}

}  // extern "C"
