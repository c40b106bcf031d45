// taskdir_host_loop.cpp — the baseline of tools/taskdir_probe.py: what a host does today for one window of the joined task
// listing or for its counters — pm_task_report's three arrays and pm_rollout_tasks fetched whole through the C ABI, a hash-map
// join on the ids of its own task list, the classes, the filter, a sort, the page cut — on one host thread.  (Without duplicate
// ids, which the probe's swarm has none of: a host that has them needs pm_rollout_groups too.)
#include <algorithm>
#include <cstdint>
#include <unordered_map>
#include <vector>

#include "pm_engine.h"

namespace {
std::vector<uint32_t> g_running, g_workers, g_allowed, g_list;
std::vector<pm_ro_task_row> g_ro;
std::vector<pm_tdir_row> g_rows;
std::unordered_map<uint64_t, uint32_t> g_first;
}  // namespace

extern "C" {

// the query of pm_task_directory by the calls a host has without it (the rollout ledger on); uid / created_at / topo_mask: the
// caller's task list.  Returns the engine's error, or PM_OK with totals, by_config [n_cfgs], *n_rows set and the window in rows
int32_t tdir_host_query(pm_engine* e, uint32_t T, uint32_t n_cfgs, const uint64_t* uid, const int64_t* created_at, const uint64_t* topo_mask,
                        const pm_tdir_query* q, pm_tdir_totals* totals, uint32_t* by_config, pm_tdir_row* rows, uint32_t cap_rows,
                        uint32_t* n_rows) {
  g_running.resize(T), g_workers.resize(T), g_allowed.resize(T);
  int32_t rc = pm_task_report(e, g_running.data(), g_workers.data(), g_allowed.data());
  if (rc) return rc;
  uint32_t nr = 0;
  rc = pm_rollout_tasks(e, nullptr, 0, &nr);
  if (rc && rc != PM_ERANGE) return rc;
  g_ro.resize(nr ? nr : 1);
  if ((rc = pm_rollout_tasks(e, g_ro.data(), nr, &nr))) return rc;
  g_first.clear();
  g_first.reserve(T);
  for (uint32_t t = 0; t < T; ++t)
    if (uid[t] != ~0ull) g_first.emplace(uid[t], t);  // (the first row of an id stays)
  g_rows.assign(T, pm_tdir_row{});
  *totals = pm_tdir_totals{};
  for (uint32_t k = 0; k < nr; ++k) {
    const pm_ro_task_row& o = g_ro[k];
    const auto it = o.uid == ~0ull ? g_first.end() : g_first.find(o.uid);
    uint32_t rep = 0;
    for (uint32_t s = 0; s < PM_TS_N; ++s) rep += o.reporters[s];
    if (it == g_first.end()) {
      totals->orphan_uids++, totals->orphan_reporters += rep;
      continue;
    }
    pm_tdir_row& r = g_rows[it->second];
    r.groups_converged = o.groups_converged, r.converged = o.converged;
    std::copy(o.reporters, o.reporters + PM_TS_N, r.reporters);
  }
  const uint64_t valid = n_cfgs >= 64 ? ~0ull : (1ull << n_cfgs) - 1ull;
  g_list.clear();
  totals->tasks = T, totals->n_cfgs = n_cfgs;
  std::fill(by_config, by_config + n_cfgs, 0u);
  for (uint32_t t = 0; t < T; ++t) {
    pm_tdir_row& r = g_rows[t];
    r.uid = uid[t], r.created_at = created_at[t], r.topo_mask = topo_mask[t], r.task = t;
    r.groups_allowed = g_allowed[t], r.groups_running = g_running[t], r.workers_running = g_workers[t];
    r.serve = uint8_t(r.groups_running ? PM_TKS_RUNNING : r.groups_allowed ? PM_TKS_WAITING : PM_TKS_STARVED);
    r.rollout = uint8_t(!r.groups_running ? PM_TKR_UNHELD : r.groups_converged == r.groups_running ? PM_TKR_CONVERGED : PM_TKR_ROLLING);
    const uint64_t m = r.topo_mask & valid;
    if (q->config_mask != ~0ull && !(m & q->config_mask)) continue;
    if (!((q->serve_mask >> r.serve) & 1u) || !((q->rollout_mask >> r.rollout) & 1u)) continue;
    if (r.workers_running < q->workers_min || r.workers_running > q->workers_max) continue;
    uint32_t rep = 0;
    for (uint32_t s = 0; s < PM_TS_N; ++s) rep += r.reporters[s];
    g_list.push_back(t);
    totals->total++, totals->by_serve[r.serve]++, totals->by_rollout[r.rollout]++;
    totals->unrestricted += r.topo_mask == ~0ull, totals->workers_running += r.workers_running, totals->reporters += rep;
    for (uint64_t b = m; b; b &= b - 1ull) by_config[__builtin_ctzll(b)]++;
  }
  const uint32_t n = q->offset >= g_list.size() ? 0u : std::min(q->limit, uint32_t(g_list.size()) - q->offset);
  *n_rows = n;
  if (!n) return PM_OK;  // (the counters alone: no sort)
  if (cap_rows < n) return PM_ERANGE;
  auto reporters = [&](uint32_t t) {
    uint32_t rep = 0;
    for (uint32_t s = 0; s < PM_TS_N; ++s) rep += g_rows[t].reporters[s];
    return rep;
  };
  if (q->order == PM_TDIR_BY_OLDEST) std::reverse(g_list.begin(), g_list.end());
  if (q->order == PM_TDIR_BY_WORKERS_DESC)
    std::stable_sort(g_list.begin(), g_list.end(), [&](uint32_t a, uint32_t b) { return g_rows[a].workers_running > g_rows[b].workers_running; });
  if (q->order == PM_TDIR_BY_REPORTERS_DESC)
    std::stable_sort(g_list.begin(), g_list.end(), [&](uint32_t a, uint32_t b) { return reporters(a) > reporters(b); });
  for (uint32_t k = 0; k < n; ++k) rows[k] = g_rows[g_list[q->offset + k]];
  return PM_OK;
}

}  // extern "C"
