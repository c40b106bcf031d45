// groupdir_host_loop.cpp — the baseline of tools/groupdir_probe.py: what a host does today for one window of the joined group
// listing or for its counters — three fetches through the C ABI (pm_get_groups with every member, pm_liveness_get over every
// row, pm_rollout_groups), the join by worker index, the classes, the filter, a sort of the id texts (std::stable_sort over
// strings, as GpuMatchPlugin::get_all_groups sorts them) or of the sizes, the page cut — on one host thread.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <string>
#include <vector>

#include "pm_engine.h"

namespace {
std::vector<uint32_t> g_idx, g_counter, g_members, g_list;
std::vector<uint8_t> g_status;
std::vector<int32_t> g_of;
std::vector<pm_group> g_groups;
std::vector<pm_ro_group_row> g_ro;
std::vector<pm_gdir_row> g_rows;
std::vector<std::string> g_text;
}  // namespace

extern "C" {

// the query of pm_group_directory by the calls a host has without it (both ledgers on).  Returns the engine's error, or PM_OK
// with totals, by_config [n_cfgs], *n_rows, *n_members set and the window in rows / members
int32_t gdir_host_query(pm_engine* e, uint32_t W, uint32_t n_cfgs, const pm_gdir_query* q, pm_gdir_totals* totals, uint32_t* by_config,
                        pm_gdir_row* rows, uint32_t cap_rows, uint32_t* n_rows, uint32_t* members, uint32_t cap_members,
                        uint32_t* n_members) {
  if (g_idx.size() != W) {
    g_idx.resize(W);
    std::iota(g_idx.begin(), g_idx.end(), 0u);
  }
  g_status.resize(W), g_counter.resize(W), g_of.resize(W);
  uint32_t ng = 0, nm = 0, nr = 0;
  int32_t rc = pm_get_groups(e, nullptr, nullptr, 0, &ng, nullptr, 0, &nm);
  if (rc) return rc;
  g_groups.resize(ng ? ng : 1), g_members.resize(nm ? nm : 1);
  if ((rc = pm_get_groups(e, g_of.data(), g_groups.data(), ng, &ng, g_members.data(), nm, &nm))) return rc;
  if ((rc = pm_liveness_get(e, g_idx.data(), W, g_status.data(), g_counter.data()))) return rc;
  rc = pm_rollout_groups(e, nullptr, 0, &nr);
  if (rc && rc != PM_ERANGE) return rc;
  g_ro.resize(nr ? nr : 1);
  if ((rc = pm_rollout_groups(e, g_ro.data(), nr, &nr))) return rc;
  g_rows.assign(ng, pm_gdir_row{});
  for (uint32_t s = 0; s < ng; ++s) {
    const pm_group& g = g_groups[s];
    pm_gdir_row& r = g_rows[s];
    r.group_id = g.id, r.slot = s, r.config = g.config, r.size = g.n_members, r.task = g.task;
    for (uint32_t k = 0; k < g.n_members; ++k) r.by_status[g_status[g_members[g.member_begin + k]]]++;
    const uint32_t lost = r.by_status[PM_NS_DEAD] + r.by_status[PM_NS_EJECTED] + r.by_status[PM_NS_BANNED] + r.by_status[PM_NS_LOWBALANCE];
    r.health = uint8_t(lost ? PM_GH_LOST : r.by_status[PM_NS_HEALTHY] != g.n_members ? PM_GH_DEGRADED : PM_GH_SOUND);
    r.rollout = uint8_t(PM_GR_NO_TASK);
  }
  for (uint32_t k = 0; k < nr; ++k) {
    const pm_ro_group_row& o = g_ro[k];
    pm_gdir_row& r = g_rows[o.slot];
    uint32_t same = 0;
    for (uint32_t s = 0; s < PM_TS_N; ++s) same += o.same[s];
    r.converged = o.same[PM_TS_RUNNING], r.behind = same - o.same[PM_TS_RUNNING], r.other = o.other, r.silent = o.silent;
    r.rollout = uint8_t(r.converged == r.size ? PM_GR_CONVERGED : PM_GR_ROLLING);
  }
  g_list.clear();
  *totals = pm_gdir_totals{};
  totals->n_cfgs = n_cfgs;
  std::fill(by_config, by_config + n_cfgs, 0u);
  for (uint32_t s = 0; s < ng; ++s) {
    const pm_gdir_row& r = g_rows[s];
    if (!((q->config_mask >> r.config) & 1ull)) continue;
    if (q->holds != PM_GDIR_ANY && (q->holds == PM_GDIR_WITH_TASK) != (r.task != PM_NONE)) continue;
    if (r.size < q->size_min || r.size > q->size_max) continue;
    if (!((q->health_mask >> r.health) & 1u) || !((q->rollout_mask >> r.rollout) & 1u)) continue;
    g_list.push_back(s);
    totals->total++, totals->members_total += r.size, totals->by_health[r.health]++, totals->by_rollout[r.rollout]++;
    by_config[r.config]++;
  }
  const uint32_t n = q->offset >= g_list.size() ? 0u : std::min(q->limit, uint32_t(g_list.size()) - q->offset);
  *n_rows = n, *n_members = 0;
  if (!n) return PM_OK;  // (the counters alone: no sort)
  if (cap_rows < n) return PM_ERANGE;
  if (q->order == PM_GDIR_BY_ID_TEXT) {
    g_text.resize(ng);
    char buf[20];
    for (const uint32_t s : g_list) {
      std::snprintf(buf, sizeof(buf), "%llx", (unsigned long long)g_rows[s].group_id);
      g_text[s] = buf;
    }
    std::stable_sort(g_list.begin(), g_list.end(), [&](uint32_t a, uint32_t b) { return g_text[a] < g_text[b]; });
  } else if (q->order == PM_GDIR_BY_SIZE_DESC) {
    std::stable_sort(g_list.begin(), g_list.end(), [&](uint32_t a, uint32_t b) { return g_rows[a].size > g_rows[b].size; });
  }
  uint32_t m = 0;
  for (uint32_t k = 0; k < n; ++k) {
    const uint32_t s = g_list[q->offset + k];
    rows[k] = g_rows[s];
    rows[k].member_begin = m;
    if (m + g_rows[s].size > cap_members) return PM_ERANGE;
    std::copy(g_members.begin() + g_groups[s].member_begin, g_members.begin() + g_groups[s].member_begin + g_rows[s].size, members + m);
    m += g_rows[s].size;
  }
  *n_members = m;
  return PM_OK;
}

}  // extern "C"
