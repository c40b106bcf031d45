// mock_groupdir.cpp — TEST INFRASTRUCTURE: the group directory's export of include/pm_engine.h (pm_group_directory), which
// tests/cpp/mock_engine.cpp does not define.  The groups are what the test says (mock_groupdir::groups: a pm_gdir_row a live
// group in slot order with its classes and counters, and its members in the order the call lays them out); the call filters,
// orders and cuts them by brute force as the header says, and logs every query.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <mutex>
#include <string>
#include <vector>

#include "pm_engine.h"

namespace mock_groupdir {
struct G {
  pm_gdir_row row;
  std::vector<uint32_t> members;
};
std::mutex mu;
bool live_on = true, rollout_on = true;  // a class filter other than "all" over a ledger that is off: PM_ESTATE
uint32_t n_cfgs = 0;
std::vector<G> groups;           // by slot
std::vector<std::string> calls;  // "cfg=.. holds=.. size=..-.. health=.. rollout=.. order=.. off=.. lim=.. caps=<cfgs>/<rows>/<members>"
}  // namespace mock_groupdir

static std::string hex_text(uint64_t v) {
  char s[20];
  std::snprintf(s, sizeof(s), "%llx", (unsigned long long)v);
  return s;
}

extern "C" {

int32_t pm_group_directory(pm_engine*, const pm_gdir_query* q, pm_gdir_totals* totals, uint32_t* by_config, uint32_t cap_cfgs,
                           pm_gdir_row* rows, uint32_t cap_rows, uint32_t* n_rows, uint32_t* members, uint32_t cap_members,
                           uint32_t* n_members) {
  using namespace mock_groupdir;
  std::lock_guard<std::mutex> lk(mu);
  if (!q || !totals || !n_rows || !n_members) return PM_EINVAL;
  if (!q->config_mask || !q->health_mask || (q->health_mask >> PM_GH_N) || !q->rollout_mask || (q->rollout_mask >> PM_GR_N) ||
      q->holds > PM_GDIR_WITHOUT_TASK || q->order > PM_GDIR_BY_SIZE_DESC || q->size_min > q->size_max)
    return PM_EINVAL;
  if ((!live_on && q->health_mask != 7u) || (!rollout_on && q->rollout_mask != 7u)) return PM_ESTATE;
  calls.push_back("cfg=" + hex_text(q->config_mask) + " holds=" + std::to_string(q->holds) + " size=" + std::to_string(q->size_min) + "-" +
                  std::to_string(q->size_max) + " health=" + std::to_string(q->health_mask) + " rollout=" + std::to_string(q->rollout_mask) +
                  " order=" + std::to_string(q->order) + " off=" + std::to_string(q->offset) + " lim=" + std::to_string(q->limit) +
                  " caps=" + std::to_string(cap_cfgs) + "/" + std::to_string(cap_rows) + "/" + std::to_string(cap_members));
  std::vector<uint32_t> list;
  *totals = pm_gdir_totals{};
  totals->n_cfgs = n_cfgs;
  std::vector<uint32_t> cfg_count(n_cfgs, 0u);
  for (uint32_t s = 0; s < groups.size(); ++s) {
    const pm_gdir_row& r = groups[s].row;
    const bool held = r.task != PM_NONE;
    if (!((q->config_mask >> r.config) & 1ull)) continue;
    if (q->holds != PM_GDIR_ANY && (q->holds == PM_GDIR_WITH_TASK) != held) continue;
    if (r.size < q->size_min || r.size > q->size_max) continue;
    if (live_on && !((q->health_mask >> r.health) & 1u)) continue;
    if (rollout_on && !((q->rollout_mask >> r.rollout) & 1u)) continue;
    list.push_back(s);
    totals->total++;
    totals->members_total += r.size;
    if (live_on) totals->by_health[r.health]++;
    if (rollout_on) totals->by_rollout[r.rollout]++;
    if (r.config < n_cfgs) cfg_count[r.config]++;
  }
  if (q->order == PM_GDIR_BY_ID_TEXT)
    std::stable_sort(list.begin(), list.end(),
                     [&](uint32_t a, uint32_t b) { return hex_text(groups[a].row.group_id) < hex_text(groups[b].row.group_id); });
  if (q->order == PM_GDIR_BY_SIZE_DESC)
    std::stable_sort(list.begin(), list.end(), [&](uint32_t a, uint32_t b) { return groups[a].row.size > groups[b].row.size; });
  const uint32_t n = q->offset >= list.size() ? 0u : std::min(q->limit, uint32_t(list.size()) - q->offset);
  *n_rows = n;
  uint32_t m = 0;
  for (uint32_t k = 0; k < n; ++k) m += uint32_t(groups[list[q->offset + k]].members.size());
  *n_members = m;
  if (by_config && cap_cfgs < n_cfgs) return PM_ERANGE;
  if (by_config) std::copy(cfg_count.begin(), cfg_count.end(), by_config);
  if (n && (!rows || cap_rows < n)) return PM_ERANGE;
  if (members && cap_members < m) return PM_ERANGE;
  m = 0;
  for (uint32_t k = 0; k < n; ++k) {
    const G& g = groups[list[q->offset + k]];
    rows[k] = g.row;
    rows[k].member_begin = m;
    if (members) std::copy(g.members.begin(), g.members.end(), members + m);
    m += uint32_t(g.members.size());
  }
  return PM_OK;
}

}  // extern "C"
