// directory_host_loop.cpp — the baseline of tools/directory_probe.py: what a host does today for one window of the node listing
// or for its counters — three full-table reads through the C ABI (pm_liveness_get over every row, pm_get_groups, pm_rollout_get
// over every row), a std::stable_sort by class or by (class, rank), the join, the page cut — on one host thread.  It flatters
// the reference, which reads every node's hash from Redis for the same list (store/domains/node_store.rs:163-209).
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

#include "pm_engine.h"

namespace {
uint8_t class_of(uint8_t st) {
  return st == PM_NS_HEALTHY ? PM_DC_HEALTHY : st == PM_NS_DISCOVERED ? PM_DC_DISCOVERED : st == PM_NS_DEAD ? PM_DC_DEAD : PM_DC_OTHER;
}
std::vector<uint32_t> g_idx, g_counter, g_members, g_list;
std::vector<uint8_t> g_status, g_state;
std::vector<uint64_t> g_uid;
std::vector<int32_t> g_of;
std::vector<pm_group> g_groups;
}  // namespace

extern "C" {

// the query of pm_directory (membership ANY) by the calls a host has without it; ranks: the caller's address ranks.  Returns
// the engine's error, or PM_OK with *total, counts [PM_NS_N] and *n_rows set and the window in out (cap rows)
int32_t dir_host_query(pm_engine* e, uint32_t W, const uint32_t* ranks, uint32_t status_mask, uint32_t order, uint32_t offset,
                       uint32_t limit, uint32_t* total, uint32_t* counts, pm_dir_row* out, uint32_t cap, uint32_t* n_rows) {
  if (g_idx.size() != W) {
    g_idx.resize(W);
    std::iota(g_idx.begin(), g_idx.end(), 0u);
  }
  g_status.resize(W), g_counter.resize(W), g_state.resize(W), g_uid.resize(W), g_of.resize(W);
  int32_t rc = pm_liveness_get(e, g_idx.data(), W, g_status.data(), g_counter.data());
  if (rc) return rc;
  uint32_t ng = 0, nm = 0;
  if ((rc = pm_get_groups(e, nullptr, nullptr, 0, &ng, nullptr, 0, &nm))) return rc;
  g_groups.resize(ng ? ng : 1), g_members.resize(nm ? nm : 1);
  if ((rc = pm_get_groups(e, g_of.data(), g_groups.data(), ng, &ng, g_members.data(), nm, &nm))) return rc;
  if ((rc = pm_rollout_get(e, g_idx.data(), W, g_uid.data(), g_state.data()))) return rc;
  g_list.clear();
  std::fill(counts, counts + PM_NS_N, 0u);
  for (uint32_t w = 0; w < W; ++w)
    if ((status_mask >> g_status[w]) & 1u) g_list.push_back(w), ++counts[g_status[w]];
  *total = uint32_t(g_list.size());
  const uint32_t n = offset >= g_list.size() ? 0u : std::min(limit, uint32_t(g_list.size()) - offset);
  *n_rows = n;
  if (!n) return PM_OK;  // (the counters alone: no sort)
  if (cap < n) return PM_ERANGE;
  if (order == PM_DIR_BY_ADDRESS)
    std::stable_sort(g_list.begin(), g_list.end(), [&](uint32_t a, uint32_t b) {
      const uint8_t ca = class_of(g_status[a]), cb = class_of(g_status[b]);
      return ca != cb ? ca < cb : ranks[a] < ranks[b];
    });
  else
    std::stable_sort(g_list.begin(), g_list.end(), [&](uint32_t a, uint32_t b) { return class_of(g_status[a]) < class_of(g_status[b]); });
  for (uint32_t k = 0; k < n; ++k) {
    const uint32_t w = g_list[offset + k];
    pm_dir_row r{};
    r.worker = w, r.status = g_status[w], r.cls = class_of(g_status[w]), r.state = g_state[w], r.counter = g_counter[w];
    r.group_slot = PM_NONE, r.group_id = PM_NONE, r.task = PM_NONE, r.uid = g_uid[w];
    if (g_of[w] >= 0) {
      const pm_group& g = g_groups[size_t(g_of[w])];
      r.group_slot = uint32_t(g_of[w]), r.group_id = g.id, r.group_size = g.n_members, r.config = g.config, r.task = g.task;
    }
    out[k] = r;
  }
  return PM_OK;
}

}  // extern "C"
