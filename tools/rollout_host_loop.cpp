// rollout_host_loop.cpp — the baseline of tools/rollout_probe.py: the rollout ledger's ingest and reads as plain C++ on one host
// thread over the same columns (an id and a state per row, the groups' claims by slot), the per-task table in an unordered_map.
// It flatters the reference, which reads every node's hash from Redis for the same scan (metrics/sync_service.rs:243-267).
#include <algorithm>
#include <cstdint>
#include <unordered_map>
#include <vector>

#include "pm_engine.h"

namespace {
std::vector<uint64_t> g_uid;
std::vector<uint8_t> g_state;

struct Acc {
  uint32_t reporters[PM_TS_N] = {};
  uint32_t groups = 0, groups_converged = 0, assigned = 0, converged = 0;
};

uint32_t class_of(uint32_t w, const int32_t* group_of, const uint64_t* g_claim, const uint8_t* g_has) {
  const int32_t g = group_of[w];
  const bool reports = g_state[w] != PM_TS_NONE;
  if (g < 0 || !g_has[g]) return reports ? PM_RO_STRAY : PM_RO_IDLE;
  if (!reports) return PM_RO_SILENT;
  if (g_uid[w] != g_claim[g] || g_uid[w] == ~0ull) return PM_RO_OTHER;
  return g_state[w] == PM_TS_RUNNING ? PM_RO_CONVERGED : PM_RO_BEHIND;
}
}  // namespace

extern "C" {

void ro_host_reset(uint32_t W) {
  g_uid.assign(W, 0);
  g_state.assign(W, uint8_t(PM_TS_NONE));
}

void ro_host_ingest(const pm_ro_report* r, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) {
    g_uid[r[i].worker] = r[i].state == PM_TS_NONE ? 0 : r[i].uid;
    g_state[r[i].worker] = uint8_t(r[i].state);
  }
}

// the classes, the groups' counters [G][PM_TS_N + 2] and the census [PM_RO_N]
void ro_host_classify(const int32_t* group_of, const uint64_t* g_claim, const uint8_t* g_has, uint32_t G, uint8_t* cls, uint32_t* g_cnt,
                      uint32_t* by_class) {
  const uint32_t W = uint32_t(g_uid.size());
  std::fill(g_cnt, g_cnt + size_t(G) * (PM_TS_N + 2), 0u);
  std::fill(by_class, by_class + PM_RO_N, 0u);
  for (uint32_t w = 0; w < W; ++w) {
    const uint32_t c = class_of(w, group_of, g_claim, g_has);
    cls[w] = uint8_t(c);
    ++by_class[c];
    if (c < PM_RO_SILENT) continue;
    uint32_t* cnt = g_cnt + size_t(group_of[w]) * (PM_TS_N + 2);
    ++cnt[c == PM_RO_SILENT ? uint32_t(PM_TS_N) + 1u : c == PM_RO_OTHER ? uint32_t(PM_TS_N) : uint32_t(g_state[w])];
  }
}

// the per-task table, ascending by uid; returns its rows (out may be NULL)
uint32_t ro_host_tasks(const int32_t* group_of, const uint64_t* g_claim, const uint8_t* g_has, const uint32_t* g_size, uint32_t G,
                       pm_ro_task_row* out, uint32_t cap) {
  const uint32_t W = uint32_t(g_uid.size());
  std::unordered_map<uint64_t, Acc> acc;
  std::vector<uint32_t> conv(G, 0);
  for (uint32_t w = 0; w < W; ++w) {
    if (g_state[w] != PM_TS_NONE) ++acc[g_uid[w]].reporters[g_state[w]];
    if (class_of(w, group_of, g_claim, g_has) == PM_RO_CONVERGED) ++conv[size_t(group_of[w])];
  }
  for (uint32_t g = 0; g < G; ++g) {
    if (!g_has[g]) continue;
    Acc& a = acc[g_claim[g]];
    ++a.groups, a.assigned += g_size[g], a.converged += conv[g], a.groups_converged += conv[g] == g_size[g];
  }
  std::vector<uint64_t> ids;
  ids.reserve(acc.size());
  for (const auto& kv : acc) ids.push_back(kv.first);
  std::sort(ids.begin(), ids.end());
  for (uint32_t d = 0; out && d < ids.size() && d < cap; ++d) {
    const Acc& a = acc[ids[d]];
    pm_ro_task_row r{};
    r.uid = ids[d], r.task = PM_NONE, r.groups = a.groups, r.groups_converged = a.groups_converged, r.assigned = a.assigned,
    r.converged = a.converged;
    std::copy(a.reporters, a.reporters + PM_TS_N, r.reporters);
    out[d] = r;
  }
  return uint32_t(ids.size());
}

}  // extern "C"
