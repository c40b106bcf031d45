// metrics_host_loop.cpp — what tools/metrics_probe.py times beside pm_metrics_ingest / _totals / _rows: the same calls as plain
// C++ on one host thread, an unordered_map per node (series -> value) where the reference keeps a Redis hash per node behind a
// round trip per field, so it flatters the reference.  Compiled by the probe (g++ -O2 -shared); not part of the product.
#include <cstdint>
#include <unordered_map>
#include <vector>

#include "pm_engine.h"

namespace {
std::vector<std::unordered_map<uint32_t, double>> g_rows;  // internal row: 0 = the manual row, w + 1
}

extern "C" {

void mx_host_reset(uint32_t W) { g_rows.assign(size_t(W) + 1, {}); }

void mx_host_ingest(const pm_mx_beat* beats, uint32_t n_beats, const pm_mx_entry* entries) {
  for (uint32_t b = 0; b < n_beats; ++b) {
    auto& node = g_rows[beats[b].row + 1u];
    const pm_mx_entry* const e = entries + beats[b].first;
    if (beats[b].kind == PM_MXB_DELETE) {
      for (uint32_t j = 0; j < beats[b].n; ++j) node.erase(e[j].series);
      continue;
    }
    if (beats[b].kind == PM_MXB_REPLACE)  // heartbeat.rs:109-140: the keys the beat does not name go first
      for (auto it = node.begin(); it != node.end();) {
        bool named = false;
        for (uint32_t j = 0; j < beats[b].n && !named; ++j) named = e[j].series == it->first;
        it = named ? std::next(it) : node.erase(it);
      }
    for (uint32_t j = 0; j < beats[b].n; ++j) {
      const auto at = node.find(e[j].series);
      if (at == node.end()) node.emplace(e[j].series, e[j].value);
      else if (!(e[j].flags & PM_MXF_MAX) || e[j].value > at->second) at->second = e[j].value;
    }
  }
}

void mx_host_totals(double* sum, uint32_t* count, uint32_t n_series) {
  for (uint32_t s = 0; s < n_series; ++s) sum[s] = 0.0, count[s] = 0u;
  for (const auto& node : g_rows)
    for (const auto& kv : node) sum[kv.first] += kv.second, ++count[kv.first];
}

// the listing with its join: group_of / g_id / g_cfg as the sync service's two plugin calls and its hash join would leave them
uint32_t mx_host_rows(const int32_t* group_of, const uint64_t* g_id, const uint32_t* g_cfg, pm_mx_row* out) {
  uint32_t n = 0;
  for (size_t r = 0; r < g_rows.size(); ++r)
    for (const auto& kv : g_rows[r]) {
      pm_mx_row o{r ? uint32_t(r - 1) : uint32_t(PM_MX_MANUAL), kv.first, kv.second, uint64_t(PM_NONE), 0u, 0u};
      if (r && group_of[r - 1] >= 0) o.group_id = g_id[group_of[r - 1]], o.config = g_cfg[group_of[r - 1]];
      out[n++] = o;
    }
  return n;
}

}  // extern "C"
