// mock_metrics.cpp — TEST INFRASTRUCTURE: the metrics exports of include/pm_engine.h (pm_metrics_enable / _ingest / _totals /
// _rows), which tests/cpp/mock_engine.cpp does not define.  A sequential ledger that follows the header (a map per row, the
// beats applied one after another), so that tests/cpp/metrics_test.cpp can check what the plugin reads back, a log of every call,
// and the last batch as it arrived.  The join's other side is what the test says (mock_metrics::group_of_row).
#include <cstdint>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "pm_engine.h"

namespace mock_metrics {
std::mutex mu;
bool on = false;
uint32_t W = 0, n_series = 0;
int32_t fail_ingest_with = PM_OK;                          // != PM_OK: the next ingest returns it (once)
std::map<uint32_t, std::map<uint32_t, double>> rows;       // internal row (0 = the manual row, w + 1) -> series -> value
std::map<uint32_t, std::pair<uint64_t, uint32_t>> group_of_row;  // worker -> (group id, configuration)
std::vector<std::string> calls;                            // "enable 1", "ingest beats=.. entries=.. series=..", "totals", "rows all|n=.."
std::vector<pm_mx_beat> last_beats;
std::vector<pm_mx_entry> last_entries;
}  // namespace mock_metrics

extern "C" {

int32_t pm_metrics_enable(pm_engine*, uint32_t on) {
  using namespace mock_metrics;
  std::lock_guard<std::mutex> lk(mu);
  mock_metrics::on = on != 0;
  rows.clear();
  n_series = 0;
  calls.push_back("enable " + std::to_string(on));
  return PM_OK;
}

int32_t pm_metrics_ingest(pm_engine*, const pm_mx_beat* beats, uint32_t n_beats, const pm_mx_entry* entries, uint32_t n_entries,
                          uint32_t series) {
  using namespace mock_metrics;
  std::lock_guard<std::mutex> lk(mu);
  calls.push_back("ingest beats=" + std::to_string(n_beats) + " entries=" + std::to_string(n_entries) + " series=" + std::to_string(series));
  last_beats.assign(beats, beats + n_beats);
  last_entries.assign(entries, entries + (entries ? n_entries : 0u));
  if (fail_ingest_with != PM_OK) {
    const int32_t rc = fail_ingest_with;
    fail_ingest_with = PM_OK;
    return rc;
  }
  if (!on) return PM_ESTATE;
  for (uint32_t b = 0; b < n_beats; ++b) {
    if (beats[b].kind > PM_MXB_DELETE || uint64_t(beats[b].first) + beats[b].n > n_entries) return PM_EINVAL;
    if (beats[b].row != PM_MX_MANUAL && beats[b].row >= W) return PM_ERANGE;
    for (uint32_t j = beats[b].first; j < beats[b].first + beats[b].n; ++j)
      if (entries[j].series >= series) return PM_ERANGE;
  }
  auto next = rows;
  for (uint32_t b = 0; b < n_beats; ++b) {
    std::map<uint32_t, double>& node = next[beats[b].row + 1u];
    const pm_mx_entry* const e = entries + beats[b].first;
    if (beats[b].kind == PM_MXB_DELETE) {
      for (uint32_t j = 0; j < beats[b].n; ++j) node.erase(e[j].series);
      continue;
    }
    if (beats[b].kind == PM_MXB_REPLACE)
      for (auto it = node.begin(); it != node.end();) {
        bool named = false;
        for (uint32_t j = 0; j < beats[b].n; ++j) named = named || e[j].series == it->first;
        it = named ? std::next(it) : node.erase(it);
      }
    for (uint32_t j = 0; j < beats[b].n; ++j) {
      const auto at = node.find(e[j].series);
      if (at == node.end()) {
        if (node.size() >= PM_MX_ROW_MAX) return PM_ERANGE;
        node[e[j].series] = e[j].value;
      } else if (!(e[j].flags & PM_MXF_MAX) || e[j].value > at->second) {
        at->second = e[j].value;
      }
    }
  }
  rows.swap(next);
  if (series > n_series) n_series = series;
  return PM_OK;
}

int32_t pm_metrics_totals(pm_engine*, double* sum, uint32_t* count, uint32_t cap, uint32_t* out_series) {
  using namespace mock_metrics;
  std::lock_guard<std::mutex> lk(mu);
  if (!on) return PM_ESTATE;
  if (!out_series) return PM_EINVAL;
  calls.push_back("totals");
  *out_series = n_series;
  if (n_series && (!sum || !count || cap < n_series)) return PM_ERANGE;
  for (uint32_t s = 0; s < n_series; ++s) sum[s] = 0.0, count[s] = 0u;
  for (const auto& row : rows)  // (ascending internal row: the manual row first)
    for (const auto& kv : row.second) sum[kv.first] += kv.second, ++count[kv.first];
  return PM_OK;
}

int32_t pm_metrics_rows(pm_engine*, const uint32_t* named, uint32_t n, pm_mx_row* out, uint32_t cap, uint32_t* n_out) {
  using namespace mock_metrics;
  std::lock_guard<std::mutex> lk(mu);
  if (!on) return PM_ESTATE;
  calls.push_back(named ? "rows n=" + std::to_string(n) : std::string("rows all"));
  std::vector<pm_mx_row> list;
  const auto give = [&](uint32_t internal) {
    const auto it = rows.find(internal);
    if (it == rows.end()) return;
    for (const auto& kv : it->second) {
      pm_mx_row r{internal ? internal - 1u : uint32_t(PM_MX_MANUAL), kv.first, kv.second, uint64_t(PM_NONE), 0u, 0u};
      const auto g = group_of_row.find(r.row);
      if (internal && g != group_of_row.end()) r.group_id = g->second.first, r.config = g->second.second;
      list.push_back(r);
    }
  };
  if (named) {
    for (uint32_t k = 0; k < n; ++k) {
      if (named[k] != PM_MX_MANUAL && named[k] >= W) return PM_ERANGE;
      give(named[k] + 1u);
    }
  } else {
    for (const auto& row : rows) give(row.first);
  }
  if (n_out) *n_out = uint32_t(list.size());
  if (!list.empty() && (!out || cap < list.size())) return PM_ERANGE;
  for (size_t i = 0; i < list.size(); ++i) out[i] = list[i];
  return PM_OK;
}

}  // extern "C"
