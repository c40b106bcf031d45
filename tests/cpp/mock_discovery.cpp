// mock_discovery.cpp — TEST INFRASTRUCTURE: pm_discovery_sync of include/pm_engine.h, which tests/cpp/mock_engine.cpp does not
// define.  The reference's pass read literally over the mock ledger of tests/cpp/mock_liveness.cpp: one row after the other,
// every row counting the other Healthy rows on its endpoint as the rows before it left them (the D x W loop) — so that
// tests/cpp/discovery_test.cpp can check what the plugin hands over and what it makes of the results.  apply is recorded, not
// carried out.
#include <atomic>
#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

#include "pm_engine.h"

namespace mock_liveness {
extern std::mutex mu;
extern bool on;
extern std::atomic<uint32_t> W;
extern std::vector<uint8_t> status;
extern std::vector<uint32_t> counter;
extern std::vector<std::string> calls;
}  // namespace mock_liveness

namespace mock_discovery {
std::vector<uint32_t> last_column;   // row_endpoint of the last call
std::vector<pm_disc_row> last_rows;
uint32_t last_n_endpoints = 0;
int32_t fail_with = PM_OK;
}  // namespace mock_discovery

extern "C" int32_t pm_discovery_sync(pm_engine*, uint64_t now, const uint32_t* row_endpoint, uint32_t n_endpoints, uint32_t max_same,
                                     const pm_disc_row* rows, uint32_t n_rows, uint32_t apply, pm_disc_result* out, uint32_t* total) {
  using namespace mock_liveness;
  std::lock_guard<std::mutex> lk(mu);
  if (mock_discovery::fail_with != PM_OK) return mock_discovery::fail_with;
  if (!on) return PM_ESTATE;
  const uint32_t Wn = W.load();
  if (status.size() < Wn) status.resize(Wn, PM_NS_HEALTHY), counter.resize(Wn, 0u);
  if ((n_rows && !rows) || (Wn && !row_endpoint) || uint64_t(n_endpoints) > uint64_t(Wn) + 2ull * n_rows) return PM_EINVAL;
  std::vector<bool> seen(Wn, false);
  for (uint32_t j = 0; j < n_rows; ++j) {
    const pm_disc_row& r = rows[j];
    if (r.flags & ~63u) return PM_EINVAL;
    if (r.row != PM_DISC_NEW && r.row >= Wn) return PM_ERANGE;
    if (r.endpoint >= n_endpoints || (r.row != PM_DISC_NEW && r.endpoint_after >= n_endpoints)) return PM_ERANGE;
    if (r.row != PM_DISC_NEW) {
      if (seen[r.row]) return PM_EINVAL;
      seen[r.row] = true;
    }
  }
  for (uint32_t w = 0; w < Wn; ++w)
    if (row_endpoint[w] != PM_EP_NONE && row_endpoint[w] >= n_endpoints) return PM_ERANGE;
  calls.push_back("discovery now=" + std::to_string(now) + " rows=" + std::to_string(n_rows) + " max=" + std::to_string(max_same) +
                  " apply=" + std::to_string(apply));
  mock_discovery::last_column.assign(row_endpoint, row_endpoint + Wn);
  mock_discovery::last_rows.assign(rows, rows + n_rows);
  mock_discovery::last_n_endpoints = n_endpoints;
  std::vector<uint32_t> ep(row_endpoint, row_endpoint + Wn);
  uint32_t sum = 0;
  for (uint32_t j = 0; j < n_rows; ++j) {
    const pm_disc_row& r = rows[j];
    pm_disc_result o{};
    for (int k = 0; k < 3; ++k) o.upd_old[k] = o.upd_new[k] = PM_NS_N;
    for (uint32_t w = 0; w < Wn; ++w)
      if (w != r.row && ep[w] == r.endpoint && status[w] == PM_NS_HEALTHY) ++o.healthy_same_endpoint;  // monitor.rs:218-234
    if (r.row == PM_DISC_NEW) {
      const bool admit = o.healthy_same_endpoint < max_same;
      o.old_status = PM_NS_N;
      o.final_status = admit ? uint8_t(PM_NS_DISCOVERED) : uint8_t(PM_NS_N);
      o.ops = admit ? PM_DO_ADMIT : PM_DO_SKIP;
    } else {
      const uint8_t s = status[r.row];
      uint8_t cur = s;
      bool stamp = false;
      auto update = [&](uint8_t to) { o.upd_old[o.n_updates] = cur, o.upd_new[o.n_updates] = to, ++o.n_updates, cur = to, stamp = true; };
      const bool validated = r.flags & PM_DF_VALIDATED, white = r.flags & PM_DF_WHITELISTED, active = r.flags & PM_DF_ACTIVE;
      o.old_status = s;
      if (o.healthy_same_endpoint > 0 && s != PM_NS_HEALTHY) {
        update(PM_NS_DEAD);
      } else {
        if (validated && !white) update(PM_NS_EJECTED);
        if (validated && white && s == PM_NS_EJECTED) update(PM_NS_DEAD);
        if (!active && s == PM_NS_HEALTHY &&
            (r.last_change_ms == 0 || (now > r.last_change_ms && now - r.last_change_ms > PM_DISC_GRACE_MS)))
          update(white ? PM_NS_DEAD : PM_NS_EJECTED);
        if (r.endpoint_after != ep[r.row]) cur = s, stamp = false, o.ops |= PM_DO_IP_REWRITE;
        if (r.flags & PM_DF_LOCATION_NEW) o.ops |= PM_DO_LOCATION;
        if (s == PM_NS_DEAD && r.last_change_ms && r.last_updated_ms && r.last_change_ms < r.last_updated_ms) {
          if (r.flags & PM_DF_SPECS_DIFFER) cur = s, stamp = false, o.ops |= PM_DO_SPECS_REWRITE;
          update(PM_NS_DISCOVERED);
        }
        if (r.flags & PM_DF_BALANCE_ZERO) update(PM_NS_LOWBALANCE);
      }
      if ((o.ops & PM_DO_IP_REWRITE) && !(o.ops & PM_DO_SPECS_REWRITE)) ep[r.row] = r.endpoint_after;
      if (stamp) o.ops |= PM_DO_STAMP_NOW;
      o.final_status = cur;
      status[r.row] = cur;
      sum += o.n_updates;
    }
    if (out) out[j] = o;
  }
  if (total) *total = sum;
  return PM_OK;
}
