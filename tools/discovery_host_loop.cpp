// discovery_host_loop.cpp — what tools/discovery_probe.py times beside pm_discovery_sync: the reference-shaped pass
// (discovery/monitor.rs:218-435) on one host thread — for every discovery row a scan of all nodes for the Healthy others on its
// endpoint, then the row's steps — with integer endpoint ids where the reference compares strings behind a Redis round trip per
// row, so it flatters the reference.  Compiled by the probe (g++ -O2 -shared); not part of the product.
#include <cstdint>
#include <vector>

#include "pm_engine.h"

extern "C" uint32_t disc_host_pass(uint64_t now, uint32_t W, const uint8_t* status_in, const uint32_t* row_endpoint, uint32_t max_same,
                                   const pm_disc_row* rows, uint32_t D, uint8_t* final_status, uint32_t* cnt_out) {
  std::vector<uint8_t> status(status_in, status_in + W);
  std::vector<uint32_t> ep(row_endpoint, row_endpoint + W);
  uint32_t total = 0;
  for (uint32_t j = 0; j < D; ++j) {
    const pm_disc_row& r = rows[j];
    uint32_t cnt = 0;
    for (uint32_t w = 0; w < W; ++w) cnt += (ep[w] == r.endpoint) & (status[w] == PM_NS_HEALTHY) & (w != r.row);
    cnt_out[j] = cnt;
    if (r.row == PM_DISC_NEW) {
      final_status[j] = cnt >= max_same ? uint8_t(PM_NS_N) : uint8_t(PM_NS_DISCOVERED);
      continue;
    }
    const uint8_t s = status[r.row];
    uint8_t cur = s;
    uint32_t ops = 0;
    const bool validated = r.flags & PM_DF_VALIDATED, white = r.flags & PM_DF_WHITELISTED, active = r.flags & PM_DF_ACTIVE;
    if (cnt > 0 && s != PM_NS_HEALTHY) {
      cur = PM_NS_DEAD, ++total;
    } else {
      if (validated && !white) cur = PM_NS_EJECTED, ++total;
      if (validated && white && s == PM_NS_EJECTED) cur = PM_NS_DEAD, ++total;
      if (!active && s == PM_NS_HEALTHY && (r.last_change_ms == 0 || (now > r.last_change_ms && now - r.last_change_ms > PM_DISC_GRACE_MS)))
        cur = white ? PM_NS_DEAD : PM_NS_EJECTED, ++total;
      if (r.endpoint_after != ep[r.row]) cur = s, ops |= PM_DO_IP_REWRITE;
      if (s == PM_NS_DEAD && r.last_change_ms && r.last_updated_ms && r.last_change_ms < r.last_updated_ms) {
        if (r.flags & PM_DF_SPECS_DIFFER) cur = s, ops |= PM_DO_SPECS_REWRITE;
        cur = PM_NS_DISCOVERED, ++total;
      }
      if (r.flags & PM_DF_BALANCE_ZERO) cur = PM_NS_LOWBALANCE, ++total;
    }
    if ((ops & PM_DO_IP_REWRITE) && !(ops & PM_DO_SPECS_REWRITE)) ep[r.row] = r.endpoint_after;
    status[r.row] = cur;
    final_status[j] = cur;
  }
  return total;
}
