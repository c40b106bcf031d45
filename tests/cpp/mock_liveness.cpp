// mock_liveness.cpp — TEST INFRASTRUCTURE: the liveness exports of include/pm_engine.h (pm_liveness_enable / _set / _get /
// _sweep / _transitions), which tests/cpp/mock_engine.cpp does not define.  A small ledger that follows the header's table, so
// that tests/cpp/liveness_test.cpp can check the statuses the plugin ends on, and a log of every call with what it was given.
// The mock engine's row count is not visible from here: the test says how many rows there are (mock_liveness::W, never more
// than the plugin's node table holds); rows start Healthy, as the test's nodes are.  apply is recorded, not carried out.
#include <atomic>
#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

#include "pm_engine.h"

namespace mock_liveness {
std::mutex mu;
bool on = false;
uint32_t m = 0, enables = 0;
std::atomic<uint32_t> W{0};
int32_t fail_with = PM_OK;           // != PM_OK: every sweep returns it
std::vector<uint8_t> status;
std::vector<uint32_t> counter;
std::vector<pm_live_row> list;       // the last sweep's
std::vector<std::string> calls;      // "enable m=3", "sweep now=.. apply=1 pool=null|bits", "transitions cap=..", "get w=..", "set w=.. s=.. c=.."
std::vector<uint64_t> last_pool;     // the pool words of the last sweep (empty = NULL)
uint32_t extra_row = PM_NONE;        // != PM_NONE: the next sweep also lists this row (one the node table may not hold)

static void cover(uint32_t rows) {
  if (status.size() < rows) status.resize(rows, PM_NS_HEALTHY), counter.resize(rows, 0u);
}
}  // namespace mock_liveness

extern "C" {

int32_t pm_liveness_enable(pm_engine*, uint32_t on, uint32_t threshold) {
  using namespace mock_liveness;
  std::lock_guard<std::mutex> lk(mu);
  ++enables;
  mock_liveness::on = on != 0;
  m = threshold;
  status.clear(), counter.clear(), list.clear();
  calls.push_back("enable m=" + std::to_string(threshold));
  return PM_OK;
}

int32_t pm_liveness_set(pm_engine*, const uint32_t* idx, const uint8_t* st, const uint32_t* cnt, uint32_t n) {
  using namespace mock_liveness;
  std::lock_guard<std::mutex> lk(mu);
  if (!on) return PM_ESTATE;
  cover(W.load());
  for (uint32_t k = 0; k < n; ++k) {
    if (idx[k] >= status.size()) return PM_ERANGE;
    if (st[k] >= PM_NS_N) return PM_EINVAL;
  }
  for (uint32_t k = 0; k < n; ++k) {
    status[idx[k]] = st[k], counter[idx[k]] = cnt ? cnt[k] : 0u;
    calls.push_back("set w=" + std::to_string(idx[k]) + " s=" + std::to_string(st[k]) + " c=" + std::to_string(counter[idx[k]]));
  }
  return PM_OK;
}

int32_t pm_liveness_get(pm_engine*, const uint32_t* idx, uint32_t n, uint8_t* st, uint32_t* cnt) {
  using namespace mock_liveness;
  std::lock_guard<std::mutex> lk(mu);
  if (!on) return PM_ESTATE;
  cover(W.load());
  for (uint32_t k = 0; k < n; ++k)
    if (idx[k] >= status.size()) return PM_ERANGE;
  for (uint32_t k = 0; k < n; ++k) {
    if (st) st[k] = status[idx[k]];
    if (cnt) cnt[k] = counter[idx[k]];
    calls.push_back("get w=" + std::to_string(idx[k]));
  }
  return PM_OK;
}

int32_t pm_liveness_sweep(pm_engine*, uint64_t now, const uint64_t* beat, const uint64_t* pool, uint32_t apply, uint32_t* n_out,
                          uint32_t* census) {
  using namespace mock_liveness;
  std::lock_guard<std::mutex> lk(mu);
  if (fail_with != PM_OK) return fail_with;
  if (!on) return PM_ESTATE;
  const uint32_t rows = W.load();
  if (rows && !beat) return PM_EINVAL;
  cover(rows);
  calls.push_back("sweep now=" + std::to_string(now) + " apply=" + std::to_string(apply) + " pool=" + (pool ? "bits" : "null"));
  last_pool.assign(pool, pool + (pool ? (rows + 63u) / 64u : 0u));
  list.clear();
  uint32_t cen[PM_NS_N] = {0};
  for (uint32_t w = 0; w < rows; ++w) {
    const bool present = beat[w] != 0 && (beat[w] > now || now - beat[w] <= PM_LIVE_TTL_MS);
    const bool in_pool = pool ? ((pool[w >> 6] >> (w & 63u)) & 1u) != 0 : true;
    const uint8_t s = status[w];
    uint8_t ns = s;
    bool listed = false;
    uint32_t c = counter[w];
    if (present) {
      if (s == PM_NS_UNHEALTHY || s == PM_NS_WAITING || s == PM_NS_DISCOVERED || s == PM_NS_DEAD)
        ns = in_pool ? PM_NS_HEALTHY : PM_NS_DISCOVERED, listed = true;
      c = 0;
    } else {
      c = c == UINT32_MAX ? c : c + 1;
      if (s == PM_NS_HEALTHY) ns = PM_NS_UNHEALTHY;
      else if (s == PM_NS_UNHEALTHY && c >= m) ns = PM_NS_DEAD;
      else if (s == PM_NS_DISCOVERED && in_pool) ns = PM_NS_UNHEALTHY;
      else if (s == PM_NS_DISCOVERED && c > PM_LIVE_GIVE_UP) ns = PM_NS_DEAD;
      else if (s == PM_NS_WAITING && c >= m) ns = PM_NS_UNHEALTHY;
      listed = ns != s;
    }
    status[w] = ns, counter[w] = c;
    if (listed) list.push_back(pm_live_row{w, s, ns, 0, c});
    ++cen[ns];
  }
  if (extra_row != PM_NONE) list.push_back(pm_live_row{extra_row, PM_NS_HEALTHY, PM_NS_UNHEALTHY, 0, 1}), extra_row = PM_NONE;
  if (n_out) *n_out = uint32_t(list.size());
  if (census)
    for (uint32_t k = 0; k < PM_NS_N; ++k) census[k] = cen[k];
  return PM_OK;
}

int32_t pm_liveness_transitions(pm_engine*, pm_live_row* rows, uint32_t cap, uint32_t* n) {
  using namespace mock_liveness;
  std::lock_guard<std::mutex> lk(mu);
  if (!on) return PM_ESTATE;
  calls.push_back("transitions cap=" + std::to_string(cap));
  if (n) *n = uint32_t(list.size());
  if (!rows || cap < list.size()) return PM_ERANGE;
  for (size_t i = 0; i < list.size(); ++i) rows[i] = list[i];
  return PM_OK;
}

}  // extern "C"
