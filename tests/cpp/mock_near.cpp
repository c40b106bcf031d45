// mock_near.cpp — TEST INFRASTRUCTURE: the nearest-candidates export of include/pm_engine.h (pm_nearest_workers), which
// tests/cpp/mock_engine.cpp does not define.  It records what it was asked and answers canned values that
// tests/cpp/near_test.cpp derives from the query, so that a row under the wrong address or configuration shows.
#include <cfloat>
#include <cstdint>
#include <vector>

#include "pm_engine.h"

namespace mock_near {
uint32_t n_workers = 0, n_cfgs = 0;  // what the mock engine holds
int32_t fail_with = PM_OK;           // != PM_OK: every call returns it
bool seed_finds_nobody = false;      // PM_NEAR_SEED: the empty row
struct Asked {
  uint32_t origin, config, pool, k;
};
std::vector<Asked> asked;
uint32_t seed_row(uint32_t config) { return 2u + config; }
uint32_t listed(uint32_t k) { return k < 5u ? k : 5u; }
uint32_t worker_at(uint32_t origin, uint32_t j) { return (origin + 3u * j + 1u) % n_workers; }
double km_at(uint32_t config, uint32_t j) { return j == 4u ? DBL_MAX : 1.5 * j + 0.25 + 1000.0 * config; }
}  // namespace mock_near

extern "C" {

int32_t pm_nearest_workers(pm_engine*, const pm_near_query* q, uint32_t n_q, uint32_t pool, uint32_t k, pm_near_row* rows,
                           uint32_t* workers, double* km) {
  using namespace mock_near;
  if (fail_with != PM_OK) return fail_with;
  if (k == 0 || k > PM_NEAR_MAX_K || pool > PM_NEAR_ELIGIBLE || (n_q && (!q || !rows || !workers))) return PM_EINVAL;
  for (uint32_t i = 0; i < n_q; ++i)
    if ((q[i].origin >= n_workers && q[i].origin != PM_NEAR_SEED) || q[i].config >= n_cfgs) return PM_ERANGE;
  for (uint32_t i = 0; i < n_q; ++i) {
    asked.push_back({q[i].origin, q[i].config, pool, k});
    const bool none = q[i].origin == PM_NEAR_SEED && seed_finds_nobody;
    const uint32_t origin = none ? PM_NONE : q[i].origin == PM_NEAR_SEED ? seed_row(q[i].config) : q[i].origin;
    const uint32_t n = none ? 0u : listed(k);
    rows[i] = pm_near_row{origin, n, none ? 0u : 10u + pool, none ? 0u : 7u};
    for (uint32_t j = 0; j < k; ++j) {
      workers[i * k + j] = j < n ? worker_at(origin, j) : PM_NONE;
      if (km) km[i * k + j] = j < n ? km_at(q[i].config, j) : DBL_MAX;
    }
  }
  return PM_OK;
}

}  // extern "C"
