// mock_report.cpp — TEST INFRASTRUCTURE: the diagnostics exports of include/pm_engine.h (pm_explain_workers, pm_config_report,
// pm_task_report), which tests/cpp/mock_engine.cpp does not define.  Each records what it was asked and answers canned values
// that tests/cpp/report_test.cpp derives from the arguments, so that a wrong row, configuration or position shows.
#include <cstdint>
#include <vector>

#include "pm_engine.h"

namespace mock_report {
std::vector<uint32_t> explained;  // worker rows pm_explain_workers was asked for
uint32_t n_cfgs = 0;              // what the mock engine holds
uint32_t n_tasks = 0;
uint32_t state_answer = PM_WS_IDLE;
int32_t fail_with = PM_OK;        // != PM_OK: every call returns it
}  // namespace mock_report

extern "C" {

// why[i][c] = (row + c) % PM_WHY_N
int32_t pm_explain_workers(pm_engine*, const uint32_t* workers, uint32_t n, uint8_t* why, uint32_t* state) {
  if (mock_report::fail_with != PM_OK) return mock_report::fail_with;
  for (uint32_t i = 0; i < n; ++i) {
    mock_report::explained.push_back(workers[i]);
    for (uint32_t c = 0; c < mock_report::n_cfgs && why; ++c) why[size_t(i) * mock_report::n_cfgs + c] = uint8_t((workers[i] + c) % PM_WHY_N);
    if (state) state[i] = mock_report::state_answer;
  }
  return PM_OK;
}

// row c: every field a distinct function of c
int32_t pm_config_report(pm_engine*, pm_config_report_row* out, uint32_t cap, uint32_t* n_cfgs) {
  if (mock_report::fail_with != PM_OK) return mock_report::fail_with;
  if (n_cfgs) *n_cfgs = mock_report::n_cfgs;
  if (cap < mock_report::n_cfgs) return PM_ERANGE;
  for (uint32_t c = 0; c < mock_report::n_cfgs; ++c) {
    pm_config_report_row& r = out[c];
    r.enabled = c & 1u;
    r.eligible_meets = 100 + c;
    r.idle_meets = 200 + c;
    for (uint32_t k = 0; k < PM_WHY_N; ++k) r.why[k] = k == 0 ? r.eligible_meets : 1000 * c + k;
    r.groups = 300 + c;
    r.members = 400 + c;
    r.groups_without_task = 500 + c;
    r.tasks_allowing = 600 + c;
  }
  return PM_OK;
}

// position t: running t, workers 10 t, allowed 100 t
int32_t pm_task_report(pm_engine*, uint32_t* groups_running, uint32_t* workers_running, uint32_t* groups_allowed) {
  if (mock_report::fail_with != PM_OK) return mock_report::fail_with;
  for (uint32_t t = 0; t < mock_report::n_tasks; ++t) {
    if (groups_running) groups_running[t] = t;
    if (workers_running) workers_running[t] = 10 * t;
    if (groups_allowed) groups_allowed[t] = 100 * t;
  }
  return PM_OK;
}

}  // extern "C"
