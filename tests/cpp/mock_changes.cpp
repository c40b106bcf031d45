// mock_changes.cpp — TEST INFRASTRUCTURE: the change feed's exports of include/pm_engine.h (pm_enable_assignment_changes,
// pm_drain_assignment_changes), which tests/cpp/mock_engine.cpp does not define.  A scripted feed: tests/cpp/changes_test.cpp
// fills `pending`, and may have the list grow behind a refused call — what a publish between a size query and its drain does.
#include <cstdint>
#include <vector>

#include "pm_engine.h"

namespace mock_changes {
bool on = false;
bool resync = false;                 // the next successful drain reports PM_CHANGES_RESYNC
int32_t fail_with = PM_OK;           // != PM_OK: every drain returns it
std::vector<pm_change_row> pending;  // ascending by worker, as the engine keeps them
std::vector<std::vector<pm_change_row>> grow_behind_refusal;  // one entry joins `pending` behind each refused call
uint32_t refused = 0, drained = 0, enables = 0;
std::vector<uint32_t> caps;          // the cap of every call
}  // namespace mock_changes

extern "C" {

int32_t pm_enable_assignment_changes(pm_engine*, uint32_t on) {
  using namespace mock_changes;
  ++enables;
  mock_changes::on = on != 0;
  if (!on) pending.clear();
  resync = on != 0;
  return PM_OK;
}

int32_t pm_drain_assignment_changes(pm_engine*, pm_change_row* rows, uint32_t cap, uint32_t* n, uint32_t* flags) {
  using namespace mock_changes;
  if (fail_with != PM_OK) return fail_with;
  if (!on) return PM_ESTATE;
  caps.push_back(cap);
  if (n) *n = uint32_t(pending.size());
  if (flags) *flags = resync ? PM_CHANGES_RESYNC : 0u;
  if (!rows || cap < pending.size()) {
    ++refused;
    if (!grow_behind_refusal.empty()) {
      pending.insert(pending.end(), grow_behind_refusal.front().begin(), grow_behind_refusal.front().end());
      grow_behind_refusal.erase(grow_behind_refusal.begin());
    }
    return PM_ERANGE;
  }
  for (size_t i = 0; i < pending.size(); ++i) rows[i] = pending[i];
  pending.clear();
  resync = false;
  ++drained;
  return PM_OK;
}

}  // extern "C"
