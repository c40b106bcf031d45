// mock_adopt.cpp — TEST INFRASTRUCTURE: the exports of include/pm_engine.h that GpuMatchPlugin::restore_groups calls and
// tests/cpp/mock_engine.cpp does not define (pm_adopt_groups, pm_group_id_state, pm_match).  Each records its arguments for
// tests/cpp/restore_test.cpp; none of them matches anything.
#include <cstdint>
#include <vector>

#include "pm_engine.h"

namespace mock_adopt {
struct AdoptCall {
  std::vector<pm_group> groups;
  std::vector<uint32_t> members;
  uint64_t id_state = 0;
};
std::vector<AdoptCall> adopt_calls;
uint32_t match_calls = 0;
uint64_t id_state_answer = 0;
}  // namespace mock_adopt

extern "C" {

int32_t pm_adopt_groups(pm_engine*, const pm_group* groups, uint32_t n_groups, const uint32_t* members, uint32_t n_members,
                        uint64_t id_state) {
  mock_adopt::AdoptCall c;
  if (n_groups) c.groups.assign(groups, groups + n_groups);
  if (n_members) c.members.assign(members, members + n_members);
  c.id_state = id_state;
  mock_adopt::adopt_calls.push_back(c);
  return PM_OK;
}

int32_t pm_group_id_state(pm_engine*, uint64_t* state) {
  *state = mock_adopt::id_state_answer;
  return PM_OK;
}

int32_t pm_match(pm_engine*, uint32_t*, uint32_t*) {
  ++mock_adopt::match_calls;
  return PM_OK;
}

}  // extern "C"
