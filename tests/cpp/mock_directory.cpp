// mock_directory.cpp — TEST INFRASTRUCTURE: the node directory's export of include/pm_engine.h (pm_directory), which
// tests/cpp/mock_engine.cpp does not define.  The rows are what the test says (mock_directory::rows, one pm_dir_row a worker:
// status, counter, group fields, state; mock_directory::ranks); the call filters, orders and cuts them by brute force as the
// header says, and logs every query.
#include <algorithm>
#include <cstdint>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "pm_engine.h"

namespace mock_directory {
std::mutex mu;
bool on = true;                  // false: PM_ESTATE (liveness off)
std::vector<pm_dir_row> rows;    // by worker
std::vector<uint32_t> ranks;     // by worker
std::vector<std::string> calls;  // "mask=.. mem=.. order=.. off=.. lim=.. cap=.."
}  // namespace mock_directory

extern "C" {

int32_t pm_directory(pm_engine*, const pm_dir_query* q, uint32_t* total, uint32_t* counts, pm_dir_row* out, uint32_t cap,
                     uint32_t* n_rows) {
  using namespace mock_directory;
  std::lock_guard<std::mutex> lk(mu);
  if (!q || !total || !n_rows) return PM_EINVAL;
  if (!q->status_mask || (q->status_mask >> PM_NS_N) || q->membership > PM_DIR_UNGROUPED || q->order > PM_DIR_BY_ADDRESS) return PM_EINVAL;
  if (!on) return PM_ESTATE;
  calls.push_back("mask=" + std::to_string(q->status_mask) + " mem=" + std::to_string(q->membership) + " order=" +
                  std::to_string(q->order) + " off=" + std::to_string(q->offset) + " lim=" + std::to_string(q->limit) + " cap=" +
                  std::to_string(cap));
  std::vector<uint32_t> list;
  uint32_t c[PM_NS_N] = {};
  for (uint32_t w = 0; w < rows.size(); ++w) {
    const pm_dir_row& r = rows[w];
    const bool grouped = r.group_slot != PM_NONE;
    if (!((q->status_mask >> r.status) & 1u)) continue;
    if (q->membership != PM_DIR_ANY && (q->membership == PM_DIR_GROUPED) != grouped) continue;
    list.push_back(w);
    ++c[r.status];
  }
  std::stable_sort(list.begin(), list.end(), [&](uint32_t a, uint32_t b) {
    const uint32_t ka = q->order == PM_DIR_BY_ADDRESS ? ranks[a] : a, kb = q->order == PM_DIR_BY_ADDRESS ? ranks[b] : b;
    return std::make_tuple(rows[a].cls, ka, a) < std::make_tuple(rows[b].cls, kb, b);
  });
  *total = uint32_t(list.size());
  if (counts) std::copy(c, c + PM_NS_N, counts);
  const uint32_t n = q->offset >= list.size() ? 0u : std::min(q->limit, uint32_t(list.size()) - q->offset);
  *n_rows = n;
  if (n && (!out || cap < n)) return PM_ERANGE;
  for (uint32_t k = 0; k < n; ++k) out[k] = rows[list[q->offset + k]];
  return PM_OK;
}

}  // extern "C"
