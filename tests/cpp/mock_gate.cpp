// mock_gate.cpp — TEST INFRASTRUCTURE: the request gate's exports of include/pm_engine.h (pm_ecrecover_many, pm_verify_requests),
// which tests/cpp/mock_engine.cpp does not define, over the product's own host helpers (pm_host_keccak256, pm_host_ecrecover).
// The join reads tests/cpp/mock_addresses.cpp's book; the liveness bytes are the test's (mock_gate::status; empty: liveness is
// off).  Every call is logged with its request count and flags.
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "pm_engine.h"

namespace mock_addresses {
extern std::mutex mu;
extern bool on;
extern std::vector<uint8_t> bytes;
extern std::vector<uint8_t> set;
}  // namespace mock_addresses

namespace mock_gate {
std::mutex mu;
std::vector<uint8_t> status;     // PM_NS_* a row; empty: liveness is off
std::vector<std::string> calls;  // "verify n=.. flags=[..]", "ecrecover n=.."
}  // namespace mock_gate

static bool recovery_id(uint8_t v) { return v == 0 || v == 1 || v == 27 || v == 28; }

extern "C" {

int32_t pm_ecrecover_many(pm_engine*, const uint8_t* hash32, const uint8_t* sig65, uint32_t n, uint8_t* addr20_out, uint8_t* pub64_out,
                          uint8_t* ok_out) {
  if (n && (!hash32 || !sig65 || !addr20_out || !ok_out)) return PM_EINVAL;
  {
    std::lock_guard<std::mutex> lk(mock_gate::mu);
    mock_gate::calls.push_back("ecrecover n=" + std::to_string(n));
  }
  for (uint32_t i = 0; i < n; ++i) {
    ok_out[i] = pm_host_ecrecover(hash32 + 32 * size_t(i), sig65 + 65 * size_t(i), addr20_out + 20 * size_t(i)) == PM_OK;
    if (pub64_out) std::memset(pub64_out + 64 * size_t(i), 0, 64);  // (the host helper gives no key)
  }
  return PM_OK;
}

int32_t pm_verify_requests(pm_engine*, const uint8_t* bytes, const uint32_t* offsets, const uint8_t* sig65, const uint8_t* claimed20,
                           const uint8_t* flags, uint32_t n, pm_rq_verdict* out, uint32_t* counts) {
  std::lock_guard<std::mutex> book(mock_addresses::mu);
  std::lock_guard<std::mutex> lk(mock_gate::mu);
  if (!mock_addresses::on) return PM_ESTATE;
  if (n && (!offsets || !sig65 || !claimed20 || !out || !counts)) return PM_EINVAL;
  std::string listed = "[";
  for (uint32_t i = 0; i < n; ++i) listed += (i ? "," : "") + std::to_string(flags ? flags[i] : 0);
  mock_gate::calls.push_back("verify n=" + std::to_string(n) + " flags=" + listed + "]");
  if (!n) return PM_OK;
  std::memset(counts, 0, PM_RQ_N_CODES * sizeof(uint32_t));
  for (uint32_t i = 0; i < n; ++i) {
    if (offsets[i + 1] < offsets[i]) return PM_EINVAL;
    pm_rq_verdict v;
    std::memset(&v, 0, sizeof v);
    v.row = 0xFFFFFFFFu, v.status = 0xFF;
    const uint8_t* sig = sig65 + 65 * size_t(i);
    const uint32_t len = offsets[i + 1] - offsets[i];
    std::string text = "\x19" "Ethereum Signed Message:\n" + std::to_string(len);
    if (len) text.append(reinterpret_cast<const char*>(bytes + offsets[i]), len);
    uint8_t hash[32];
    pm_host_keccak256(reinterpret_cast<const uint8_t*>(text.data()), text.size(), hash);
    if (!recovery_id(sig[64])) {
      v.code = PM_RQ_BAD_SIGNATURE;
    } else if (pm_host_ecrecover(hash, sig, v.address) != PM_OK) {
      v.code = PM_RQ_NO_KEY;
    } else if (flags && (flags[i] & PM_RQ_FLAG_BAD_ADDRESS)) {
      v.code = PM_RQ_BAD_ADDRESS;
    } else {
      for (uint32_t w = 0; w < mock_addresses::set.size() && v.row == 0xFFFFFFFFu; ++w)
        if (mock_addresses::set[w] && std::memcmp(mock_addresses::bytes.data() + 20 * size_t(w), v.address, 20) == 0) v.row = w;
      if (v.row != 0xFFFFFFFFu && v.row < mock_gate::status.size()) v.status = mock_gate::status[v.row];
      if (std::memcmp(claimed20 + 20 * size_t(i), v.address, 20) != 0)
        v.code = PM_RQ_MISMATCH;
      else if (v.row == 0xFFFFFFFFu)
        v.code = PM_RQ_UNKNOWN;
      else if (v.status == PM_NS_EJECTED)
        v.code = PM_RQ_EJECTED;
      else if (v.status == PM_NS_BANNED)
        v.code = PM_RQ_BANNED;
      else
        v.code = PM_RQ_OK;
    }
    out[i] = v;
    counts[v.code]++;
  }
  return PM_OK;
}

}  // extern "C"
