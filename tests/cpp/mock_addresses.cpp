// mock_addresses.cpp — TEST INFRASTRUCTURE: the address book's exports of include/pm_engine.h (pm_addresses_enable / _set / _rank /
// _text, pm_invite_digests), which tests/cpp/mock_engine.cpp does not define.  One book for the process (a test runs one plugin
// with the book on at a time); the texts and digests are the product's own host helpers (pm_host_eip55, pm_host_keccak256), the
// rank is a sort of those texts with the row as tie-break, installed through the mock engine's pm_set_addr_ranks — which also
// holds the column's length to the engine's row count.  Every call is logged.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "pm_engine.h"

namespace mock_addresses {
std::mutex mu;
bool on = false;
std::vector<uint8_t> bytes;      // 20 a row
std::vector<uint8_t> set;        // a row holds an address
std::vector<std::string> calls;  // "enable 1", "set first=.. n=..", "rank", "text rows=[..]", "invite n=.."
}  // namespace mock_addresses

static std::string text_of(uint32_t row) {
  char t[43];
  pm_host_eip55(mock_addresses::bytes.data() + 20 * size_t(row), t);
  return t;
}

extern "C" {

int32_t pm_addresses_enable(pm_engine*, uint32_t enable) {
  using namespace mock_addresses;
  std::lock_guard<std::mutex> lk(mu);
  on = enable != 0;
  bytes.clear();
  set.clear();
  calls.push_back("enable " + std::to_string(enable));
  return PM_OK;
}

int32_t pm_addresses_set(pm_engine*, uint32_t first_row, const uint8_t* addr20, uint32_t n) {
  using namespace mock_addresses;
  std::lock_guard<std::mutex> lk(mu);
  if (!on) return PM_ESTATE;
  if (n && !addr20) return PM_EINVAL;
  calls.push_back("set first=" + std::to_string(first_row) + " n=" + std::to_string(n));
  if (set.size() < size_t(first_row) + n) set.resize(size_t(first_row) + n, 0), bytes.resize(20 * (size_t(first_row) + n), 0);
  std::memcpy(bytes.data() + 20 * size_t(first_row), addr20, 20 * size_t(n));
  std::fill(set.begin() + first_row, set.begin() + first_row + n, uint8_t(1));
  return PM_OK;
}

int32_t pm_addresses_rank(pm_engine* e, uint32_t* rank_out) {
  using namespace mock_addresses;
  std::lock_guard<std::mutex> lk(mu);
  if (!on) return PM_ESTATE;
  calls.push_back("rank");
  const uint32_t W = uint32_t(set.size());
  if (std::find(set.begin(), set.end(), uint8_t(0)) != set.end()) return PM_ESTATE;
  std::vector<std::string> texts(W);
  for (uint32_t w = 0; w < W; ++w) texts[w] = text_of(w);
  std::vector<uint32_t> order(W), rank(W);
  for (uint32_t w = 0; w < W; ++w) order[w] = w;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return texts[a] < texts[b]; });
  for (uint32_t i = 0; i < W; ++i) rank[order[i]] = i;
  if (W) {
    const int32_t rc = pm_set_addr_ranks(e, rank.data(), W);  // (PM_EINVAL unless the engine has exactly W rows)
    if (rc) return PM_ESTATE;
  }
  if (rank_out) std::copy(rank.begin(), rank.end(), rank_out);
  return PM_OK;
}

int32_t pm_addresses_text(pm_engine*, const uint32_t* rows, uint32_t n, char* out) {
  using namespace mock_addresses;
  std::lock_guard<std::mutex> lk(mu);
  if (!on) return PM_ESTATE;
  std::string listed = "[";
  for (uint32_t k = 0; k < n; ++k) listed += (k ? "," : "") + std::to_string(rows ? rows[k] : k);
  calls.push_back("text rows=" + listed + "]");
  for (uint32_t k = 0; k < n; ++k) {
    const uint32_t w = rows ? rows[k] : k;
    if (w >= set.size()) return PM_ERANGE;
    if (!set[w]) return PM_ESTATE;
    std::memcpy(out + 43 * size_t(k), text_of(w).c_str(), 43);
  }
  return PM_OK;
}

int32_t pm_invite_digests(pm_engine*, uint32_t domain_id, uint32_t pool_id, const uint32_t* rows, uint32_t n, const uint8_t* nonce,
                          const uint64_t* expiration_s, uint8_t* digest, uint8_t* signing_hash) {
  using namespace mock_addresses;
  std::lock_guard<std::mutex> lk(mu);
  if (!on) return PM_ESTATE;
  calls.push_back("invite n=" + std::to_string(n));
  for (uint32_t k = 0; k < n; ++k) {
    if (rows[k] >= set.size()) return PM_ERANGE;
    if (!set[rows[k]]) return PM_ESTATE;
    uint8_t msg[148] = {}, signed_msg[60];
    for (int j = 0; j < 4; ++j) msg[28 + j] = uint8_t(domain_id >> (8 * (3 - j))), msg[60 + j] = uint8_t(pool_id >> (8 * (3 - j)));
    std::memcpy(msg + 64, bytes.data() + 20 * size_t(rows[k]), 20);
    std::memcpy(msg + 84, nonce + 32 * size_t(k), 32);
    for (int j = 0; j < 8; ++j) msg[140 + j] = uint8_t(expiration_s[k] >> (8 * (7 - j)));
    pm_host_keccak256(msg, sizeof(msg), digest + 32 * size_t(k));
    std::memcpy(signed_msg, "\x19" "Ethereum Signed Message:\n32", 28);
    std::memcpy(signed_msg + 28, digest + 32 * size_t(k), 32);
    pm_host_keccak256(signed_msg, sizeof(signed_msg), signing_hash + 32 * size_t(k));
  }
  return PM_OK;
}

}  // extern "C"
