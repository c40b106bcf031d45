// mock_admission.cpp — TEST INFRASTRUCTURE: the admission exports of include/pm_engine.h (pm_admission_enable, pm_admit_requests,
// pm_admission_rate_get / _set, pm_admission_nonces, pm_beats_get / _set, pm_liveness_sweep_beats), which tests/cpp/mock_engine.cpp
// does not define.  The gate's stage is tests/cpp/mock_gate.cpp's pm_verify_requests, the sweep tests/cpp/mock_liveness.cpp's
// pm_liveness_sweep; behind them the middleware's rules one request at a time, over maps.  Every call is logged.
#include <algorithm>
#include <array>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "pm_engine.h"

namespace mock_addresses {
extern bool on;
}  // namespace mock_addresses

namespace mock_liveness {
extern std::atomic<uint32_t> W;
}  // namespace mock_liveness

namespace mock_admission {
std::mutex mu;
bool on = false;
uint32_t enables = 0;
std::map<uint32_t, std::pair<uint64_t, uint32_t>> rate;  // row -> (window_start_ms, count)
std::map<std::array<uint8_t, 32>, uint64_t> nonces;      // digest -> stored_ms
std::map<uint32_t, uint64_t> beats;                      // row -> last_beat_ms
std::vector<std::string> calls;  // "enable on=..", "admit now=.. n=.. flags=[..] ts=[..] nonces=[..]", "sweep_beats now=.. host=[..]"
std::vector<uint64_t> last_column;                       // what the last pm_liveness_sweep_beats swept over
}  // namespace mock_admission

static bool nonce_live(uint64_t now, uint64_t stored) { return now < stored || now - stored <= PM_RQ_NONCE_TTL_MS; }

extern "C" {

int32_t pm_admission_enable(pm_engine*, uint32_t on) {
  using namespace mock_admission;
  std::lock_guard<std::mutex> lk(mu);
  calls.push_back("enable on=" + std::to_string(on));
  if (on && !mock_addresses::on) return PM_ESTATE;
  ++enables;
  mock_admission::on = on != 0;
  rate.clear(), nonces.clear(), beats.clear();
  return PM_OK;
}

int32_t pm_admit_requests(pm_engine* e, uint64_t now_ms, const uint8_t* bytes, const uint32_t* offsets, const uint8_t* sig65,
                          const uint8_t* claimed20, const uint8_t* flags, const uint64_t* timestamp_s, const uint8_t* nonce_bytes,
                          const uint32_t* nonce_offsets, uint32_t n, pm_rq_verdict* out, uint32_t* counts) {
  using namespace mock_admission;
  std::lock_guard<std::mutex> lk(mu);
  if (!on) return PM_ESTATE;
  if (n && (!offsets || !sig65 || !claimed20 || !out || !counts)) return PM_EINVAL;
  std::string f = "[", t = "[", x = "[";
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t fl = flags ? flags[i] : 0u;
    if (!(fl & PM_RQ_FLAG_NO_TIMESTAMP) && !timestamp_s) return PM_EINVAL;
    if (!(fl & PM_RQ_FLAG_NO_NONCE) && (!nonce_offsets || (nonce_offsets[n] && !nonce_bytes))) return PM_EINVAL;
    if (nonce_offsets && nonce_offsets[i + 1] < nonce_offsets[i]) return PM_EINVAL;
    f += (i ? "," : "") + std::to_string(fl);
    t += (i ? "," : "") + ((fl & PM_RQ_FLAG_NO_TIMESTAMP) ? std::string("-") : std::to_string(timestamp_s[i]));
    x += (i ? "," : "") + ((fl & PM_RQ_FLAG_NO_NONCE) ? std::string("-")
                                                      : std::string(reinterpret_cast<const char*>(nonce_bytes) + nonce_offsets[i],
                                                                    nonce_offsets[i + 1] - nonce_offsets[i]));
  }
  calls.push_back("admit now=" + std::to_string(now_ms) + " n=" + std::to_string(n) + " flags=" + f + "] ts=" + t + "] nonces=" + x + "]");
  if (!n) return PM_OK;
  uint32_t gate_counts[PM_RQ_N_CODES];
  const int32_t rc = pm_verify_requests(e, bytes, offsets, sig65, claimed20, flags, n, out, gate_counts);
  if (rc != PM_OK) return rc;
  std::memset(counts, 0, PM_AD_N_CODES * sizeof(uint32_t));
  for (uint32_t i = 0; i < n; ++i) {
    pm_rq_verdict& v = out[i];
    const uint32_t fl = flags ? flags[i] : 0u;
    const uint32_t gate = v.code;
    if (gate == PM_RQ_BANNED || gate == PM_RQ_OK) {
      auto& [w, c] = rate[v.row];
      if ((w == 0 && c == 0) || (now_ms >= w && now_ms - w >= 60000u)) {
        w = now_ms, c = 1;
      } else if (c >= 100u) {
        v.code = PM_RQ_RATE_LIMITED;
      } else {
        ++c;
      }
      if (v.code == gate && !(fl & PM_RQ_FLAG_NO_TIMESTAMP) && now_ms / 1000u - timestamp_s[i] > 300u) v.code = PM_RQ_EXPIRED;
      if (v.code == gate && (fl & PM_RQ_FLAG_NO_NONCE)) v.code = PM_RQ_NO_NONCE;
      if (v.code == gate) {
        const uint8_t* s = nonce_bytes + nonce_offsets[i];
        const uint32_t len = nonce_offsets[i + 1] - nonce_offsets[i];
        bool good = len >= 16u && len <= 64u;
        for (uint32_t q = 0; good && q < len; ++q)
          good = (s[q] >= '0' && s[q] <= '9') || (s[q] >= 'A' && s[q] <= 'Z') || (s[q] >= 'a' && s[q] <= 'z') || s[q] == '-';
        if (!good) {
          v.code = PM_RQ_BAD_NONCE;
        } else {
          std::array<uint8_t, 32> d;
          pm_host_keccak256(s, len, d.data());
          const auto it = nonces.find(d);
          if (it != nonces.end() && nonce_live(now_ms, it->second))
            v.code = PM_RQ_REPLAY;
          else
            nonces[d] = now_ms;
        }
      }
      if (v.code == PM_RQ_OK && (fl & PM_RQ_FLAG_BEAT)) beats[v.row] = std::max(beats[v.row], now_ms);
    }
    counts[v.code]++;
  }
  for (auto it = nonces.begin(); it != nonces.end();) it = nonce_live(now_ms, it->second) ? std::next(it) : nonces.erase(it);
  return PM_OK;
}

int32_t pm_admission_rate_get(pm_engine*, const uint32_t* idx, uint32_t n, uint64_t* window_start_ms, uint32_t* count) {
  using namespace mock_admission;
  std::lock_guard<std::mutex> lk(mu);
  if (!on) return PM_ESTATE;
  for (uint32_t k = 0; k < n; ++k) {
    const auto it = rate.find(idx[k]);
    if (window_start_ms) window_start_ms[k] = it == rate.end() ? 0u : it->second.first;
    if (count) count[k] = it == rate.end() ? 0u : it->second.second;
  }
  return PM_OK;
}

int32_t pm_admission_rate_set(pm_engine*, const uint32_t* idx, const uint64_t* window_start_ms, const uint32_t* count, uint32_t n) {
  using namespace mock_admission;
  std::lock_guard<std::mutex> lk(mu);
  if (!on) return PM_ESTATE;
  for (uint32_t k = 0; k < n; ++k) rate[idx[k]] = {window_start_ms[k], count[k]};
  return PM_OK;
}

int32_t pm_admission_nonces(pm_engine*, uint64_t now_ms, uint32_t* n_live, uint32_t* n_held) {
  using namespace mock_admission;
  std::lock_guard<std::mutex> lk(mu);
  if (!on) return PM_ESTATE;
  uint32_t live = 0;
  for (const auto& kv : nonces) live += nonce_live(now_ms, kv.second);
  if (n_live) *n_live = live;
  if (n_held) *n_held = uint32_t(nonces.size());
  return PM_OK;
}

int32_t pm_beats_get(pm_engine*, const uint32_t* idx, uint32_t n, uint64_t* last_beat_ms) {
  using namespace mock_admission;
  std::lock_guard<std::mutex> lk(mu);
  if (!on) return PM_ESTATE;
  for (uint32_t k = 0; k < n; ++k) {
    const auto it = beats.find(idx[k]);
    last_beat_ms[k] = it == beats.end() ? 0u : it->second;
  }
  return PM_OK;
}

int32_t pm_beats_set(pm_engine*, const uint32_t* idx, const uint64_t* last_beat_ms, uint32_t n) {
  using namespace mock_admission;
  std::lock_guard<std::mutex> lk(mu);
  if (!on) return PM_ESTATE;
  for (uint32_t k = 0; k < n; ++k) beats[idx[k]] = last_beat_ms[k];
  return PM_OK;
}

int32_t pm_liveness_sweep_beats(pm_engine* e, uint64_t now_ms, const uint64_t* last_beat_ms, const uint64_t* in_pool_bits, uint32_t apply,
                                uint32_t* n_transitions, uint32_t* census) {
  using namespace mock_admission;
  std::vector<uint64_t> column;
  {
    std::lock_guard<std::mutex> lk(mu);
    if (!on) return PM_ESTATE;
    const uint32_t W = mock_liveness::W.load();
    column.assign(W, 0);
    std::string host = last_beat_ms ? "[" : "null";
    for (uint32_t w = 0; w < W; ++w) {
      const auto it = beats.find(w);
      column[w] = std::max(it == beats.end() ? uint64_t(0) : it->second, last_beat_ms ? last_beat_ms[w] : uint64_t(0));
      if (last_beat_ms) host += (w ? "," : "") + std::to_string(last_beat_ms[w]);
    }
    calls.push_back("sweep_beats now=" + std::to_string(now_ms) + " host=" + host + (last_beat_ms ? "]" : ""));
    last_column = column;
  }
  column.push_back(0);  // (an empty table still has an address)
  return pm_liveness_sweep(e, now_ms, column.data(), in_pool_bits, apply, n_transitions, census);
}

}  // extern "C"
