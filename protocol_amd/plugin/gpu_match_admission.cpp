// gpu_match_admission.cpp — GpuMatchPlugin::enable_admission / admit_requests (see gpu_match_plugin.hpp): the engine's admission
// ledger (pm_admission_enable, pm_admit_requests, pm_liveness_sweep_beats).  The twin of the same methods of
// rust/gpu_match_plugin.rs — whose headers are parsed before the plugin sees them, so that it parses nothing: everything else is
// its transcription (INTEGRATION.md "Request gate: admission").  (A file of its own: the plugin's other methods are also linked
// against a mock engine that has not these exports.)
#include <shared_mutex>

#include "gpu_match_plugin.hpp"

namespace orchestrator {

void GpuMatchPlugin::enable_admission() {
  std::unique_lock<std::shared_mutex> nodes(nodes_mu_);  // (LOCK ORDER: nodes, the engine)
  if (!book_.on) throw EngineError(PM_ESTATE, "the address book is off (enable_address_book)");
  check(pm_admission_enable(engine_, 1u));
  sweep_call_ = pm_liveness_sweep_beats;
  admission_on_ = true;
}

// a u64 in decimal digits, as the query parameter's parse::<u64>() takes it
static bool parse_u64_text(const std::string& text, uint64_t* out) {
  if (text.empty() || text.size() > 20) return false;
  uint64_t v = 0;
  for (const char c : text) {
    if (c < '0' || c > '9') return false;
    const uint64_t d = uint64_t(c - '0');
    if (v > (UINT64_MAX - d) / 10) return false;
    v = v * 10 + d;
  }
  *out = v;
  return true;
}

GpuMatchPlugin::AdmitResult GpuMatchPlugin::admit_requests(const std::vector<AdmitRequest>& requests, uint64_t now_ms) const {
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);
  if (!book_.on) throw EngineError(PM_ESTATE, "the address book is off (enable_address_book)");
  if (!admission_on_) throw EngineError(PM_ESTATE, "admission is off (enable_admission)");
  const uint32_t n = uint32_t(requests.size());
  AdmitResult out;
  out.verdicts.resize(n);
  if (!n) return out;
  std::vector<uint8_t> bytes, nonces, sig(65 * size_t(n)), claimed(20 * size_t(n), 0), flags(n, 0);
  std::vector<uint32_t> offsets(size_t(n) + 1, 0), nonce_offsets(size_t(n) + 1, 0);
  std::vector<uint64_t> timestamps(n, 0);
  for (uint32_t k = 0; k < n; ++k) {
    const AdmitRequest& r = requests[k];
    bytes.insert(bytes.end(), r.message.begin(), r.message.end());
    if (bytes.size() > 0xFFFFFF00ull) throw EngineError(PM_ERANGE, "too many message bytes in one call");
    offsets[k + 1] = uint32_t(bytes.size());
    if (!parse_signature_text(r.signature, sig.data() + 65 * size_t(k))) std::fill_n(sig.begin() + 65 * size_t(k), 65, uint8_t(0xFF));
    if (!parse_address_text(r.address, claimed.data() + 20 * size_t(k))) {
      std::fill_n(claimed.begin() + 20 * size_t(k), 20, uint8_t(0));
      flags[k] = PM_RQ_FLAG_BAD_ADDRESS;
    }
    // (a timestamp that is no u64 is none: the middleware's as_u64 / parse::<u64>() give None, :344-358)
    if (!r.timestamp || !parse_u64_text(*r.timestamp, &timestamps[k])) flags[k] |= PM_RQ_FLAG_NO_TIMESTAMP;
    if (!r.nonce)
      flags[k] |= PM_RQ_FLAG_NO_NONCE;
    else
      nonces.insert(nonces.end(), r.nonce->begin(), r.nonce->end());
    if (nonces.size() > 0xFFFFFF00ull) throw EngineError(PM_ERANGE, "too many nonce bytes in one call");
    nonce_offsets[k + 1] = uint32_t(nonces.size());
    if (r.heartbeat) flags[k] |= PM_RQ_FLAG_BEAT;
  }
  nonces.push_back(0);  // (never read: a batch without a nonce still has an address)
  std::vector<pm_rq_verdict> v(n);
  check(pm_admit_requests(engine_, now_ms, bytes.data(), offsets.data(), sig.data(), claimed.data(), flags.data(), timestamps.data(),
                          nonces.data(), nonce_offsets.data(), n, v.data(), out.counts.data()));
  for (uint32_t k = 0; k < n; ++k) {
    GateVerdict& g = out.verdicts[k];
    g.code = v[k].code, g.row = v[k].row, g.status = v[k].status;
    std::copy(v[k].address, v[k].address + 20, g.address.begin());
  }
  return out;
}

}  // namespace orchestrator
