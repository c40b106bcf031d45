// gpu_match_gate.cpp — GpuMatchPlugin::verify_requests / parse_signature_text (see gpu_match_plugin.hpp): the engine's request
// gate (pm_verify_requests).  The twin of the same method of rust/gpu_match_plugin.rs — whose Signature and Address are parsed
// by alloy before the plugin sees them, so that it parses nothing and sets no flag: everything else is its transcription
// (INTEGRATION.md "Request gate").  (A file of its own: the plugin's other methods are also linked against a mock engine that
// has not this export.)
#include <shared_mutex>

#include "gpu_match_plugin.hpp"

namespace orchestrator {

bool GpuMatchPlugin::parse_signature_text(const std::string& text, uint8_t out65[65]) {
  const size_t from = text.compare(0, 2, "0x") == 0 ? 2 : 0;
  if (text.size() - from != 130) return false;
  const auto nibble = [](char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; };
  for (size_t i = 0; i < 65; ++i) {
    const int hi = nibble(text[from + 2 * i]), lo = nibble(text[from + 2 * i + 1]);
    if (hi < 0 || lo < 0) return false;
    out65[i] = uint8_t(hi << 4 | lo);
  }
  return true;
}

GpuMatchPlugin::GateResult GpuMatchPlugin::verify_requests(const std::vector<GateRequest>& requests) const {
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);
  if (!book_.on) throw EngineError(PM_ESTATE, "the address book is off (enable_address_book)");
  const uint32_t n = uint32_t(requests.size());
  GateResult out;
  out.verdicts.resize(n);
  if (!n) return out;
  std::vector<uint8_t> bytes, sig(65 * size_t(n)), claimed(20 * size_t(n), 0), flags(n, 0);
  std::vector<uint32_t> offsets(size_t(n) + 1, 0);
  for (uint32_t k = 0; k < n; ++k) {
    const GateRequest& r = requests[k];
    bytes.insert(bytes.end(), r.message.begin(), r.message.end());
    if (bytes.size() > 0xFFFFFF00ull) throw EngineError(PM_ERANGE, "too many message bytes in one call");
    offsets[k + 1] = uint32_t(bytes.size());
    // (no signature: every byte 0xFF, whose v is no recovery id — the engine answers PM_RQ_BAD_SIGNATURE and counts it)
    if (!parse_signature_text(r.signature, sig.data() + 65 * size_t(k))) std::fill_n(sig.begin() + 65 * size_t(k), 65, uint8_t(0xFF));
    if (!parse_address_text(r.address, claimed.data() + 20 * size_t(k))) {
      std::fill_n(claimed.begin() + 20 * size_t(k), 20, uint8_t(0));
      flags[k] = PM_RQ_FLAG_BAD_ADDRESS;
    }
  }
  std::vector<pm_rq_verdict> v(n);
  check(pm_verify_requests(engine_, bytes.data(), offsets.data(), sig.data(), claimed.data(), flags.data(), n, v.data(), out.counts.data()));
  for (uint32_t k = 0; k < n; ++k) {
    GateVerdict& g = out.verdicts[k];
    g.code = v[k].code, g.row = v[k].row, g.status = v[k].status;
    std::copy(v[k].address, v[k].address + 20, g.address.begin());
  }
  return out;
}

}  // namespace orchestrator
