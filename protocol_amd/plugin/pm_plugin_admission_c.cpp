// pm_plugin_admission_c.cpp — see pm_plugin_c.h "request gate: admission": the C face of GpuMatchPlugin::enable_admission /
// admit_requests.  (A file of its own: pm_plugin_c.cpp is also linked against a mock engine that has not these exports.)
#include <sstream>
#include <string>

#include "pm_plugin_c.h"
#include "pm_plugin_c_internal.hpp"

using namespace orchestrator;

namespace {
template <typename F>
int32_t guarded(F&& f) {
  try {
    return f();
  } catch (const std::exception& e) {
    pmx_detail::set_error(e.what());
    return -1;
  }
}
const char* const CODE_NAMES[PM_AD_N_CODES] = {"bad_signature", "no_key", "bad_address", "mismatch", "unknown", "ejected", "banned", "ok",
                                               "rate_limited", "expired", "bad_nonce", "replay", "no_nonce"};
}  // namespace

extern "C" {

int32_t pmx_enable_admission(pmx_plugin* p) {
  return guarded([&] { return p->plugin->enable_admission(), 0; });
}

int32_t pmx_admit_requests(pmx_plugin* p, const char* requests, uint64_t now_ms, char* out, size_t cap, size_t* needed) {
  return guarded([&] {
    std::vector<GpuMatchPlugin::AdmitRequest> reqs;
    std::istringstream is(requests ? requests : "");
    for (std::string line; std::getline(is, line);) {
      size_t at[5], from = 0;
      for (size_t& t : at) {
        t = line.find('\t', from);
        if (t == std::string::npos) throw std::runtime_error("a request line is '<signature>\\t<address>\\t<timestamp>\\t<nonce>\\t<beat>\\t<message>'");
        from = t + 1;
      }
      GpuMatchPlugin::AdmitRequest r;
      r.signature = line.substr(0, at[0]);
      r.address = line.substr(at[0] + 1, at[1] - at[0] - 1);
      const std::string ts = line.substr(at[1] + 1, at[2] - at[1] - 1), nonce = line.substr(at[2] + 1, at[3] - at[2] - 1);
      if (ts != "-") r.timestamp = ts;
      if (nonce != "-") r.nonce = nonce;
      r.heartbeat = line.substr(at[3] + 1, at[4] - at[3] - 1) == "1";
      r.message = line.substr(at[4] + 1);
      reqs.push_back(std::move(r));
    }
    const GpuMatchPlugin::AdmitResult r = p->plugin->admit_requests(reqs, now_ms);
    static const char digits[] = "0123456789abcdef";
    std::string text;
    for (const GpuMatchPlugin::GateVerdict& v : r.verdicts) {
      text += CODE_NAMES[v.code < PM_AD_N_CODES ? v.code : 0];
      text += '\t' + (v.row == 0xFFFFFFFFu ? std::string("-") : std::to_string(v.row));
      text += '\t' + (v.status == 0xFF ? std::string("-") : std::to_string(unsigned(v.status))) + "\t0x";
      for (uint8_t byte : v.address) text += digits[byte >> 4], text += digits[byte & 15];
      text += '\n';
    }
    text += "counts";
    for (uint32_t c : r.counts) text += '\t' + std::to_string(c);
    text += '\n';
    return pmx_detail::give_text(text, out, cap, needed);
  });
}

}  // extern "C"
