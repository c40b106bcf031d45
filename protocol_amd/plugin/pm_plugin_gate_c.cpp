// pm_plugin_gate_c.cpp — see pm_plugin_c.h "request gate": the C face of GpuMatchPlugin::verify_requests.  (A file of its own:
// pm_plugin_c.cpp is also linked against a mock engine that has not this export.)
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
const char* const CODE_NAMES[PM_RQ_N_CODES] = {"bad_signature", "no_key", "bad_address", "mismatch", "unknown", "ejected", "banned", "ok"};
}  // namespace

extern "C" {

int32_t pmx_verify_requests(pmx_plugin* p, const char* requests, char* out, size_t cap, size_t* needed) {
  return guarded([&] {
    std::vector<GpuMatchPlugin::GateRequest> reqs;
    std::istringstream is(requests ? requests : "");
    for (std::string line; std::getline(is, line);) {
      const size_t a = line.find('\t'), b = a == std::string::npos ? a : line.find('\t', a + 1);
      if (b == std::string::npos) throw std::runtime_error("a request line is '<signature>\\t<address>\\t<message>'");
      reqs.push_back({line.substr(b + 1), line.substr(0, a), line.substr(a + 1, b - a - 1)});
    }
    const GpuMatchPlugin::GateResult r = p->plugin->verify_requests(reqs);
    static const char digits[] = "0123456789abcdef";
    std::string text;
    for (const GpuMatchPlugin::GateVerdict& v : r.verdicts) {
      text += CODE_NAMES[v.code < PM_RQ_N_CODES ? v.code : 0];
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
