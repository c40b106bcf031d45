// pm_plugin_addresses_c.cpp — see pm_plugin_c.h "address book": the C face of GpuMatchPlugin::enable_address_book /
// invite_digests.  (A file of its own: pm_plugin_c.cpp is also linked against a mock engine that has not these exports.)
#include <array>
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
std::string hex(const std::array<uint8_t, 32>& b) {
  static const char digits[] = "0123456789abcdef";
  std::string out;
  for (uint8_t v : b) out += digits[v >> 4], out += digits[v & 15];
  return out;
}
}  // namespace

extern "C" {

int32_t pmx_enable_address_book(pmx_plugin* p) {
  return guarded([&] { return p->plugin->enable_address_book(), 0; });
}

int32_t pmx_invite_digests(pmx_plugin* p, uint32_t domain_id, uint32_t pool_id, uint64_t nonce_seed, uint64_t expiration_s, char* out,
                           size_t cap, size_t* needed) {
  return guarded([&] {
    uint64_t state = nonce_seed;
    const auto nonce = [&] {  // splitmix64, four words a nonce, little-endian
      std::array<uint8_t, 32> n{};
      for (int w = 0; w < 4; ++w) {
        uint64_t z = (state += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        for (int j = 0; j < 8; ++j) n[8 * w + j] = uint8_t(z >> (8 * j));
      }
      return n;
    };
    std::string text;
    for (const GpuMatchPlugin::InviteDigest& d : p->plugin->invite_digests(domain_id, pool_id, nonce, expiration_s))
      text += d.address + "\t" + hex(d.nonce) + "\t" + hex(d.digest) + "\t" + hex(d.signing_hash) + "\n";
    return pmx_detail::give_text(text, out, cap, needed);
  });
}

}  // extern "C"
