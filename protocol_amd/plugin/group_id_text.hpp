// group_id_text.hpp — a group id as the reference writes it: format!("{:x}", u64) (generate_group_id, node_groups/mod.rs:1489-1493),
// and back.  Shared by gpu_match_plugin.cpp and gpu_match_restore.cpp.
#ifndef PM_GROUP_ID_TEXT_HPP
#define PM_GROUP_ID_TEXT_HPP

#include <cstdint>
#include <cstdio>
#include <string>

namespace orchestrator {

inline std::string hex_lower(uint64_t v) {  // format!("{:x}", v)
  char buf[24];
  std::snprintf(buf, sizeof(buf), "%llx", (unsigned long long)v);
  return buf;
}

// the inverse of format!("{:x}", u64): lower-case hex digits, no sign, no prefix, no leading zero (but "0"), <= 16 of them.
// Anything else is the text of no group id (a Redis key that does not exist in the reference).
inline bool parse_group_id(const std::string& s, uint64_t* out) {
  if (s.empty() || s.size() > 16 || (s.size() > 1 && s[0] == '0')) return false;
  uint64_t v = 0;
  for (char c : s) {
    uint64_t d;
    if (c >= '0' && c <= '9') d = uint64_t(c - '0');
    else if (c >= 'a' && c <= 'f') d = uint64_t(c - 'a' + 10);
    else return false;
    v = (v << 4) | d;
  }
  *out = v;
  return true;
}

}  // namespace orchestrator
#endif
