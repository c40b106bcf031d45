// pm_host.cpp — host-side mirror of the reference's configuration front end (no GPU needed):
//   ComputeRequirements::from_str      crates/shared/src/models/node.rs:180-374
//   GpuSpecs::meets model-string rule  crates/shared/src/models/node.rs:463-484
//   config priority order              crates/orchestrator/src/plugins/node_groups/mod.rs:150-164, :399-418
// This is product code: it shares nothing with oracle/, which restates the same rules separately so
// the two can be checked against each other and against the reference's known-answer tests.
#include <algorithm>
#include <cstring>
#include <string>
#include <string_view>
#include <vector>

#include "pm_engine.h"
#include "pm_internal.h"

namespace pm {

namespace {

#include "pm_unicode_lower.inc"  // GENERATED (tools/make_unicode_tables.py): pm_uc_lower_map, pm_uc_cased_ranges, pm_uc_case_ignorable_ranges

// One code point of a UTF-8 string (Rust strings are valid UTF-8; a byte that is not the start of a well-formed sequence is
// passed through as itself: *len = 1, value = 0x110000 + byte, which no table knows).
uint32_t decode_utf8(std::string_view s, size_t i, size_t* len) {
  const auto b = [&](size_t k) { return uint32_t(static_cast<unsigned char>(s[k])); };
  const uint32_t c = b(i);
  *len = 1;
  if (c < 0x80u) return c;
  const auto cont = [&](size_t k) { return k < s.size() && (b(k) & 0xC0u) == 0x80u; };
  if (c >= 0xC2u && c <= 0xDFu && cont(i + 1)) {
    *len = 2;
    return ((c & 0x1Fu) << 6) | (b(i + 1) & 0x3Fu);
  }
  if (c >= 0xE0u && c <= 0xEFu && cont(i + 1) && cont(i + 2)) {
    const uint32_t v = ((c & 0x0Fu) << 12) | ((b(i + 1) & 0x3Fu) << 6) | (b(i + 2) & 0x3Fu);
    if (v >= 0x800u && !(v >= 0xD800u && v <= 0xDFFFu)) {
      *len = 3;
      return v;
    }
  }
  if (c >= 0xF0u && c <= 0xF4u && cont(i + 1) && cont(i + 2) && cont(i + 3)) {
    const uint32_t v = ((c & 0x07u) << 18) | ((b(i + 1) & 0x3Fu) << 12) | ((b(i + 2) & 0x3Fu) << 6) | (b(i + 3) & 0x3Fu);
    if (v >= 0x10000u && v <= 0x10FFFFu) {
      *len = 4;
      return v;
    }
  }
  return 0x110000u + c;
}
void encode_utf8(uint32_t v, std::string* o) {
  if (v < 0x80u) o->push_back(char(v));
  else if (v < 0x800u) { o->push_back(char(0xC0u | (v >> 6))); o->push_back(char(0x80u | (v & 0x3Fu))); }
  else if (v < 0x10000u) { o->push_back(char(0xE0u | (v >> 12))); o->push_back(char(0x80u | ((v >> 6) & 0x3Fu))); o->push_back(char(0x80u | (v & 0x3Fu))); }
  else { o->push_back(char(0xF0u | (v >> 18))); o->push_back(char(0x80u | ((v >> 12) & 0x3Fu))); o->push_back(char(0x80u | ((v >> 6) & 0x3Fu))); o->push_back(char(0x80u | (v & 0x3Fu))); }
}

// char::is_whitespace (the White_Space property): what str::trim strips
bool is_whitespace(uint32_t c) {
  return (c >= 0x09u && c <= 0x0Du) || c == 0x20u || c == 0x85u || c == 0xA0u || c == 0x1680u || (c >= 0x2000u && c <= 0x200Au) ||
         c == 0x2028u || c == 0x2029u || c == 0x202Fu || c == 0x205Fu || c == 0x3000u;
}

template <size_t N>
bool in_ranges(const uint32_t (&r)[N][2], uint32_t c) {
  size_t lo = 0, hi = N;
  while (lo < hi) {
    const size_t mid = (lo + hi) / 2;
    if (c > r[mid][1]) lo = mid + 1;
    else hi = mid;
  }
  return lo < N && c >= r[lo][0];
}

std::string_view trim(std::string_view s) {  // str::trim
  size_t b = 0, e = s.size();
  while (b < e) {
    size_t n;
    if (!is_whitespace(decode_utf8(s, b, &n))) break;
    b += n;
  }
  while (e > b) {  // (the last code point: step back over continuation bytes)
    size_t k = e - 1;
    while (k > b && (static_cast<unsigned char>(s[k]) & 0xC0u) == 0x80u && e - k < 4) --k;
    size_t n;
    const uint32_t c = decode_utf8(s, k, &n);
    if (k + n != e || !is_whitespace(c)) break;
    e = k;
  }
  return s.substr(b, e - b);
}

// alloc::str: case_ignorable_then_cased over the code points of s[from..to) (forwards) or backwards from `from`
bool cased_after_ignorables_fwd(std::string_view s, size_t i) {
  while (i < s.size()) {
    size_t n;
    const uint32_t c = decode_utf8(s, i, &n);
    if (!in_ranges(pm_uc_case_ignorable_ranges, c)) return in_ranges(pm_uc_cased_ranges, c);
    i += n;
  }
  return false;
}
bool cased_after_ignorables_back(std::string_view s, size_t i) {
  while (i > 0) {
    size_t k = i - 1;
    while (k > 0 && (static_cast<unsigned char>(s[k]) & 0xC0u) == 0x80u && i - k < 4) --k;
    size_t n;
    uint32_t c = decode_utf8(s, k, &n);
    if (k + n != i) {  // (a stray continuation byte: a code point of its own)
      k = i - 1;
      c = decode_utf8(s, k, &n);
    }
    if (!in_ranges(pm_uc_case_ignorable_ranges, c)) return in_ranges(pm_uc_cased_ranges, c);
    i = k;
  }
  return false;
}

}  // namespace

// str::to_lowercase (node.rs:465, :470): every code point through char::to_lowercase — which may give up to three — and
// a capital sigma at the end of a word as the final form (alloc::str::to_lowercase, map_uppercase_sigma)
std::string to_lowercase(std::string_view s) {
  std::string o;
  o.reserve(s.size());
  for (size_t i = 0; i < s.size();) {
    size_t n;
    const uint32_t c = decode_utf8(s, i, &n);
    if (c < 0x80u) {
      o.push_back(c >= 'A' && c <= 'Z' ? char(c - 'A' + 'a') : char(c));
    } else if (c == 0x3A3u) {
      const bool word_final = cased_after_ignorables_back(s, i) && !cased_after_ignorables_fwd(s, i + n);
      encode_utf8(word_final ? 0x3C2u : 0x3C3u, &o);
    } else {
      constexpr size_t N = sizeof(pm_uc_lower_map) / sizeof(pm_uc_lower_map[0]);
      size_t lo = 0, hi = N;
      while (lo < hi) {
        const size_t mid = (lo + hi) / 2;
        if (pm_uc_lower_map[mid].cp < c) lo = mid + 1;
        else hi = mid;
      }
      if (lo < N && pm_uc_lower_map[lo].cp == c)
        for (uint32_t k = 0; k < pm_uc_lower_map[lo].n; ++k) encode_utf8(pm_uc_lower_map[lo].out[k], &o);
      else
        o.append(s.substr(i, n));
    }
    i += n;
  }
  return o;
}

namespace {

// <u32 as FromStr>: optional '+', at least one ASCII digit, no overflow.
bool parse_u32(std::string_view s, uint32_t* out) {
  if (!s.empty() && s.front() == '+') s.remove_prefix(1);
  if (s.empty()) return false;
  uint64_t v = 0;
  for (char c : s) {
    if (c < '0' || c > '9') return false;
    v = v * 10 + uint64_t(c - '0');
    if (v > 0xFFFFFFFFull) return false;
  }
  *out = uint32_t(v);
  return true;
}

std::string normalize_model(std::string_view s) {  // to_lowercase().replace(' ', "_")
  std::string o = to_lowercase(s);
  for (char& c : o)
    if (c == ' ') c = '_';
  return o;
}
std::string drop_underscores(const std::string& s) {
  std::string o;
  o.reserve(s.size());
  for (char c : s)
    if (c != '_') o.push_back(c);
  return o;
}
bool contains(const std::string& hay, const std::string& needle) { return hay.find(needle) != std::string::npos; }

}  // namespace

bool model_matches(std::string_view spec_model, std::string_view req_model) {
  const std::string ns = normalize_model(spec_model);  // node.rs:465
  const std::string ns_nu = drop_underscores(ns);      // :473
  size_t pos = 0;
  for (;;) {  // req_model.split(',') — an empty string still yields one (empty) part
    const size_t comma = req_model.find(',', pos);
    const std::string_view part =
        req_model.substr(pos, comma == std::string_view::npos ? std::string_view::npos : comma - pos);
    const std::string nr = normalize_model(trim(part));  // :468-470
    const std::string nr_nu = drop_underscores(nr);      // :474
    if (contains(ns, nr) || contains(nr, ns) || contains(ns_nu, nr_nu) || contains(nr_nu, ns_nu)) return true;
    if (comma == std::string_view::npos) break;
    pos = comma + 1;
  }
  return false;
}

// Parsed requirement with owned model strings.
int32_t parse_requirements(std::string_view s, ParsedRequirements* out) {
  out->flags = 0;
  out->cpu_cores = out->ram_mb = out->storage_gb = 0;
  out->alts.clear();
  out->models.clear();
  pm_gpu_alt_row cur{};
  std::string cur_model;
  bool started = false;  // gpu_spec_started, node.rs:185
  auto push_cur = [&]() {
    out->alts.push_back(cur);
    out->models.push_back(cur_model);
    cur = pm_gpu_alt_row{};
    cur_model.clear();
  };
  size_t pos = 0;
  for (;;) {
    const size_t semi = s.find(';', pos);
    std::string_view part = trim(s.substr(pos, semi == std::string_view::npos ? std::string_view::npos : semi - pos));
    if (!part.empty()) {
      const size_t eq = part.find('=');  // splitn(2, '=')
      if (eq == std::string_view::npos) return set_error(PM_EPARSE, "Invalid key-value pair format");
      const std::string_view key = trim(part.substr(0, eq));
      const std::string_view value = trim(part.substr(eq + 1));
      uint32_t v = 0;
      const bool num = parse_u32(value, &v);
      if (key == "gpu:count") {  // :203-216
        if (started && (cur.flags & PM_G_COUNT)) push_cur();
        started = true;
        if (!num) return set_error(PM_EPARSE, "Invalid gpu:count value");
        cur.flags |= PM_G_COUNT;
        cur.count = v;
      } else if (key == "gpu:model") {  // :217-222
        started = true;
        cur.flags |= PM_G_MODEL;
        cur_model.assign(value);
      } else if (key == "gpu:memory_mb") {  // :223-238
        started = true;
        if (cur.flags & (PM_G_MEM_MIN | PM_G_MEM_MAX))
          return set_error(PM_EPARSE, "Cannot specify both exact memory and min/max memory");
        if (!num) return set_error(PM_EPARSE, "Invalid gpu:memory_mb value");
        cur.flags |= PM_G_MEM;
        cur.memory_mb = v;
      } else if (key == "gpu:memory_mb_min") {  // :239-262
        started = true;
        if (cur.flags & PM_G_MEM) return set_error(PM_EPARSE, "Cannot specify both exact memory and min/max memory");
        if (cur.flags & PM_G_MEM_MAX) {
          if (!num) return set_error(PM_EPANIC, "reference panics: unwrap on non-numeric gpu:memory_mb_min");
          if (cur.memory_mb_max < v) return set_error(PM_EPARSE, "min value is greater than max value");
        }
        if (!num) return set_error(PM_EPARSE, "Invalid gpu:memory_mb_min value");
        cur.flags |= PM_G_MEM_MIN;
        cur.memory_mb_min = v;
      } else if (key == "gpu:memory_mb_max") {  // :263-288
        started = true;
        if (cur.flags & PM_G_MEM) return set_error(PM_EPARSE, "Cannot specify both exact memory and min/max memory");
        if (cur.flags & PM_G_MEM_MIN) {
          if (!num) return set_error(PM_EPANIC, "reference panics: unwrap on non-numeric gpu:memory_mb_max");
          if (cur.memory_mb_min > v) return set_error(PM_EPARSE, "max value is less than min value");
        }
        if (!num) return set_error(PM_EPARSE, "Invalid gpu:memory_mb_max value");
        cur.flags |= PM_G_MEM_MAX;
        cur.memory_mb_max = v;
      } else if (key == "gpu:total_memory_min") {  // :290-310
        started = true;
        if (cur.flags & PM_G_TOT_MAX) {
          if (!num) return set_error(PM_EPANIC, "reference panics: unwrap on non-numeric gpu:total_memory_min");
          if (cur.total_memory_max < v) return set_error(PM_EPARSE, "min value is greater than max value");
        }
        if (!num) return set_error(PM_EPARSE, "Invalid gpu:total_memory_min value");
        cur.flags |= PM_G_TOT_MIN;
        cur.total_memory_min = v;
      } else if (key == "gpu:total_memory_max") {  // :311-331
        started = true;
        if (cur.flags & PM_G_TOT_MIN) {
          if (!num) return set_error(PM_EPANIC, "reference panics: unwrap on non-numeric gpu:total_memory_max");
          if (cur.total_memory_min > v) return set_error(PM_EPARSE, "max value is less than min value");
        }
        if (!num) return set_error(PM_EPARSE, "Invalid gpu:total_memory_max value");
        cur.flags |= PM_G_TOT_MAX;
        cur.total_memory_max = v;
      } else if (key == "cpu:cores") {  // :333-341
        if (!num) return set_error(PM_EPARSE, "Invalid cpu:cores value");
        out->flags |= PM_R_CPU | PM_R_CPU_CORES;
        out->cpu_cores = v;
      } else if (key == "ram_mb") {  // :344-350
        if (!num) return set_error(PM_EPARSE, "Invalid ram_mb value");
        out->flags |= PM_R_RAM;
        out->ram_mb = v;
      } else if (key == "storage_gb") {  // :351-357
        if (!num) return set_error(PM_EPARSE, "Invalid storage_gb value");
        out->flags |= PM_R_STORAGE;
        out->storage_gb = v;
      } else {
        return set_error(PM_EPARSE, "Unknown requirement key");  // :358
      }
    }
    if (semi == std::string_view::npos) break;
    pos = semi + 1;
  }
  if (started && cur.flags != 0) push_cur();  // :360-370
  return PM_OK;
}

// Constructor sort (mod.rs:150-164): min_group_size desc, then with-requirements first; stable.
void template_order(const pm_config_row* cfgs, uint32_t n, std::vector<uint32_t>* order) {
  order->resize(n);
  for (uint32_t i = 0; i < n; ++i) (*order)[i] = i;
  std::stable_sort(order->begin(), order->end(), [&](uint32_t a, uint32_t b) {
    if (cfgs[a].min_group_size != cfgs[b].min_group_size) return cfgs[a].min_group_size > cfgs[b].min_group_size;
    return (cfgs[a].flags & PM_R_HAS_REQ) && !(cfgs[b].flags & PM_R_HAS_REQ);
  });
}

// get_available_configurations (mod.rs:399-418): enabled filter, then stable min_group_size desc.
void available_order(const pm_config_row* cfgs, uint32_t n, uint64_t enabled, std::vector<uint32_t>* out) {
  std::vector<uint32_t> tmpl;
  template_order(cfgs, n, &tmpl);
  out->clear();
  for (uint32_t c : tmpl)
    if ((enabled >> c) & 1ull) out->push_back(c);
  std::stable_sort(out->begin(), out->end(),
                   [&](uint32_t a, uint32_t b) { return cfgs[a].min_group_size > cfgs[b].min_group_size; });
}

}  // namespace pm

extern "C" {

int32_t pm_host_parse_requirements(const char* s, pm_config_row* cfg, pm_gpu_alt_row* alts, uint32_t alt_cap,
                                   char* models_out, size_t models_cap) {
  if (!s || !cfg) return pm::set_error(PM_EINVAL, "null argument");
  pm::ParsedRequirements pr;
  const int32_t rc = pm::parse_requirements(s, &pr);
  if (rc != PM_OK) return rc;
  if (pr.alts.size() > alt_cap) return pm::set_error(PM_ERANGE, "too many GPU alternatives for the caller buffer");
  cfg->flags = (cfg->flags & ~uint32_t(PM_R_CPU | PM_R_CPU_CORES | PM_R_RAM | PM_R_STORAGE)) | pr.flags | PM_R_HAS_REQ;
  cfg->cpu_cores = pr.cpu_cores;
  cfg->ram_mb = pr.ram_mb;
  cfg->storage_gb = pr.storage_gb;
  cfg->alt_count = uint32_t(pr.alts.size());
  size_t off = 0;
  for (size_t i = 0; i < pr.alts.size(); ++i) {
    pm_gpu_alt_row a = pr.alts[i];
    a.model_row = 0;
    if (a.flags & PM_G_MODEL) {
      const std::string& m = pr.models[i];
      if (!models_out || off + m.size() + 1 > models_cap)
        return pm::set_error(PM_ERANGE, "model string buffer too small");
      std::memcpy(models_out + off, m.c_str(), m.size() + 1);
      a.model_row = uint32_t(off);
      off += m.size() + 1;
    }
    if (alts) alts[i] = a;
  }
  return PM_OK;
}

int32_t pm_host_model_matches(const char* spec_model, const char* req_model) {
  if (!spec_model || !req_model) return pm::set_error(PM_EINVAL, "null argument");
  return pm::model_matches(spec_model, req_model) ? 1 : 0;
}

int32_t pm_host_to_lowercase(const char* in, char* out, size_t cap, size_t* needed) {
  if (!in || !needed) return pm::set_error(PM_EINVAL, "null argument");
  const std::string r = pm::to_lowercase(in);
  *needed = r.size() + 1;
  if (!out && cap == 0) return PM_OK;  // sizing call
  if (!out || cap < r.size() + 1) return pm::set_error(PM_ERANGE, "output buffer too small");
  std::memcpy(out, r.c_str(), r.size() + 1);
  return PM_OK;
}

int32_t pm_host_build_model_table(const char* const* req_models, uint32_t n_rows, const char* const* spec_models,
                                  uint32_t n_classes, uint32_t* bits_out) {
  if ((n_rows && !req_models) || (n_classes && !spec_models) || !bits_out)
    return pm::set_error(PM_EINVAL, "null argument");
  const uint32_t words = (n_classes + 31u) / 32u;
  std::memset(bits_out, 0, sizeof(uint32_t) * size_t(n_rows) * words);
  for (uint32_t r = 0; r < n_rows; ++r)
    for (uint32_t c = 0; c < n_classes; ++c)
      if (pm::model_matches(spec_models[c], req_models[r])) bits_out[size_t(r) * words + (c >> 5)] |= 1u << (c & 31u);
  return PM_OK;
}

int32_t pm_host_config_order(const pm_config_row* cfgs, uint32_t n_cfgs, uint64_t enabled, uint32_t* order_out,
                             uint32_t* n_out) {
  if ((n_cfgs && !cfgs) || !order_out || !n_out) return pm::set_error(PM_EINVAL, "null argument");
  if (n_cfgs > PM_MAX_CONFIGS) return pm::set_error(PM_EINVAL, "more than PM_MAX_CONFIGS configurations");
  for (uint32_t i = 0; i < n_cfgs; ++i)
    if (cfgs[i].max_group_size < cfgs[i].min_group_size)
      return pm::set_error(PM_EINVAL, "Plugin configuration is invalid (max_group_size < min_group_size)");
  std::vector<uint32_t> o;
  pm::available_order(cfgs, n_cfgs, enabled, &o);
  for (size_t i = 0; i < o.size(); ++i) order_out[i] = o[i];
  *n_out = uint32_t(o.size());
  return PM_OK;
}

// ---- group variables (scheduler_impl.rs:155-200, storage.rs:150-215)

namespace {
// str::replace: every non-overlapping occurrence, scanning left to right; an empty pattern never occurs here
void replace_all(std::string& s, std::string_view pat, std::string_view with) {
  if (pat.empty()) return;
  std::string out;
  size_t pos = 0;
  for (;;) {
    const size_t hit = s.find(pat, pos);
    if (hit == std::string::npos) break;
    out.append(s, pos, hit - pos);
    out.append(with);
    pos = hit + pat.size();
  }
  if (pos == 0) return;  // no occurrence
  out.append(s, pos, std::string::npos);
  s.swap(out);
}
int32_t give(const std::string& r, char* out, size_t cap, size_t* needed) {
  if (needed) *needed = r.size() + 1;
  if (cap < r.size() + 1 || !out) {
    if (!out && cap == 0 && needed) return PM_OK;  // sizing call
    return pm::set_error(PM_ERANGE, "output buffer too small");
  }
  std::memcpy(out, r.c_str(), r.size() + 1);
  return PM_OK;
}
}  // namespace

uint32_t pm_host_last_file_idx(const char* total_upload_count) {
  // u32::from_str: optional '+', at least one ASCII digit, nothing else, no overflow; Err => 0
  if (!total_upload_count) return 0;
  const char* p = total_upload_count;
  if (*p == '+') ++p;
  if (!*p) return 0;
  uint64_t v = 0;
  for (; *p; ++p) {
    if (*p < '0' || *p > '9') return 0;
    v = v * 10 + uint64_t(*p - '0');
    if (v > 0xFFFFFFFFull) return 0;
  }
  return v ? uint32_t(v - 1) : 0u;  // saturating_sub(1)
}

uint32_t pm_host_task_state(const char* s) {
  // TaskState::from(&str), shared/src/models/task.rs:24-37: a match on the exact text, `"UNKNOWN" | &_` for the rest
  static const char* const names[PM_TS_N] = {"PENDING", "PULLING", "RUNNING", "COMPLETED", "FAILED", "PAUSED", "RESTARTING", "UNKNOWN"};
  if (!s) return PM_TS_UNKNOWN;
  for (uint32_t k = 0; k < PM_TS_N; ++k)
    if (!std::strcmp(s, names[k])) return k;
  return PM_TS_UNKNOWN;
}

int32_t pm_host_group_vars(const char* in, const pm_group_vars* v, char* out, size_t cap, size_t* needed) {
  if (!in || !v || !v->next_p2p_address || !v->group_id || !v->total_upload_count)
    return pm::set_error(PM_EINVAL, "null argument");
  std::string s(in);
  replace_all(s, "${GROUP_INDEX}", std::to_string(v->group_index));
  replace_all(s, "${GROUP_SIZE}", std::to_string(v->group_size));
  replace_all(s, "${NEXT_P2P_ADDRESS}", v->next_p2p_address);
  replace_all(s, "${GROUP_ID}", v->group_id);
  replace_all(s, "${TOTAL_UPLOAD_COUNT}", v->total_upload_count);
  replace_all(s, "${LAST_FILE_IDX}", std::to_string(pm_host_last_file_idx(v->total_upload_count)));
  return give(s, out, cap, needed);
}

int32_t pm_host_volume_vars(const char* in, const char* group_id, char* out, size_t cap, size_t* needed) {
  if (!in || !group_id) return pm::set_error(PM_EINVAL, "null argument");
  std::string s(in);
  replace_all(s, "${GROUP_ID}", group_id);
  return give(s, out, cap, needed);
}

int32_t pm_host_upload_name_vars(const char* in, const char* group_id, uint32_t group_size, uint32_t group_index,
                                 uint64_t upload_count, char* out, size_t cap, size_t* needed) {
  if (!in) return pm::set_error(PM_EINVAL, "null argument");
  std::string s(in);
  if (group_id) {  // storage.rs:150-158: only for a node that is in a group
    replace_all(s, "${NODE_GROUP_ID}", group_id);
    replace_all(s, "${NODE_GROUP_SIZE}", std::to_string(group_size));
    replace_all(s, "${NODE_GROUP_INDEX}", std::to_string(group_index));
  }
  replace_all(s, "${TOTAL_UPLOAD_COUNT_AFTER}", std::to_string(upload_count));
  replace_all(s, "${CURRENT_FILE_INDEX}", std::to_string(upload_count ? upload_count - 1 : 0));
  return give(s, out, cap, needed);
}

// keccak-256 (rate 136, padding 0x01 ... 0x80) with the state as an array and the steps as loops: written apart from the
// device's unrolled permutation (pm_keccak.inc) on purpose, so that either checks the other
static void keccak_f1600_host(uint64_t s[25]) {
  static const unsigned rot[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
  uint64_t lfsr = 1;  // the round constants' bits: x^8 + x^6 + x^5 + x^4 + 1
  for (int round = 0; round < 24; ++round) {
    uint64_t c[5], b[25];
    for (int x = 0; x < 5; ++x) c[x] = s[x] ^ s[x + 5] ^ s[x + 10] ^ s[x + 15] ^ s[x + 20];
    for (int x = 0; x < 5; ++x) {
      const uint64_t r = c[(x + 1) % 5], d = c[(x + 4) % 5] ^ ((r << 1) | (r >> 63));
      for (int y = 0; y < 5; ++y) s[x + 5 * y] ^= d;
    }
    for (int x = 0; x < 5; ++x)
      for (int y = 0; y < 5; ++y) {
        const uint64_t v = s[x + 5 * y];
        const unsigned r = rot[x + 5 * y];
        b[y + 5 * ((2 * x + 3 * y) % 5)] = r ? (v << r) | (v >> (64 - r)) : v;
      }
    for (int y = 0; y < 5; ++y)
      for (int x = 0; x < 5; ++x) s[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]);
    for (int j = 0; j < 7; ++j) {
      if (lfsr & 1) s[0] ^= 1ull << ((1u << j) - 1u);
      lfsr = (lfsr << 1) ^ ((lfsr >> 7) ? 0x171ull : 0ull);
    }
  }
}

int32_t pm_host_keccak256(const uint8_t* bytes, size_t len, uint8_t* out32) {
  if ((len && !bytes) || !out32) return pm::set_error(PM_EINVAL, "null argument");
  uint64_t s[25] = {};
  const size_t blocks = len / 136 + 1;
  for (size_t blk = 0; blk < blocks; ++blk) {
    uint8_t block[136] = {};
    const size_t at = blk * 136, have = len > at ? std::min<size_t>(len - at, 136) : 0;
    if (have) std::memcpy(block, bytes + at, have);
    if (blk + 1 == blocks) block[have] ^= 0x01, block[135] ^= 0x80;
    for (int i = 0; i < 17; ++i) {
      uint64_t v = 0;
      for (int j = 0; j < 8; ++j) v |= uint64_t(block[8 * i + j]) << (8 * j);
      s[i] ^= v;
    }
    keccak_f1600_host(s);
  }
  for (int j = 0; j < 32; ++j) out32[j] = uint8_t(s[j / 8] >> (8 * (j % 8)));
  return PM_OK;
}

int32_t pm_host_eip55(const uint8_t* addr20, char* out43) {
  if (!addr20 || !out43) return pm::set_error(PM_EINVAL, "null argument");
  static const char hex[] = "0123456789abcdef";
  uint8_t text[40], digest[32];
  for (int i = 0; i < 20; ++i) text[2 * i] = uint8_t(hex[addr20[i] >> 4]), text[2 * i + 1] = uint8_t(hex[addr20[i] & 15]);
  pm_host_keccak256(text, 40, digest);
  out43[0] = '0', out43[1] = 'x';
  for (int i = 0; i < 40; ++i) {
    const unsigned nib = (i & 1) ? digest[i / 2] & 15u : digest[i / 2] >> 4;
    out43[2 + i] = char(text[i] >= 'a' && nib >= 8 ? text[i] - 32 : text[i]);
  }
  out43[42] = 0;
  return PM_OK;
}

}  // extern "C"

// secp256k1 public-key recovery on the host, with the numbers as arrays of four 64-bit limbs (least significant first), the
// steps as loops over them and one reduction for both moduli: written apart from the device's named-limb arithmetic
// (pm_secp256k1.inc) on purpose, so that either checks the other.  Public data: nothing here is constant time.
namespace {

typedef unsigned __int128 u128;
struct U256 {
  uint64_t w[4];
};
// a modulus m > 2^255 as its limbs and c = 2^256 - m (three limbs at the most)
struct Modulus {
  U256 m;
  uint64_t c[3];
};
const Modulus FP = {{{0xFFFFFFFEFFFFFC2Full, 0xFFFFFFFFFFFFFFFFull, 0xFFFFFFFFFFFFFFFFull, 0xFFFFFFFFFFFFFFFFull}}, {0x1000003D1ull, 0, 0}};
const Modulus FN = {{{0xBFD25E8CD0364141ull, 0xBAAEDCE6AF48A03Bull, 0xFFFFFFFFFFFFFFFEull, 0xFFFFFFFFFFFFFFFFull}},
                    {0x402DA1732FC9BEBFull, 0x4551231950B75FC4ull, 1}};
const U256 SECP_GX = {{0x59F2815B16F81798ull, 0x029BFCDB2DCE28D9ull, 0x55A06295CE870B07ull, 0x79BE667EF9DCBBACull}};
const U256 SECP_GY = {{0x9C47D08FFB10D4B8ull, 0xFD17B448A6855419ull, 0x5DA4FBFC0E1108A8ull, 0x483ADA7726A3C465ull}};

bool u_is_zero(const U256& a) { return !(a.w[0] | a.w[1] | a.w[2] | a.w[3]); }
bool u_eq(const U256& a, const U256& b) { return a.w[0] == b.w[0] && a.w[1] == b.w[1] && a.w[2] == b.w[2] && a.w[3] == b.w[3]; }
bool u_less(const U256& a, const U256& b) {
  for (int i = 3; i >= 0; --i)
    if (a.w[i] != b.w[i]) return a.w[i] < b.w[i];
  return false;
}
uint64_t u_add(U256& r, const U256& a, const U256& b) {
  u128 t = 0;
  for (int i = 0; i < 4; ++i) t += u128(a.w[i]) + b.w[i], r.w[i] = uint64_t(t), t >>= 64;
  return uint64_t(t);
}
uint64_t u_sub(U256& r, const U256& a, const U256& b) {
  uint64_t borrow = 0;
  for (int i = 0; i < 4; ++i) {
    const u128 t = u128(a.w[i]) - b.w[i] - borrow;
    r.w[i] = uint64_t(t), borrow = uint64_t(t >> 64) & 1u;
  }
  return borrow;
}
U256 m_add(const U256& a, const U256& b, const Modulus& M) {
  U256 r, t;
  const uint64_t carry = u_add(r, a, b);
  if (carry || !u_less(r, M.m)) u_sub(t, r, M.m), r = t;
  return r;
}
U256 m_sub(const U256& a, const U256& b, const Modulus& M) {
  U256 r, t;
  if (u_sub(r, a, b)) u_add(t, r, M.m), r = t;
  return r;
}
// a b mod m: the 512-bit product, then high half times c folded into the low half until nothing is left above 2^256
U256 m_mul(const U256& a, const U256& b, const Modulus& M) {
  uint64_t t[8] = {};
  for (int i = 0; i < 4; ++i) {
    u128 carry = 0;
    for (int j = 0; j < 4; ++j) carry += u128(a.w[i]) * b.w[j] + t[i + j], t[i + j] = uint64_t(carry), carry >>= 64;
    t[i + 4] = uint64_t(carry);
  }
  while (t[4] | t[5] | t[6] | t[7]) {
    uint64_t f[8] = {t[0], t[1], t[2], t[3], 0, 0, 0, 0};
    for (int i = 0; i < 4; ++i) {
      u128 carry = 0;
      for (int j = 0; j < 3; ++j) carry += u128(t[4 + i]) * M.c[j] + f[i + j], f[i + j] = uint64_t(carry), carry >>= 64;
      for (int k = i + 3; carry && k < 8; ++k) carry += f[k], f[k] = uint64_t(carry), carry >>= 64;
    }
    std::memcpy(t, f, sizeof t);
  }
  U256 r = {{t[0], t[1], t[2], t[3]}}, d;
  while (!u_less(r, M.m)) u_sub(d, r, M.m), r = d;
  return r;
}
// a^e mod m, the exponent's bits from the top
U256 m_pow(const U256& a, const U256& e, const Modulus& M) {
  U256 r = {{1, 0, 0, 0}};
  for (int i = 255; i >= 0; --i) {
    r = m_mul(r, r, M);
    if ((e.w[i >> 6] >> (i & 63)) & 1u) r = m_mul(r, a, M);
  }
  return r;
}
U256 m_inv(const U256& a, const Modulus& M) {  // Fermat: m is prime
  U256 e, two = {{2, 0, 0, 0}};
  u_sub(e, M.m, two);
  return m_pow(a, e, M);
}
U256 from_be(const uint8_t* p) {
  U256 r;
  for (int i = 0; i < 4; ++i) {
    uint64_t v = 0;
    for (int j = 0; j < 8; ++j) v = (v << 8) | p[8 * (3 - i) + j];
    r.w[i] = v;
  }
  return r;
}
void to_be(const U256& a, uint8_t* p) {
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 8; ++j) p[8 * (3 - i) + j] = uint8_t(a.w[i] >> (8 * (7 - j)));
}

// a point in Jacobian coordinates (x = X / Z^2, y = Y / Z^3); Z = 0 is infinity
struct Jac {
  U256 x, y, z;
};
Jac j_infinity() { return Jac{{{1, 0, 0, 0}}, {{1, 0, 0, 0}}, {{0, 0, 0, 0}}}; }
Jac j_double(const Jac& p) {
  if (u_is_zero(p.z)) return p;
  const U256 a = m_mul(p.x, p.x, FP), b = m_mul(p.y, p.y, FP), c = m_mul(b, b, FP);
  U256 d = m_add(p.x, b, FP);
  d = m_sub(m_sub(m_mul(d, d, FP), a, FP), c, FP);
  d = m_add(d, d, FP);
  const U256 e = m_add(m_add(a, a, FP), a, FP), f = m_mul(e, e, FP);
  Jac r;
  r.x = m_sub(f, m_add(d, d, FP), FP);
  U256 c8 = m_add(c, c, FP);
  c8 = m_add(c8, c8, FP), c8 = m_add(c8, c8, FP);
  r.y = m_sub(m_mul(e, m_sub(d, r.x, FP), FP), c8, FP);
  r.z = m_mul(p.y, p.z, FP);
  r.z = m_add(r.z, r.z, FP);
  return r;
}
// p + (qx, qy), the second one affine and not infinity
Jac j_add_affine(const Jac& p, const U256& qx, const U256& qy) {
  if (u_is_zero(p.z)) return Jac{qx, qy, {{1, 0, 0, 0}}};
  const U256 zz = m_mul(p.z, p.z, FP), u2 = m_mul(qx, zz, FP), s2 = m_mul(qy, m_mul(p.z, zz, FP), FP);
  const U256 h = m_sub(u2, p.x, FP), rr = m_sub(s2, p.y, FP);
  if (u_is_zero(h)) return u_is_zero(rr) ? j_double(p) : j_infinity();  // equal points; opposite points
  const U256 hh = m_mul(h, h, FP), hhh = m_mul(h, hh, FP), v = m_mul(p.x, hh, FP);
  Jac r;
  r.x = m_sub(m_sub(m_mul(rr, rr, FP), hhh, FP), m_add(v, v, FP), FP);
  r.y = m_sub(m_mul(rr, m_sub(v, r.x, FP), FP), m_mul(p.y, hhh, FP), FP);
  r.z = m_mul(p.z, h, FP);
  return r;
}
// k (px, py) by double-and-add from the top bit
Jac j_mul(const U256& k, const U256& px, const U256& py) {
  Jac r = j_infinity();
  for (int i = 255; i >= 0; --i) {
    r = j_double(r);
    if ((k.w[i >> 6] >> (i & 63)) & 1u) r = j_add_affine(r, px, py);
  }
  return r;
}
bool j_affine(const Jac& p, U256& x, U256& y) {
  if (u_is_zero(p.z)) return false;
  const U256 zi = m_inv(p.z, FP), zi2 = m_mul(zi, zi, FP);
  x = m_mul(p.x, zi2, FP);
  y = m_mul(p.y, m_mul(zi, zi2, FP), FP);
  return true;
}

}  // namespace

extern "C" {

// Q = r^-1 (s R - z G) as two products and one addition (the device interleaves them: pm_secp256k1.inc)
int32_t pm_host_ecrecover(const uint8_t* hash32, const uint8_t* sig65, uint8_t* addr20) {
  if (!hash32 || !sig65 || !addr20) return pm::set_error(PM_EINVAL, "null argument");
  std::memset(addr20, 0, 20);
  const uint8_t v = sig65[64];
  if (v != 0 && v != 1 && v != 27 && v != 28) return pm::set_error(PM_EPARSE, "not a recovery id");
  const unsigned parity = (v == 1 || v == 28) ? 1u : 0u;  // (0, 27: even; 1, 28: odd)
  const U256 r = from_be(sig65), s = from_be(sig65 + 32);
  if (u_is_zero(r) || u_is_zero(s) || !u_less(r, FN.m) || !u_less(s, FN.m)) return pm::set_error(PM_EPARSE, "r or s out of range");
  // R: x = r itself, y = (x^3 + 7)^((p + 1) / 4) if that is a root
  const U256 seven = {{7, 0, 0, 0}};
  const U256 rhs = m_add(m_mul(m_mul(r, r, FP), r, FP), seven, FP);
  const U256 exp = {{0xFFFFFFFFBFFFFF0Cull, 0xFFFFFFFFFFFFFFFFull, 0xFFFFFFFFFFFFFFFFull, 0x3FFFFFFFFFFFFFFFull}};
  U256 y = m_pow(rhs, exp, FP);
  if (!u_eq(m_mul(y, y, FP), rhs)) return pm::set_error(PM_EPARSE, "r is no x coordinate");
  if ((y.w[0] & 1u) != parity) y = m_sub(U256{{0, 0, 0, 0}}, y, FP);
  U256 z = from_be(hash32), t;
  if (!u_less(z, FN.m)) u_sub(t, z, FN.m), z = t;
  const U256 ri = m_inv(r, FN), u1 = m_mul(m_sub(U256{{0, 0, 0, 0}}, z, FN), ri, FN), u2 = m_mul(s, ri, FN);
  Jac q = j_mul(u2, r, y);
  U256 ax, ay;
  if (j_affine(j_mul(u1, SECP_GX, SECP_GY), ax, ay)) q = j_add_affine(q, ax, ay);
  U256 qx, qy;
  if (!j_affine(q, qx, qy)) return pm::set_error(PM_EPARSE, "the key is the point at infinity");
  uint8_t pub[64], digest[32];
  to_be(qx, pub), to_be(qy, pub + 32);
  pm_host_keccak256(pub, 64, digest);
  std::memcpy(addr20, digest + 12, 20);
  return PM_OK;
}

uint32_t pm_abi_version(void) { return PM_ABI_VERSION; }

}  // extern "C"
