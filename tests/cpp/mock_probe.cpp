// mock_probe.cpp — TEST INFRASTRUCTURE: the probe exports of include/pm_engine.h (pm_probe_configs, pm_config_overlap), which
// tests/cpp/mock_engine.cpp does not define.  It keeps a copy of the tables it was given and answers canned values that
// tests/cpp/probe_test.cpp derives from the probe's index, so that a row under the wrong name or configuration shows.
#include <cstdint>
#include <vector>

#include "pm_engine.h"

namespace mock_probe {
uint32_t n_cfgs = 0;        // what the mock engine holds
uint32_t n_classes = 0;     // ... and its model table's class count
int32_t fail_with = PM_OK;  // != PM_OK: every call returns it
struct Asked {
  std::vector<pm_config_row> probes;
  std::vector<pm_gpu_alt_row> alts;
  std::vector<uint32_t> bits;
  uint32_t n_model_rows, n_classes;
  bool want_overlap, want_mask;
};
std::vector<Asked> asked;
uint32_t overlap_calls = 0;
uint32_t why_at(uint32_t p, uint32_t j) { return 100u * p + j + 1u; }
uint32_t idle_at(uint32_t p) { return 50u + 3u * p; }
uint32_t overlap_at(uint32_t p, uint32_t c) { return 1000u * p + c + 5u; }
uint32_t pair_at(uint32_t a, uint32_t b) { return 7u * (a + 1u) * (b + 1u); }
}  // namespace mock_probe

extern "C" {

int32_t pm_probe_configs(pm_engine*, const pm_config_row* probes, uint32_t n_probes, const pm_gpu_alt_row* alts, uint32_t n_alts,
                         const uint32_t* model_bits, uint32_t n_model_rows, uint32_t n_classes, pm_probe_row* rows,
                         uint32_t* overlap, uint64_t* mask_out) {
  using namespace mock_probe;
  if (fail_with != PM_OK) return fail_with;
  if (n_probes > PM_MAX_CONFIGS || (n_probes && (!probes || !rows)) || (n_alts && !alts)) return PM_EINVAL;
  for (uint32_t p = 0; p < n_probes; ++p) {
    if (!probes[p].min_group_size || probes[p].max_group_size < probes[p].min_group_size) return PM_EINVAL;
    if (uint64_t(probes[p].alt_begin) + probes[p].alt_count > n_alts) return PM_ERANGE;
  }
  if (!n_probes) return PM_OK;
  if (n_classes != mock_probe::n_classes) return PM_EINVAL;
  Asked a;
  a.probes.assign(probes, probes + n_probes);
  if (n_alts) a.alts.assign(alts, alts + n_alts);
  const size_t words = size_t(n_model_rows) * ((n_classes + 31u) / 32u);
  if (words) a.bits.assign(model_bits, model_bits + words);
  a.n_model_rows = n_model_rows, a.n_classes = n_classes;
  a.want_overlap = overlap != nullptr, a.want_mask = mask_out != nullptr;
  asked.push_back(a);
  for (uint32_t p = 0; p < n_probes; ++p) {
    pm_probe_row& r = rows[p];
    for (uint32_t j = 0; j < PM_WHY_N; ++j) r.why[j] = why_at(p, j);
    r.eligible_meets = r.why[PM_WHY_OK];
    r.idle_meets = idle_at(p);
    r.idle_located = idle_at(p) - 1u;
    r.idle_exclusive = idle_at(p) - 2u;
    r.groups_max = r.idle_meets / probes[p].min_group_size;
    r.groups_exclusive = r.idle_exclusive / probes[p].min_group_size;
    if (overlap)
      for (uint32_t c = 0; c < n_cfgs; ++c) overlap[p * n_cfgs + c] = overlap_at(p, c);
  }
  return PM_OK;
}

int32_t pm_config_overlap(pm_engine*, uint32_t* overlap, uint32_t cap, uint32_t* n_out) {
  using namespace mock_probe;
  if (fail_with != PM_OK) return fail_with;
  ++overlap_calls;
  if (n_out) *n_out = n_cfgs;
  if (cap < n_cfgs * n_cfgs || (n_cfgs && !overlap)) return PM_ERANGE;
  for (uint32_t a = 0; a < n_cfgs; ++a)
    for (uint32_t b = 0; b < n_cfgs; ++b) overlap[a * n_cfgs + b] = pair_at(a, b);
  return PM_OK;
}

}  // extern "C"
