// mock_spread.cpp — TEST INFRASTRUCTURE: the group geography exports of include/pm_engine.h (pm_group_spread, pm_config_spread,
// pm_force_regroup), which tests/cpp/mock_engine.cpp does not define.  They go through the mock engine's own exports
// (pm_get_groups, pm_dissolve_group_by_id), record what they were asked, and answer canned values that
// tests/cpp/spread_test.cpp derives from a group's id and members, so that a row under the wrong id or name shows.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "pm_engine.h"

namespace mock_spread {
uint32_t n_cfgs = 0;        // what the mock engine holds
int32_t fail_with = PM_OK;  // != PM_OK: every call returns it
struct Asked {
  uint32_t config, metric;
  double threshold_km;
};
std::vector<Asked> regroups;  // what pm_force_regroup was asked
double diameter_of(uint64_t id) { return double(id % 9973u) + 0.25; }

struct Listed {
  std::vector<pm_group> groups;
  std::vector<uint32_t> members;
};
static int32_t list(pm_engine* e, Listed* out) {
  uint32_t ng = 0, nm = 0;
  int32_t rc = pm_get_groups(e, nullptr, nullptr, 0, &ng, nullptr, 0, &nm);
  if (rc != PM_OK) return rc;
  out->groups.resize(ng);
  out->members.resize(nm);
  return pm_get_groups(e, nullptr, ng ? out->groups.data() : nullptr, ng, &ng, nm ? out->members.data() : nullptr, nm, &nm);
}
}  // namespace mock_spread

extern "C" {

// a group's row: located = its size, far_a / far_b = its first / last member, hop_from = its second (or first), diameter a
// function of the id, ring twice that, the longest hop half of it
int32_t pm_group_spread(pm_engine* e, pm_group_spread_row* out, uint32_t cap, uint32_t* n_groups) {
  if (mock_spread::fail_with != PM_OK) return mock_spread::fail_with;
  mock_spread::Listed l;
  const int32_t rc = mock_spread::list(e, &l);
  if (rc != PM_OK) return rc;
  const uint32_t n = uint32_t(l.groups.size());
  if (n_groups) *n_groups = n;
  if (cap < n) return PM_ERANGE;
  for (uint32_t g = 0; g < n; ++g) {
    const pm_group& gr = l.groups[g];
    const uint32_t* m = l.members.data() + gr.member_begin;
    pm_group_spread_row& r = out[g];
    r.located = gr.n_members;
    r.ring_hops = gr.n_members > 1 ? gr.n_members : 0;
    r.far_a = gr.n_members > 1 ? m[0] : PM_NONE;
    r.far_b = gr.n_members > 1 ? m[gr.n_members - 1] : PM_NONE;
    r.hop_from = gr.n_members > 1 ? m[1] : PM_NONE;
    r._pad = 0;
    r.diameter_km = gr.n_members > 1 ? mock_spread::diameter_of(gr.id) : 0.0;
    r.ring_km = 2.0 * r.diameter_km;
    r.longest_hop_km = 0.5 * r.diameter_km;
  }
  return PM_OK;
}

// row c: every field a distinct function of c
int32_t pm_config_spread(pm_engine*, pm_config_spread_row* out, uint32_t cap, uint32_t* n_cfgs) {
  if (mock_spread::fail_with != PM_OK) return mock_spread::fail_with;
  if (n_cfgs) *n_cfgs = mock_spread::n_cfgs;
  if (cap < mock_spread::n_cfgs) return PM_ERANGE;
  for (uint32_t c = 0; c < mock_spread::n_cfgs; ++c) {
    pm_config_spread_row& r = out[c];
    r.groups = 100 + c;
    r.measured = 90 + c;
    for (uint32_t k = 0; k < PM_SPREAD_BUCKETS; ++k) r.hist[k] = 10 * c + k;
    r._pad = 0;
    r.max_diameter_km = 1000.5 + c;
    r.max_hop_km = 500.25 + c;
    r.sum_diameter_m = 7000000000ull + c;
    r.sum_ring_m = 9000000000ull + c;
  }
  return PM_OK;
}

// the selection of the header over the canned rows, dissolved through the mock engine in "{:x}" text order
int32_t pm_force_regroup(pm_engine* e, uint32_t config, uint32_t metric, double threshold_km, uint32_t* dissolved_groups,
                         uint32_t* affected_workers) {
  if (mock_spread::fail_with != PM_OK) return mock_spread::fail_with;
  mock_spread::regroups.push_back({config, metric, threshold_km});
  if (dissolved_groups) *dissolved_groups = 0;
  if (affected_workers) *affected_workers = 0;
  if (config >= mock_spread::n_cfgs) return PM_ERANGE;
  if (metric > PM_REGROUP_LONGEST_HOP || (metric != PM_REGROUP_ALL && !(threshold_km >= 0.0))) return PM_EINVAL;
  mock_spread::Listed l;
  const int32_t rc = mock_spread::list(e, &l);
  if (rc != PM_OK) return rc;
  std::vector<std::pair<std::string, const pm_group*>> sel;
  for (const pm_group& g : l.groups) {
    if (g.config != config) continue;
    const double d = g.n_members > 1 ? mock_spread::diameter_of(g.id) : 0.0;
    if (metric == PM_REGROUP_DIAMETER && !(g.n_members > 1 && d >= threshold_km)) continue;
    if (metric == PM_REGROUP_LONGEST_HOP && !(g.n_members > 1 && 0.5 * d >= threshold_km)) continue;
    char text[24];
    std::snprintf(text, sizeof text, "%llx", (unsigned long long)g.id);
    sel.emplace_back(text, &g);
  }
  std::sort(sel.begin(), sel.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
  uint32_t workers = 0;
  for (const auto& s : sel) {
    uint32_t done = 0;
    const int32_t rd = pm_dissolve_group_by_id(e, s.second->id, &done);
    if (rd != PM_OK) return rd;
    workers += s.second->n_members;
  }
  if (dissolved_groups) *dissolved_groups = uint32_t(sel.size());
  if (affected_workers) *affected_workers = workers;
  return PM_OK;
}

}  // extern "C"
