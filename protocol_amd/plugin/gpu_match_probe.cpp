// gpu_match_probe.cpp — GpuMatchPlugin::probe_configurations / configuration_overlap (see gpu_match_plugin.hpp): the engine's
// probe calls (pm_probe_configs, pm_config_overlap) by configuration name and requirement string.  The twin of the same
// methods of rust/gpu_match_plugin.rs, statement for statement.  (A file of its own: the plugin's other methods are also
// linked against a mock engine that has not these exports.)
#include <algorithm>
#include <shared_mutex>

#include "gpu_match_plugin.hpp"

namespace orchestrator {

std::vector<GpuMatchPlugin::ProbeResult> GpuMatchPlugin::probe_configurations(const std::vector<NodeGroupConfiguration>& probes) const {
  std::vector<pm_config_row> rows;
  std::vector<pm_gpu_alt_row> alts;
  std::vector<std::string> req_models;
  pack_templates(probes, rows, alts, req_models);  // (throws before any engine call)
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);  // (LOCK ORDER: nodes, the engine)
  // the probes' model rule against the interned spec models: the list the installed table was last built against
  std::vector<const char*> spec_p, req_p;
  for (const std::string& s : nodes_.spec_models) spec_p.push_back(s.c_str());
  for (const std::string& s : req_models) req_p.push_back(s.c_str());
  const size_t words = (spec_p.size() + 31) / 32;
  std::vector<uint32_t> bits(std::max<size_t>(req_p.size() * words, 1), 0u);
  check(pm_host_build_model_table(req_p.data(), uint32_t(req_p.size()), spec_p.data(), uint32_t(spec_p.size()), bits.data()));
  const size_t C = config_names_.size();
  std::vector<pm_probe_row> out(std::max<size_t>(rows.size(), 1));
  std::vector<uint32_t> overlap(std::max<size_t>(rows.size() * C, 1), 0u);
  check(pm_probe_configs(engine_, rows.data(), uint32_t(rows.size()), alts.data(), uint32_t(alts.size()), bits.data(),
                         uint32_t(req_p.size()), uint32_t(spec_p.size()), out.data(), overlap.data(), nullptr));
  std::vector<ProbeResult> res(rows.size());
  for (size_t p = 0; p < rows.size(); ++p) {
    ProbeResult& r = res[p];
    const pm_probe_row& k = out[p];
    r.name = probes[p].name;
    for (size_t j = 0; j < r.why.size(); ++j) r.why[j] = k.why[j];
    r.eligible_meets = k.eligible_meets;
    r.idle_meets = k.idle_meets;
    r.idle_located = k.idle_located;
    r.idle_exclusive = k.idle_exclusive;
    r.groups_max = k.groups_max;
    r.groups_exclusive = k.groups_exclusive;
    r.overlap.reserve(C);
    for (size_t c = 0; c < C; ++c) r.overlap.emplace_back(config_names_[c], overlap[p * C + c]);
  }
  return res;
}

GpuMatchPlugin::ConfigurationOverlap GpuMatchPlugin::configuration_overlap() const {
  ConfigurationOverlap out;
  out.names = config_names_;
  const size_t C = config_names_.size();
  out.idle.assign(std::max<size_t>(C * C, 1), 0u);
  uint32_t n = 0;
  check(pm_config_overlap(engine_, out.idle.data(), uint32_t(C * C), &n));
  out.idle.resize(C * C);
  return out;
}

}  // namespace orchestrator
