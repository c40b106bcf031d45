// probe_test.cpp — GpuMatchPlugin::probe_configurations / configuration_overlap (protocol_amd/plugin/gpu_match_probe.cpp) and
// their C face (pm_plugin_probe_c.cpp) against tests/cpp/mock_engine.cpp + tests/cpp/mock_probe.cpp: the probes go down packed
// as the constructor packs the installed configurations (rows, alternatives, model rows of their own), their model table is
// built against the spec models the plugin interned, results come back under the probes' names with the overlap keyed by
// installed configuration name, a requirement string that does not parse is the constructor's error and asks the engine
// nothing, and an engine refusal is thrown as EngineError.
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "gpu_match_plugin.hpp"
#include "pm_plugin_c.h"
#include "pm_plugin_c_internal.hpp"

namespace mock_probe {
struct Asked {
  std::vector<pm_config_row> probes;
  std::vector<pm_gpu_alt_row> alts;
  std::vector<uint32_t> bits;
  uint32_t n_model_rows, n_classes;
  bool want_overlap, want_mask;
};
extern uint32_t n_cfgs, n_classes, overlap_calls;
extern int32_t fail_with;
extern std::vector<Asked> asked;
uint32_t why_at(uint32_t p, uint32_t j);
uint32_t idle_at(uint32_t p);
uint32_t overlap_at(uint32_t p, uint32_t c);
uint32_t pair_at(uint32_t a, uint32_t b);
}  // namespace mock_probe

using namespace orchestrator;

static int g_failed = 0;
#define CHECK(cond)                                                                      \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      std::fprintf(stderr, "  CHECK failed at %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                                        \
    }                                                                                    \
  } while (0)

static const int N = 12;
static const char* const MODELS[3] = {"NVIDIA A100 80GB", "NVIDIA H100 PCIe", "RTX 4090"};
static OrchestratorNode node(int k) {
  char s[48];
  std::snprintf(s, sizeof(s), "0x%040x", 0x500 + k * 11);
  OrchestratorNode n;
  n.address = Address(s);
  n.status = NodeStatus::Healthy;
  n.p2p_id = "p2p-" + std::to_string(k);
  ComputeSpecs specs;
  GpuSpecs gpu;
  gpu.count = 1;
  gpu.model = std::string(MODELS[k % 3]);
  gpu.memory_mb = 80000;
  specs.gpu = gpu;
  n.compute_specs = specs;
  return n;
}

static std::shared_ptr<GpuMatchPlugin> make_plugin() {
  // (the installed set has a model row of its own: the probes' rows must not continue its numbering)
  std::vector<NodeGroupConfiguration> cfgs = {{"pair", 2, 2, std::nullopt}, {"solo", 1, 1, std::string("gpu:model=4090")},
                                              {"trio", 3, 3, std::string("ram_mb=1")}};
  auto p = std::make_shared<GpuMatchPlugin>(cfgs, 0, nullptr, std::vector<std::shared_ptr<WebhookPlugin>>{});
  std::vector<OrchestratorNode> snap;
  for (int k = 0; k < N; ++k) snap.push_back(node(k));
  p->sync_nodes(snap);
  mock_probe::n_cfgs = 3;
  mock_probe::n_classes = 3;
  mock_probe::fail_with = PM_OK;
  mock_probe::asked.clear();
  mock_probe::overlap_calls = 0;
  return p;
}

static uint32_t popcount_row(const mock_probe::Asked& a, uint32_t row) {
  const uint32_t words = (a.n_classes + 31u) / 32u;
  uint32_t n = 0;
  for (uint32_t k = 0; k < words; ++k) n += uint32_t(__builtin_popcount(a.bits[row * words + k]));
  return n;
}

static const std::vector<NodeGroupConfiguration> PROBES = {
    {"wants-h100", 2, 4, std::string("gpu:count=1;gpu:model=h100")},
    {"anything", 1, 1, std::nullopt},
    {"a-or-h", 3, 8, std::string("cpu:cores=4;ram_mb=64;gpu:count=1;gpu:model=a100;gpu:count=8;gpu:model=h100;gpu:count=2;gpu:memory_mb=1000")},
    {"nobody-has", 1, 2, std::string("gpu:model=mi355x")}};

static void probes_are_packed_like_installed_configurations() {
  auto p = make_plugin();
  const std::vector<GpuMatchPlugin::ProbeResult> res = p->probe_configurations(PROBES);
  CHECK(mock_probe::asked.size() == 1 && res.size() == PROBES.size());
  const mock_probe::Asked& a = mock_probe::asked.back();
  CHECK(a.probes.size() == 4 && a.alts.size() == 5 && a.want_overlap && !a.want_mask);
  CHECK(a.probes[0].flags == PM_R_HAS_REQ && a.probes[0].alt_begin == 0 && a.probes[0].alt_count == 1);
  CHECK(a.probes[0].min_group_size == 2 && a.probes[0].max_group_size == 4);
  CHECK(a.probes[1].flags == 0 && a.probes[1].alt_count == 0 && a.probes[1].min_group_size == 1);
  CHECK(a.probes[2].flags == (PM_R_HAS_REQ | PM_R_CPU | PM_R_CPU_CORES | PM_R_RAM) && a.probes[2].cpu_cores == 4 &&
        a.probes[2].ram_mb == 64 && a.probes[2].alt_begin == 1 && a.probes[2].alt_count == 3);
  CHECK(a.probes[3].alt_begin == 4 && a.probes[3].alt_count == 1 && a.probes[3].max_group_size == 2);
  // the alternatives: model rows number the PROBES' requirement models from 0, in order
  CHECK(a.alts[0].flags == (PM_G_COUNT | PM_G_MODEL) && a.alts[0].count == 1 && a.alts[0].model_row == 0);
  CHECK(a.alts[1].flags == (PM_G_COUNT | PM_G_MODEL) && a.alts[1].count == 1 && a.alts[1].model_row == 1);
  CHECK(a.alts[2].flags == (PM_G_COUNT | PM_G_MODEL) && a.alts[2].count == 8 && a.alts[2].model_row == 2);
  CHECK(a.alts[3].flags == (PM_G_COUNT | PM_G_MEM) && a.alts[3].count == 2 && a.alts[3].memory_mb == 1000);
  CHECK(a.alts[4].flags == PM_G_MODEL && a.alts[4].model_row == 3);
  // the model table: four rows against the three interned spec models; h100 and a100 match one class each, mi355x none
  CHECK(a.n_model_rows == 4 && a.n_classes == 3 && a.bits.size() == 4);
  CHECK(popcount_row(a, 0) == 1 && popcount_row(a, 1) == 1 && popcount_row(a, 2) == 1 && popcount_row(a, 3) == 0);
  CHECK(a.bits[0] == a.bits[2] && a.bits[0] != a.bits[1] && a.bits[0] < 8 && a.bits[1] < 8);
  // the results: the probes' names, the engine's rows, the overlap under the installed names in constructor order
  for (uint32_t k = 0; k < res.size(); ++k) {
    const GpuMatchPlugin::ProbeResult& r = res[k];
    CHECK(r.name == PROBES[k].name);
    for (uint32_t j = 0; j < 10; ++j) CHECK(r.why[j] == mock_probe::why_at(k, j));
    CHECK(r.eligible_meets == mock_probe::why_at(k, 0) && r.idle_meets == mock_probe::idle_at(k));
    CHECK(r.idle_located == mock_probe::idle_at(k) - 1 && r.idle_exclusive == mock_probe::idle_at(k) - 2);
    CHECK(r.groups_max == mock_probe::idle_at(k) / PROBES[k].min_group_size);
    CHECK(r.groups_exclusive == (mock_probe::idle_at(k) - 2) / PROBES[k].min_group_size);
    CHECK(r.overlap.size() == 3 && r.overlap[0].first == "pair" && r.overlap[1].first == "solo" && r.overlap[2].first == "trio");
    for (uint32_t c = 0; c < r.overlap.size(); ++c) CHECK(r.overlap[c].second == mock_probe::overlap_at(k, c));
  }
  // no probes: nothing comes back
  CHECK(p->probe_configurations({}).empty());
}

static void bad_strings_and_refusals() {
  auto p = make_plugin();
  bool threw = false;
  try {
    p->probe_configurations({{"ok", 1, 1, std::nullopt}, {"bad", 1, 1, std::string("gpu:count=notanumber")}});
  } catch (const std::invalid_argument& x) {
    threw = std::string(x.what()).find("bad") != std::string::npos;
  }
  CHECK(threw && mock_probe::asked.empty());  // the constructor's error, before any engine call
  for (const NodeGroupConfiguration& c : {NodeGroupConfiguration{"zero", 0, 1, std::nullopt}, NodeGroupConfiguration{"inverted", 3, 2, std::nullopt}}) {
    threw = false;
    try {
      p->probe_configurations({c});
    } catch (const EngineError& x) {
      threw = x.code() == PM_EINVAL;
    }
    CHECK(threw);
  }
  mock_probe::n_classes = 2;  // a table built before a model was interned: the engine's refusal comes up
  threw = false;
  try {
    p->probe_configurations(PROBES);
  } catch (const EngineError& x) {
    threw = x.code() == PM_EINVAL;
  }
  CHECK(threw);
  mock_probe::fail_with = PM_ESTATE;
  for (int which = 0; which < 2; ++which) {
    threw = false;
    try {
      if (which) p->configuration_overlap();
      else p->probe_configurations(PROBES);
    } catch (const EngineError& x) {
      threw = x.code() == PM_ESTATE;
    }
    CHECK(threw);
  }
}

static void the_overlap_matrix() {
  auto p = make_plugin();
  const GpuMatchPlugin::ConfigurationOverlap o = p->configuration_overlap();
  CHECK(mock_probe::overlap_calls == 1);
  CHECK(o.names == (std::vector<std::string>{"pair", "solo", "trio"}) && o.idle.size() == 9);
  for (uint32_t a = 0; a < 3; ++a)
    for (uint32_t b = 0; b < 3; ++b) CHECK(o.idle[a * 3 + b] == mock_probe::pair_at(a, b));
}

template <typename F>
static std::string text_of(F call, int32_t* rc_out) {
  size_t need = 0;
  int32_t rc = call(nullptr, 0, &need);
  *rc_out = rc;
  if (rc == -1 || need == 0) return "";
  std::string buf(need, '\0');
  rc = call(buf.data(), buf.size(), &need);
  *rc_out = rc;
  buf.resize(need ? need - 1 : 0);
  return buf;
}

static void the_c_face() {
  pmx_plugin h;
  h.plugin = make_plugin();
  const pmx_config probes[2] = {{"wants-h100", 2, 4, "gpu:count=1;gpu:model=h100"}, {"anything", 1, 1, nullptr}};
  int32_t rc = 0;
  const std::string t = text_of([&](char* out, size_t cap, size_t* need) { return pmx_probe_configurations(&h, probes, 2, out, cap, need); }, &rc);
  CHECK(rc == 0);
  std::string want;
  for (uint32_t k = 0; k < 2; ++k) {
    const uint32_t idle = mock_probe::idle_at(k), mn = probes[k].min_group_size;
    want += std::string(probes[k].name) + "\t" + std::to_string(mock_probe::why_at(k, 0)) + "\t" + std::to_string(idle) + "\t" +
            std::to_string(idle - 1) + "\t" + std::to_string(idle - 2) + "\t" + std::to_string(idle / mn) + "\t" +
            std::to_string((idle - 2) / mn);
    for (uint32_t j = 0; j < 10; ++j) want += "\t" + std::to_string(mock_probe::why_at(k, j));
    const char* names[3] = {"pair", "solo", "trio"};
    for (uint32_t c = 0; c < 3; ++c) want += std::string("\t") + names[c] + "=" + std::to_string(mock_probe::overlap_at(k, c));
    want += "\n";
  }
  CHECK(t == want);
  const std::string o = text_of([&](char* out, size_t cap, size_t* need) { return pmx_configuration_overlap(&h, out, cap, need); }, &rc);
  CHECK(rc == 0 && o == "pair\t7\t14\t21\nsolo\t14\t28\t42\ntrio\t21\t42\t63\n");
  // a bad string, a refusal: -1 and a message
  const pmx_config bad[1] = {{"broken", 1, 1, "gpu:count=x"}};
  const size_t n_asked = mock_probe::asked.size();
  text_of([&](char* out, size_t cap, size_t* need) { return pmx_probe_configurations(&h, bad, 1, out, cap, need); }, &rc);
  CHECK(rc == -1 && std::string(pmx_last_error()).find("broken") != std::string::npos && mock_probe::asked.size() == n_asked);
  mock_probe::fail_with = PM_ESTATE;
  text_of([&](char* out, size_t cap, size_t* need) { return pmx_configuration_overlap(&h, out, cap, need); }, &rc);
  CHECK(rc == -1);
}

int main() {
  probes_are_packed_like_installed_configurations();
  bad_strings_and_refusals();
  the_overlap_matrix();
  the_c_face();
  std::printf("4 tests, %d failed checks\n", g_failed);
  return g_failed ? 1 : 0;
}
