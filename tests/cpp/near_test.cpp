// near_test.cpp — GpuMatchPlugin::nearest_nodes (protocol_amd/plugin/gpu_match_near.cpp) and its C face pmx_nearest_nodes
// (pm_plugin_near_c.cpp) against tests/cpp/mock_engine.cpp + tests/cpp/mock_near.cpp: the address becomes the worker row and
// the configuration name its index, the seed goes down as PM_NEAR_SEED, worker rows come back as node addresses with their
// distances, an unknown address is the not-found result and asks the engine nothing, an unknown configuration name is an
// error, and an engine refusal is thrown as EngineError.
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "gpu_match_plugin.hpp"
#include "pm_plugin_c.h"
#include "pm_plugin_c_internal.hpp"

namespace mock_near {
struct Asked {
  uint32_t origin, config, pool, k;
};
extern uint32_t n_workers, n_cfgs;
extern int32_t fail_with;
extern bool seed_finds_nobody;
extern std::vector<Asked> asked;
uint32_t seed_row(uint32_t config);
uint32_t listed(uint32_t k);
uint32_t worker_at(uint32_t origin, uint32_t j);
double km_at(uint32_t config, uint32_t j);
}  // namespace mock_near

using namespace orchestrator;

static int g_failed = 0;
#define CHECK(cond)                                                                      \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      std::fprintf(stderr, "  CHECK failed at %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                                        \
    }                                                                                    \
  } while (0)

static const int N = 23;
static std::string addr(int k) {
  char s[48];
  std::snprintf(s, sizeof(s), "0x%040x", 0x300 + k * 7);
  return s;
}
static OrchestratorNode node(int k) {
  OrchestratorNode n;
  n.address = Address(addr(k));
  n.status = NodeStatus::Healthy;
  n.p2p_id = "p2p-" + std::to_string(k);
  return n;
}

static std::shared_ptr<GpuMatchPlugin> make_plugin() {
  std::vector<NodeGroupConfiguration> cfgs = {{"pair", 2, 2, std::nullopt}, {"solo", 1, 1, std::nullopt}};
  auto p = std::make_shared<GpuMatchPlugin>(cfgs, 0, nullptr, std::vector<std::shared_ptr<WebhookPlugin>>{});
  std::vector<OrchestratorNode> snap;
  for (int k = 0; k < N; ++k) snap.push_back(node(k));
  p->sync_nodes(snap);
  mock_near::n_workers = N;
  mock_near::n_cfgs = 2;
  mock_near::fail_with = PM_OK;
  mock_near::seed_finds_nobody = false;
  mock_near::asked.clear();
  return p;
}
// the row the plugin gave an address (the node table need not be in snapshot order)
static uint32_t row(const GpuMatchPlugin& p, int k) {
  const std::optional<uint32_t> r = p.row_of(Address(addr(k)));
  CHECK(r.has_value());
  return r.value_or(0);
}
static std::string addr_of_row(const GpuMatchPlugin& p, uint32_t w) {
  for (int k = 0; k < N; ++k)
    if (row(p, k) == w) return addr(k);
  CHECK(!"no node has this row");
  return "";
}

static void by_address_and_by_seed() {
  auto p = make_plugin();
  const auto r = p->nearest_nodes(addr(9), "solo", PM_NEAR_ELIGIBLE, 3);
  CHECK(r.has_value());
  CHECK(mock_near::asked.size() == 1);
  const mock_near::Asked a = mock_near::asked.back();
  CHECK(a.origin == row(*p, 9) && a.config == 1 && a.pool == PM_NEAR_ELIGIBLE && a.k == 3);
  CHECK(r->origin == addr(9) && r->candidates == 11 && r->located == 7 && r->nodes.size() == 3);
  for (uint32_t j = 0; j < r->nodes.size(); ++j) {
    CHECK(r->nodes[j].first == addr_of_row(*p, mock_near::worker_at(a.origin, j)));
    CHECK(r->nodes[j].second == mock_near::km_at(1, j));
  }
  // the seed: PM_NEAR_SEED goes down, the origin comes back as an address; k above what there is: five entries, the last
  // one unmeasured
  const auto s = p->nearest_nodes(std::nullopt, "pair", PM_NEAR_IDLE, 64);
  CHECK(s.has_value() && mock_near::asked.size() == 2);
  CHECK(mock_near::asked.back().origin == PM_NEAR_SEED && mock_near::asked.back().config == 0 && mock_near::asked.back().k == 64);
  CHECK(s->origin == addr_of_row(*p, mock_near::seed_row(0)) && s->candidates == 10 && s->nodes.size() == 5);
  CHECK(s->nodes[4].second == DBL_MAX && s->nodes[3].second == mock_near::km_at(0, 3));
  // defaults: the IDLE pool, k = 16
  CHECK(p->nearest_nodes(addr(0), "pair").has_value());
  CHECK(mock_near::asked.back().pool == PM_NEAR_IDLE && mock_near::asked.back().k == 16);
  // the seed rule found nobody: a result with an empty origin and no nodes
  mock_near::seed_finds_nobody = true;
  const auto e = p->nearest_nodes(std::nullopt, "solo", PM_NEAR_IDLE, 8);
  CHECK(e.has_value() && e->origin.empty() && e->nodes.empty() && e->candidates == 0 && e->located == 0);
}

static void unknown_address_unknown_name_and_refusals() {
  auto p = make_plugin();
  CHECK(!p->nearest_nodes(addr(N + 5), "pair", PM_NEAR_IDLE, 4).has_value());   // not found ...
  CHECK(!p->nearest_nodes(std::string("not an address"), "pair", PM_NEAR_IDLE, 4).has_value());
  CHECK(mock_near::asked.empty());                                              // ... and the engine was not asked
  bool threw = false;
  try {
    p->nearest_nodes(addr(1), "no such configuration", PM_NEAR_IDLE, 4);
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  CHECK(threw && mock_near::asked.empty());
  for (uint32_t k : {0u, PM_NEAR_MAX_K + 1u}) {                                 // the engine's refusals come up as EngineError
    threw = false;
    try {
      p->nearest_nodes(addr(1), "pair", PM_NEAR_IDLE, k);
    } catch (const EngineError& x) {
      threw = x.code() == PM_EINVAL;
    }
    CHECK(threw);
  }
  threw = false;
  try {
    p->nearest_nodes(addr(1), "pair", 7, 4);
  } catch (const EngineError& x) {
    threw = x.code() == PM_EINVAL;
  }
  CHECK(threw);
  mock_near::fail_with = PM_ESTATE;
  threw = false;
  try {
    p->nearest_nodes(std::nullopt, "pair", PM_NEAR_IDLE, 4);
  } catch (const EngineError& x) {
    threw = x.code() == PM_ESTATE;
  }
  CHECK(threw);
}

static std::string text_of(pmx_plugin* h, const char* address, const char* name, uint32_t pool, uint32_t k, int32_t* found,
                           int32_t* rc_out) {
  size_t need = 0;
  int32_t rc = pmx_nearest_nodes(h, address, name, pool, k, found, nullptr, 0, &need);
  *rc_out = rc;
  if (rc == -1 || need == 0) return "";
  std::string buf(need, '\0');
  rc = pmx_nearest_nodes(h, address, name, pool, k, found, buf.data(), buf.size(), &need);
  *rc_out = rc;
  buf.resize(need ? need - 1 : 0);
  return buf;
}

static void the_c_face() {
  pmx_plugin h;
  h.plugin = make_plugin();
  int32_t found = -1, rc = 0;
  const std::string t = text_of(&h, addr(4).c_str(), "solo", PM_NEAR_IDLE, 5, &found, &rc);
  CHECK(rc == 0 && found == 1);
  const uint32_t o = row(*h.plugin, 4);
  std::string want = "origin\t" + addr(4) + "\t10\t7\n";
  for (uint32_t j = 0; j < 5; ++j) {
    char km[40] = "-";
    if (j != 4) std::snprintf(km, sizeof km, "%.17g", mock_near::km_at(1, j));
    want += addr_of_row(*h.plugin, mock_near::worker_at(o, j)) + "\t" + km + "\n";
  }
  CHECK(t == want);
  CHECK(std::strtod("1000.25", nullptr) == mock_near::km_at(1, 0) && t.find("\t1000.25\n") != std::string::npos);
  // NULL address: the seed
  const std::string s = text_of(&h, nullptr, "pair", PM_NEAR_ELIGIBLE, 2, &found, &rc);
  CHECK(rc == 0 && found == 1 && mock_near::asked.back().origin == PM_NEAR_SEED && mock_near::asked.back().pool == PM_NEAR_ELIGIBLE);
  CHECK(s.rfind("origin\t" + addr_of_row(*h.plugin, mock_near::seed_row(0)) + "\t11\t7\n", 0) == 0);
  mock_near::seed_finds_nobody = true;
  CHECK(text_of(&h, nullptr, "pair", PM_NEAR_IDLE, 2, &found, &rc) == "origin\t-\t0\t0\n" && found == 1 && rc == 0);
  // an unknown address: found = 0, empty text; an unknown configuration name, an engine refusal: -1 and a message
  const size_t n_asked = mock_near::asked.size();
  CHECK(text_of(&h, addr(N + 1).c_str(), "pair", PM_NEAR_IDLE, 2, &found, &rc).empty() && found == 0 && rc == 0);
  CHECK(mock_near::asked.size() == n_asked);
  text_of(&h, addr(1).c_str(), "nope", PM_NEAR_IDLE, 2, &found, &rc);
  CHECK(rc == -1 && std::string(pmx_last_error()).find("nope") != std::string::npos);
  text_of(&h, addr(1).c_str(), "pair", PM_NEAR_IDLE, 0, &found, &rc);
  CHECK(rc == -1);
}

int main() {
  by_address_and_by_seed();
  unknown_address_unknown_name_and_refusals();
  the_c_face();
  std::printf("3 tests, %d failed checks\n", g_failed);
  return g_failed ? 1 : 0;
}
