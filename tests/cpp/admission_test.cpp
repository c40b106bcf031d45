// admission_test.cpp — the request gate's admission without a GPU: GpuMatchPlugin::enable_admission / admit_requests
// (protocol_amd/plugin/gpu_match_admission.cpp) with their C face (pm_plugin_admission_c.cpp), and sweep_statuses' switch to
// pm_liveness_sweep_beats, against tests/cpp/mock_engine.cpp + mock_addresses.cpp + mock_directory.cpp + mock_gate.cpp +
// mock_liveness.cpp + mock_admission.cpp: what the twin packs (flags, timestamps, nonces), one engine call per batch, all
// thirteen codes through it, and the states it refuses in.
//
// argv[1]: what tests/test_admission_cpp.py wrote from the big-integer model (this program cannot sign), one record a line:
//   signed <key> <address hex> <sig65 hex> <message>          (the message holds no blank)
#include <atomic>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <mutex>
#include <sstream>
#include <string>
#include <vector>

#include "gpu_match_plugin.hpp"
#include "pm_plugin_c.h"
#include "pm_plugin_c_internal.hpp"

namespace mock_gate {
extern std::mutex mu;
extern std::vector<uint8_t> status;
extern std::vector<std::string> calls;
}  // namespace mock_gate
namespace mock_liveness {
extern std::mutex mu;
extern std::atomic<uint32_t> W;
extern std::vector<std::string> calls;
}  // namespace mock_liveness
namespace mock_admission {
extern std::mutex mu;
extern bool on;
extern uint32_t enables;
extern std::vector<std::string> calls;
extern std::vector<uint64_t> last_column;
}  // namespace mock_admission

using namespace orchestrator;

static int g_failed = 0;
#define CHECK(cond)                                                                      \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      std::fprintf(stderr, "  CHECK failed at %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                                        \
    }                                                                                    \
  } while (0)

static std::map<std::pair<int, std::string>, std::string> g_sig;  // (key, message) -> signature hex
static std::map<int, std::string> g_addr;                         // key -> address hex
using Calls = std::vector<std::string>;
static const uint64_t T0 = 1700000000000ull;

static Calls take_calls() {
  std::lock_guard<std::mutex> lk(mock_admission::mu);
  Calls c;
  c.swap(mock_admission::calls);
  return c;
}
static OrchestratorNode node(const std::string& address, int k) {
  OrchestratorNode n;
  n.address = Address(address);
  n.status = NodeStatus::Healthy;
  n.p2p_id = "p2p-" + std::to_string(k);
  return n;
}
static std::shared_ptr<GpuMatchPlugin> make_plugin(bool book, bool admission) {
  auto p = std::make_shared<GpuMatchPlugin>(std::vector<NodeGroupConfiguration>{{"solo", 1, 1, std::nullopt}}, 0,
                                            [](const Address&, const std::string&) { return size_t(3); },
                                            std::vector<std::shared_ptr<WebhookPlugin>>{});
  p->clock = [] { return int64_t(555); };
  if (book) p->enable_address_book();
  if (admission) p->enable_admission();
  return p;
}
static int32_t code_of(const std::function<void()>& f) {
  try {
    f();
  } catch (const EngineError& e) {
    return e.code();
  }
  return 0;
}
static std::string msg(int k) { return "/heartbeat{\"n\":" + std::to_string(k) + "}"; }
static std::string nonce(int k) { return "nonce-" + std::to_string(100000 + k) + "-AbCdEf"; }
static GpuMatchPlugin::AdmitRequest request(int key, int m, std::optional<std::string> ts, std::optional<std::string> nonce_text, bool beat) {
  GpuMatchPlugin::AdmitRequest r;
  r.message = msg(m), r.signature = "0x" + g_sig.at({key, msg(m)}), r.address = "0x" + g_addr.at(key);
  r.timestamp = std::move(ts), r.nonce = std::move(nonce_text), r.heartbeat = beat;
  return r;
}
static const std::string NOW_S = std::to_string(T0 / 1000);

static void the_thirteen_codes_in_one_call() {
  auto p = make_plugin(true, true);
  p->sync_nodes({node("0x" + g_addr.at(0), 0), node("0x" + g_addr.at(1), 1), node("0x" + g_addr.at(2), 2)});
  {
    std::lock_guard<std::mutex> lk(mock_gate::mu);
    mock_gate::status = {uint8_t(PM_NS_HEALTHY), uint8_t(PM_NS_EJECTED), uint8_t(PM_NS_BANNED)};
  }
  const uint32_t row0 = 0;
  const uint64_t start = T0 - 5;
  const uint32_t count = 96;
  CHECK(pm_admission_rate_set(p->engine_ptr(), &row0, &start, &count, 1) == PM_OK);
  take_calls();
  GpuMatchPlugin::AdmitRequest bad_v = request(0, 0, NOW_S, nonce(0), true);
  bad_v.signature.replace(bad_v.signature.size() - 2, 2, "1d");  // v = 29
  GpuMatchPlugin::AdmitRequest no_key = request(0, 1, NOW_S, nonce(0), true);
  no_key.signature = std::string(64, '0') + std::string(63, '0') + "1" + "1b";  // r = 0
  GpuMatchPlugin::AdmitRequest flagged = request(0, 2, NOW_S, nonce(0), true);
  flagged.address = "0xnot-an-address";
  GpuMatchPlugin::AdmitRequest mismatch = request(0, 3, NOW_S, nonce(0), true);
  mismatch.address = "0x" + g_addr.at(1);
  const std::vector<GpuMatchPlugin::AdmitRequest> reqs = {
      bad_v,                                                        // 0 BAD_SIGNATURE
      no_key,                                                       // 1 NO_KEY
      flagged,                                                      // 2 BAD_ADDRESS
      mismatch,                                                     // 3 MISMATCH
      request(3, 4, NOW_S, nonce(0), true),                         // 4 UNKNOWN
      request(1, 5, NOW_S, nonce(0), true),                         // 5 EJECTED: none of these six has touched nonce 0
      request(0, 6, NOW_S, nonce(0), true),                         // 6 OK, the row's 97th request; stamps the beat
      request(0, 7, std::to_string(T0 / 1000 - 301), nonce(1), true),  // 7 EXPIRED (98th)
      request(0, 8, std::nullopt, std::nullopt, true),              // 8 NO_NONCE (99th), no timestamp either
      request(0, 9, "not-a-number", "bad_nonce_bad_nonce", true),   // 9 BAD_NONCE (100th); a timestamp that is no u64 is none
      request(0, 10, NOW_S, nonce(2), true),                        // 10 RATE_LIMITED
      request(2, 11, NOW_S, nonce(0), false),                       // 11 REPLAY, before the handler's ban check
      request(2, 6, NOW_S, nonce(3), true)};                        // 12 BANNED: no beat
  const GpuMatchPlugin::AdmitResult r = p->admit_requests(reqs, T0);
  const std::string ts = NOW_S, old = std::to_string(T0 / 1000 - 301);
  const Calls calls = take_calls();
  CHECK(calls.size() == 1);  // one engine call, the columns as parsed
  if (calls.size() == 1) {
    const std::string want = "admit now=" + std::to_string(T0) + " n=13 flags=[8,8,9,8,8,8,8,8,14,10,8,0,8] ts=[" + ts + "," + ts + "," + ts + "," +
                             ts + "," + ts + "," + ts + "," + ts + "," + old + ",-,-," + ts + "," + ts + "," + ts + "] nonces=[" + nonce(0) + "," +
                             nonce(0) + "," + nonce(0) + "," + nonce(0) + "," + nonce(0) + "," + nonce(0) + "," + nonce(0) + "," + nonce(1) +
                             ",-,bad_nonce_bad_nonce," + nonce(2) + "," + nonce(0) + "," + nonce(3) + "]";
    if (calls[0] != want) std::fprintf(stderr, "  got  %s\n  want %s\n", calls[0].c_str(), want.c_str());
    CHECK(calls[0] == want);
  }
  const uint32_t want[13] = {PM_RQ_BAD_SIGNATURE, PM_RQ_NO_KEY,  PM_RQ_BAD_ADDRESS, PM_RQ_MISMATCH,     PM_RQ_UNKNOWN, PM_RQ_EJECTED, PM_RQ_OK,
                             PM_RQ_EXPIRED,       PM_RQ_NO_NONCE, PM_RQ_BAD_NONCE,  PM_RQ_RATE_LIMITED, PM_RQ_REPLAY,  PM_RQ_BANNED};
  CHECK(r.verdicts.size() == 13);
  for (size_t k = 0; k < r.verdicts.size() && k < 13; ++k) {
    if (r.verdicts[k].code != want[k]) std::fprintf(stderr, "  request %zu: code %u\n", k, r.verdicts[k].code);
    CHECK(r.verdicts[k].code == want[k]);
  }
  for (uint32_t c = 0; c < PM_AD_N_CODES; ++c) CHECK(r.counts[c] == 1);
  CHECK(r.verdicts[6].row == 0 && r.verdicts[6].status == PM_NS_HEALTHY && r.verdicts[12].row == 2 && r.verdicts[4].row == 0xFFFFFFFFu);
  uint64_t w = 0, beats[3] = {9, 9, 9};
  uint32_t c = 0, live = 0, held = 0;
  const uint32_t rows[3] = {0, 1, 2};
  CHECK(pm_admission_rate_get(p->engine_ptr(), &row0, 1, &w, &c) == PM_OK && w == start && c == 100);
  CHECK(pm_beats_get(p->engine_ptr(), rows, 3, beats) == PM_OK && beats[0] == T0 && beats[1] == 0 && beats[2] == 0);
  CHECK(pm_admission_nonces(p->engine_ptr(), T0, &live, &held) == PM_OK && live == 2 && held == 2);  // nonce 0 and the banned node's
  // nothing to admit: no engine call
  CHECK(p->admit_requests({}, T0).verdicts.empty() && take_calls().empty());
}

static void the_states_it_refuses_in() {
  {
    auto p = make_plugin(false, false);
    take_calls();
    CHECK(code_of([&] { p->enable_admission(); }) == PM_ESTATE && take_calls().empty());  // the book is off: nothing reaches the engine
    CHECK(code_of([&] { p->admit_requests({request(0, 0, NOW_S, nonce(0), false)}, T0); }) == PM_ESTATE);
  }
  auto p = make_plugin(true, false);
  p->sync_nodes({node("0x" + g_addr.at(0), 0)});
  take_calls();
  CHECK(code_of([&] { p->admit_requests({request(0, 0, NOW_S, nonce(0), false)}, T0); }) == PM_ESTATE && take_calls().empty());
  p->enable_admission();
  CHECK((take_calls() == Calls{"enable on=1"}));
  CHECK(p->admit_requests({request(0, 0, NOW_S, nonce(0), false)}, T0).verdicts[0].code == PM_RQ_OK);
}

static void the_sweep_reads_the_later_column() {
  auto p = make_plugin(true, false);
  p->sync_nodes({node("0x" + g_addr.at(0), 0), node("0x" + g_addr.at(1), 1), node("0x" + g_addr.at(2), 2)});
  mock_liveness::W = 3;
  {
    std::lock_guard<std::mutex> lk(mock_gate::mu);
    mock_gate::status.clear();
  }
  p->enable_liveness(3);
  p->beat(Address("0x" + g_addr.at(1)), T0 - 100);
  take_calls();
  p->sweep_statuses(T0, {});
  CHECK(take_calls().empty());  // admission off: pm_liveness_sweep as ever
  p->enable_admission();
  CHECK(p->admit_requests({request(0, 0, std::nullopt, nonce(0), true), request(1, 1, std::nullopt, nonce(1), true)}, T0 - 200).counts[PM_RQ_OK] == 2);
  take_calls();
  {
    std::lock_guard<std::mutex> lk(mock_liveness::mu);
    mock_liveness::calls.clear();
  }
  p->sweep_statuses(T0, {});
  CHECK((take_calls() == Calls{"sweep_beats now=" + std::to_string(T0) + " host=[0," + std::to_string(T0 - 100) + ",0]"}));
  std::vector<uint64_t> column;
  {
    std::lock_guard<std::mutex> lk(mock_admission::mu);
    column = mock_admission::last_column;
  }
  CHECK((column == std::vector<uint64_t>{T0 - 200, T0 - 100, 0}));  // the device's, the plugin's own (later), neither
  mock_liveness::W = 0;
}

static void the_c_face() {
  pmx_plugin* h = nullptr;
  const pmx_config cfgs[1] = {{"solo", 1, 1, nullptr}};
  CHECK(pmx_create(cfgs, 1, 0, &h) == 0 && h);
  if (!h) return;
  {
    std::lock_guard<std::mutex> lk(mock_gate::mu);
    mock_gate::status.clear();
  }
  const std::string head = "0x" + g_sig.at({0, msg(0)}) + "\t0x" + g_addr.at(0) + "\t";
  const std::string lines = head + NOW_S + "\t" + nonce(7) + "\t1\t" + msg(0) + "\n" + head + "-\t" + nonce(7) + "\t0\t" + msg(0) + "\n" + head +
                            NOW_S + "\t-\t0\t" + msg(0) + "\n";
  size_t need = 0;
  CHECK(pmx_enable_admission(h) != 0);  // the book is off
  CHECK(pmx_enable_address_book(h) == 0);
  CHECK(pmx_admit_requests(h, lines.c_str(), T0, nullptr, 0, &need) != 0);  // admission is off
  CHECK(pmx_enable_admission(h) == 0);
  h->plugin->sync_nodes({node("0x" + g_addr.at(0), 0)});
  CHECK(pmx_admit_requests(h, "", T0, nullptr, 0, &need) == 0 && need > 0);
  std::string text(4096, '\0');
  CHECK(pmx_admit_requests(h, lines.c_str(), T0, text.data(), text.size(), &need) == 0);
  text.resize(need ? need - 1 : 0);
  const std::string a = "\t0\t-\t0x" + g_addr.at(0) + "\n";
  const std::string want = "ok" + a + "replay" + a + "no_nonce" + a + "counts\t0\t0\t0\t0\t0\t0\t0\t1\t0\t0\t0\t1\t1\n";
  if (text != want) std::fprintf(stderr, "  got:\n%s", text.c_str());
  CHECK(text == want);
  CHECK(pmx_admit_requests(h, "a line\twith\ttoo few\ttabs\n", T0, text.data(), text.size(), &need) != 0);
  pmx_destroy(h);
}

int main(int argc, char** argv) {
  if (argc < 2) return std::fprintf(stderr, "usage: admission_test <cases>\n"), 2;
  std::ifstream in(argv[1]);
  for (std::string line; std::getline(in, line);) {
    std::istringstream is(line);
    std::string kind, addr, sig, m;
    int key;
    is >> kind >> key >> addr >> sig >> m;
    if (kind != "signed") continue;
    g_addr[key] = addr;
    g_sig[{key, m}] = sig;
  }
  struct {
    const char* name;
    void (*fn)();
  } tests[] = {{"the_thirteen_codes_in_one_call", the_thirteen_codes_in_one_call},
               {"the_states_it_refuses_in", the_states_it_refuses_in},
               {"the_sweep_reads_the_later_column", the_sweep_reads_the_later_column},
               {"the_c_face", the_c_face}};
  int n = 0;
  for (auto& t : tests) {
    const int before = g_failed;
    t.fn();
    std::printf("%s %s\n", g_failed == before ? "ok  " : "FAIL", t.name);
    ++n;
  }
  std::printf("%d tests, %d failed checks\n", n, g_failed);
  return g_failed ? 1 : 0;
}
