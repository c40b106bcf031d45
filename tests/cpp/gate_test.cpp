// gate_test.cpp — the request gate without a GPU: pm_host_ecrecover (protocol_amd/csrc/pm_host.cpp) on the named cases of
// tests/gate_cases.py, and GpuMatchPlugin::verify_requests (protocol_amd/plugin/gpu_match_gate.cpp) with its C face
// (pm_plugin_gate_c.cpp) against tests/cpp/mock_engine.cpp + mock_addresses.cpp + mock_directory.cpp + mock_gate.cpp: the
// signature parser, the address flag, the precedence of all eight codes, and one engine call per batch.
//
// argv[1]: what tests/test_gate_cpp.py wrote from the big-integer model (this program cannot sign), one record a line:
//   case <name> <hash32 hex> <sig65 hex> <ok> <address hex>
//   signed <key> <address hex> <sig65 hex> <message>          (the message holds no blank)
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

using namespace orchestrator;

static int g_failed = 0;
#define CHECK(cond)                                                                      \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      std::fprintf(stderr, "  CHECK failed at %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                                        \
    }                                                                                    \
  } while (0)

struct Case {
  std::string name, hash, sig, address;
  int ok;
};
static std::vector<Case> g_cases;
static std::map<std::pair<int, std::string>, std::string> g_sig;  // (key, message) -> signature hex
static std::map<int, std::string> g_addr;                         // key -> address hex

static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> out;
  for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back(uint8_t(std::stoi(s.substr(i, 2), nullptr, 16)));
  return out;
}
static std::string hex(const uint8_t* b, size_t n) {
  static const char digits[] = "0123456789abcdef";
  std::string out;
  for (size_t i = 0; i < n; ++i) out += digits[b[i] >> 4], out += digits[b[i] & 15];
  return out;
}
static std::vector<std::string> take_gate_calls() {
  std::lock_guard<std::mutex> lk(mock_gate::mu);
  std::vector<std::string> c;
  c.swap(mock_gate::calls);
  return c;
}
using Calls = std::vector<std::string>;

static OrchestratorNode node(const std::string& address, int k) {
  OrchestratorNode n;
  n.address = Address(address);
  n.status = NodeStatus::Healthy;
  n.p2p_id = "p2p-" + std::to_string(k);
  return n;
}
static std::shared_ptr<GpuMatchPlugin> make_plugin(bool book) {
  auto p = std::make_shared<GpuMatchPlugin>(std::vector<NodeGroupConfiguration>{{"solo", 1, 1, std::nullopt}}, 0,
                                            [](const Address&, const std::string&) { return size_t(3); },
                                            std::vector<std::shared_ptr<WebhookPlugin>>{});
  p->clock = [] { return int64_t(555); };
  if (book) p->enable_address_book();
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
static GpuMatchPlugin::GateRequest signed_by(int key, int m) { return {msg(m), "0x" + g_sig.at({key, msg(m)}), "0x" + g_addr.at(key)}; }

static void host_ecrecover_on_the_named_cases() {
  CHECK(g_cases.size() >= 25);
  int recovered = 0;
  for (const Case& c : g_cases) {
    const std::vector<uint8_t> h = unhex(c.hash), s = unhex(c.sig);
    uint8_t a[20];
    std::memset(a, 0xEE, sizeof a);
    const int32_t rc = pm_host_ecrecover(h.data(), s.data(), a);
    if (!((rc == PM_OK) == (c.ok == 1) && hex(a, 20) == c.address)) std::fprintf(stderr, "  case %s\n", c.name.c_str());
    CHECK((rc == PM_OK) == (c.ok == 1) && hex(a, 20) == c.address);
    CHECK(rc == PM_OK || rc == PM_EPARSE);
    recovered += rc == PM_OK;
  }
  CHECK(recovered >= 10 && recovered < int(g_cases.size()));
  uint8_t a[20];
  CHECK(pm_host_ecrecover(nullptr, nullptr, a) == PM_EINVAL);
}

static void the_signature_parser() {
  const std::string good = g_sig.at({0, msg(0)});
  uint8_t b[65], c[65];
  CHECK(GpuMatchPlugin::parse_signature_text(good, b) && hex(b, 65) == good);
  CHECK(GpuMatchPlugin::parse_signature_text("0x" + good, c) && std::memcmp(b, c, 65) == 0);
  std::string upper = good;
  for (char& ch : upper) ch = char(std::toupper(static_cast<unsigned char>(ch)));
  CHECK(GpuMatchPlugin::parse_signature_text(upper, c) && std::memcmp(b, c, 65) == 0);
  for (const std::string& bad : {std::string(), std::string("0x"), good.substr(0, 129), good + "0", "0X" + good, " " + good,
                                 good.substr(0, 10) + "g" + good.substr(11), "0x0x" + good.substr(2)})
    CHECK(!GpuMatchPlugin::parse_signature_text(bad, c));
}

static void the_eight_codes_and_their_precedence() {
  auto p = make_plugin(true);
  p->sync_nodes({node("0x" + g_addr.at(0), 0), node("0x" + g_addr.at(1), 1), node("0x" + g_addr.at(2), 2)});
  {
    std::lock_guard<std::mutex> lk(mock_gate::mu);
    mock_gate::status = {uint8_t(PM_NS_HEALTHY), uint8_t(PM_NS_EJECTED), uint8_t(PM_NS_BANNED)};
  }
  take_gate_calls();
  std::string no_key;
  for (const Case& c : g_cases)
    if (c.name == "r_no_x") no_key = c.sig;
  CHECK(!no_key.empty());
  GpuMatchPlugin::GateRequest bad_v = signed_by(0, 0);
  bad_v.signature.replace(bad_v.signature.size() - 2, 2, "1d");  // v = 29
  GpuMatchPlugin::GateRequest flagged = signed_by(0, 2);
  flagged.address = "0xnot-an-address";
  GpuMatchPlugin::GateRequest mismatch = signed_by(0, 3);
  mismatch.address = "0x" + g_addr.at(1);
  GpuMatchPlugin::GateRequest other_spelling = signed_by(0, 7);
  for (char& ch : other_spelling.address) ch = char(std::toupper(static_cast<unsigned char>(ch)));
  other_spelling.address[1] = 'x';
  GpuMatchPlugin::GateRequest flag_and_unknown = signed_by(3, 11);
  flag_and_unknown.address = "";
  const std::vector<GpuMatchPlugin::GateRequest> reqs = {
      bad_v,                                                 // 0 BAD_SIGNATURE (the engine's: v is no recovery id)
      {msg(1), no_key, "0x" + g_addr.at(0)},                 // 1 NO_KEY
      flagged,                                               // 2 BAD_ADDRESS
      mismatch,                                              // 3 MISMATCH
      signed_by(3, 4),                                       // 4 UNKNOWN
      signed_by(1, 5),                                       // 5 EJECTED
      signed_by(2, 6),                                       // 6 BANNED
      other_spelling,                                        // 7 OK (an upper-case x-address)
      {msg(8), no_key, "junk"},                              // 8 flag + no key: NO_KEY
      {msg(9), "0xnot-a-signature", "junk"},                 // 9 flag + a text that is no signature: BAD_SIGNATURE (the host's)
      {msg(10), g_sig.at({1, msg(10)}), "0x" + g_addr.at(0)},  // 10 an ejected node's signature under another address: MISMATCH
      flag_and_unknown};                                     // 11 flag + unknown signer: BAD_ADDRESS
  const GpuMatchPlugin::GateResult r = p->verify_requests(reqs);
  CHECK((take_gate_calls() == Calls{"verify n=12 flags=[0,0,1,0,0,0,0,0,1,1,0,1]"}));  // one engine call, the flags as parsed
  const uint32_t want[12] = {PM_RQ_BAD_SIGNATURE, PM_RQ_NO_KEY, PM_RQ_BAD_ADDRESS, PM_RQ_MISMATCH, PM_RQ_UNKNOWN, PM_RQ_EJECTED,
                             PM_RQ_BANNED,        PM_RQ_OK,     PM_RQ_NO_KEY,      PM_RQ_BAD_SIGNATURE, PM_RQ_MISMATCH, PM_RQ_BAD_ADDRESS};
  CHECK(r.verdicts.size() == 12);
  uint32_t census[PM_RQ_N_CODES] = {};
  for (size_t k = 0; k < r.verdicts.size() && k < 12; ++k) {
    if (r.verdicts[k].code != want[k]) std::fprintf(stderr, "  request %zu: code %u\n", k, r.verdicts[k].code);
    CHECK(r.verdicts[k].code == want[k]);
    census[want[k]]++;
  }
  for (uint32_t c = 0; c < PM_RQ_N_CODES; ++c) CHECK(r.counts[c] == census[c]);
  CHECK(r.verdicts[7].row == 0 && r.verdicts[7].status == PM_NS_HEALTHY && hex(r.verdicts[7].address.data(), 20) == g_addr.at(0));
  CHECK(r.verdicts[5].row == 1 && r.verdicts[5].status == PM_NS_EJECTED && r.verdicts[6].row == 2 && r.verdicts[6].status == PM_NS_BANNED);
  CHECK(r.verdicts[4].row == 0xFFFFFFFFu && r.verdicts[4].status == 0xFF && hex(r.verdicts[4].address.data(), 20) == g_addr.at(3));
  CHECK(r.verdicts[10].row == 1 && r.verdicts[3].row == 0);
  CHECK(r.verdicts[0].row == 0xFFFFFFFFu && hex(r.verdicts[0].address.data(), 20) == std::string(40, '0'));
  // nothing to verify: no engine call
  CHECK(p->verify_requests({}).verdicts.empty() && take_gate_calls().empty());
  // liveness off: the ejected and the banned node pass
  {
    std::lock_guard<std::mutex> lk(mock_gate::mu);
    mock_gate::status.clear();
  }
  const GpuMatchPlugin::GateResult off = p->verify_requests({signed_by(1, 5), signed_by(2, 6)});
  CHECK(off.verdicts[0].code == PM_RQ_OK && off.verdicts[1].code == PM_RQ_OK && off.verdicts[0].status == 0xFF && off.counts[PM_RQ_OK] == 2);
}

static void the_book_must_be_on() {
  auto p = make_plugin(false);
  p->sync_nodes({node("0x" + g_addr.at(0), 0)});
  take_gate_calls();
  CHECK(code_of([&] { p->verify_requests({signed_by(0, 0)}); }) == PM_ESTATE && take_gate_calls().empty());
}

static void the_c_face() {
  pmx_plugin* h = nullptr;
  const pmx_config cfgs[1] = {{"solo", 1, 1, nullptr}};
  CHECK(pmx_create(cfgs, 1, 0, &h) == 0 && h);
  if (!h) return;
  const std::string line = "0x" + g_sig.at({0, msg(0)}) + "\t0x" + g_addr.at(0) + "\t" + msg(0) + "\n" + "nonsense\t0x" + g_addr.at(0) + "\t" +
                           msg(1) + "\n";
  size_t need = 0;
  CHECK(pmx_verify_requests(h, line.c_str(), nullptr, 0, &need) != 0);  // the book is off
  CHECK(pmx_enable_address_book(h) == 0);
  h->plugin->sync_nodes({node("0x" + g_addr.at(0), 0)});
  CHECK(pmx_verify_requests(h, line.c_str(), nullptr, 0, &need) == 0 && need > 0);
  std::string text(need, '\0');
  CHECK(pmx_verify_requests(h, line.c_str(), text.data(), text.size(), &need) == 0);
  text.resize(need ? need - 1 : 0);
  const std::string want = "ok\t0\t-\t0x" + g_addr.at(0) + "\nbad_signature\t-\t-\t0x" + std::string(40, '0') + "\ncounts\t1\t0\t0\t0\t0\t0\t0\t1\n";
  if (text != want) std::fprintf(stderr, "  got:\n%s", text.c_str());
  CHECK(text == want);
  CHECK(pmx_verify_requests(h, "a line without tabs\n", text.data(), text.size(), &need) != 0);
  pmx_destroy(h);
}

int main(int argc, char** argv) {
  if (argc < 2) return std::fprintf(stderr, "usage: gate_test <cases>\n"), 2;
  std::ifstream in(argv[1]);
  for (std::string line; std::getline(in, line);) {
    std::istringstream is(line);
    std::string kind;
    is >> kind;
    if (kind == "case") {
      Case c;
      is >> c.name >> c.hash >> c.sig >> c.ok >> c.address;
      g_cases.push_back(c);
    } else if (kind == "signed") {
      int key;
      std::string addr, sig, m;
      is >> key >> addr >> sig >> m;
      g_addr[key] = addr;
      g_sig[{key, m}] = sig;
    }
  }
  struct {
    const char* name;
    void (*fn)();
  } tests[] = {{"host_ecrecover_on_the_named_cases", host_ecrecover_on_the_named_cases},
               {"the_signature_parser", the_signature_parser},
               {"the_eight_codes_and_their_precedence", the_eight_codes_and_their_precedence},
               {"the_book_must_be_on", the_book_must_be_on},
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
