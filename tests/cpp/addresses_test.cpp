// addresses_test.cpp — GpuMatchPlugin with the address book on (protocol_amd/plugin/gpu_match_addresses.cpp, the book's part of
// sync_nodes in gpu_match_plugin.cpp) and its C face (pm_plugin_addresses_c.cpp) against tests/cpp/mock_engine.cpp +
// mock_addresses.cpp + mock_directory.cpp: the parser and its errors, what sync_nodes sends (only the new rows' bytes, one rank per
// interval that appended, the new rows' texts once), the rendered texts and the look-up by any spelling, the invite digests, the
// stale-table resend, and that on digit-only addresses the book changes nothing a caller can see.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <sstream>
#include <string>
#include <vector>

#include "gpu_match_plugin.hpp"
#include "pm_plugin_c.h"
#include "pm_plugin_c_internal.hpp"

extern "C" const char* pm_mock_calls(void);
extern "C" void pm_mock_reset_calls(void);
extern "C" void pm_mock_fail_appends(int n);

namespace mock_addresses {
extern std::mutex mu;
extern bool on;
extern std::vector<std::string> calls;
}  // namespace mock_addresses
namespace mock_directory {
extern std::mutex mu;
extern bool on;
extern std::vector<pm_dir_row> rows;
extern std::vector<uint32_t> ranks;
}  // namespace mock_directory

using namespace orchestrator;

static int g_failed = 0;
#define CHECK(cond)                                                                      \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      std::fprintf(stderr, "  CHECK failed at %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                                        \
    }                                                                                    \
  } while (0)

static std::vector<std::string> engine_calls(const std::string& name) {
  std::vector<std::string> out;
  std::istringstream is(pm_mock_calls());
  for (std::string line; std::getline(is, line);)
    if (line.compare(0, name.size() + 1, name + " ") == 0 || line == name) out.push_back(line);
  return out;
}
static std::vector<std::string> take_book_calls() {
  std::lock_guard<std::mutex> lk(mock_addresses::mu);
  std::vector<std::string> c;
  c.swap(mock_addresses::calls);
  return c;
}
using Calls = std::vector<std::string>;

// the EIP-55 vectors; as byte strings "0x5a.." < "0xD1.." < "0xdb.." < "0xfB..", lower-cased "0x5a.." < "0xd1.." < "0xdb.." < "0xfb.."
static const char* const KAT[4] = {"0x5aAeb6053F3E94C9b9A09f33669435E7Ef1BeAed", "0xfB6916095ca1df60bB79Ce92cE3Ea74c37c5d359",
                                   "0xdbF03B407c01E7cD3CBea99509d93f8DDDC8C6FB", "0xD1220A0cf47c7B9Be7A2E6BA89F429762e7b9aDb"};
static std::string lower(std::string s) {
  std::transform(s.begin(), s.end(), s.begin(), [](unsigned char c) { return char(c >= 'A' && c <= 'F' ? c + 32 : c); });
  return s;
}
static std::string digits(int k) {  // a digit-only address: every order agrees on these
  char s[48];
  std::snprintf(s, sizeof(s), "0x%040d", 1000 + ((k * 37) % 101));
  return s;
}
static OrchestratorNode node(const std::string& address, int k, NodeStatus st = NodeStatus::Healthy) {
  OrchestratorNode n;
  n.address = Address(address);
  n.status = st;
  n.p2p_id = "p2p-" + std::to_string(k);
  return n;
}
static std::vector<NodeGroupConfiguration> two_configs() { return {{"pair", 2, 2, std::nullopt}, {"solo", 1, 1, std::nullopt}}; }
static std::shared_ptr<GpuMatchPlugin> make_plugin(bool book) {
  auto p = std::make_shared<GpuMatchPlugin>(two_configs(), 0, [](const Address&, const std::string&) { return size_t(3); },
                                            std::vector<std::shared_ptr<WebhookPlugin>>{});
  p->clock = [] { return int64_t(555); };
  if (book) p->enable_address_book();
  return p;
}
static Task pair_task() {
  Task t;
  t.id = "00000000-0000-4000-8000-000000001001";
  t.name = "task-1";
  t.image = "image";
  t.created_at = 100;
  t.allowed_topologies = std::vector<std::string>{"pair"};
  t.env_vars = std::map<std::string, std::string>{{"IDX", "${GROUP_INDEX}/${GROUP_SIZE}"}, {"NEXT", "${NEXT_P2P_ADDRESS}"}};
  return t;
}
static int32_t code_of(const std::function<void()>& f, std::string* what = nullptr) {
  try {
    f();
  } catch (const EngineError& e) {
    if (what) *what = e.what();
    return e.code();
  }
  return 0;
}

static void the_parser_and_its_errors() {
  uint8_t b[20], c[20];
  CHECK(GpuMatchPlugin::parse_address_text(KAT[0], b) && b[0] == 0x5a && b[1] == 0xae && b[19] == 0xed);
  CHECK(GpuMatchPlugin::parse_address_text(lower(KAT[0]).substr(2), c) && std::memcmp(b, c, 20) == 0);  // no "0x", lower case
  std::string upper = KAT[0];
  std::transform(upper.begin() + 2, upper.end(), upper.begin() + 2, [](unsigned char ch) { return char(std::toupper(ch)); });
  CHECK(GpuMatchPlugin::parse_address_text(upper, c) && std::memcmp(b, c, 20) == 0);
  const std::string good = KAT[1];
  for (const std::string& bad : {std::string(), std::string("0x"), good.substr(0, 41), good + "0", "0X" + good.substr(2), " " + good,
                                 good.substr(0, 10) + "g" + good.substr(11), good.substr(2) + "\n", "0x0x" + good.substr(6)})
    CHECK(!GpuMatchPlugin::parse_address_text(bad, c));
  // a snapshot with a text that is no address: PM_EINVAL naming it, and nothing has changed
  auto p = make_plugin(true);
  p->sync_nodes({node(KAT[0], 0)});
  take_book_calls();
  pm_mock_reset_calls();
  std::string what;
  CHECK(code_of([&] { p->sync_nodes({node(KAT[0], 0), node(KAT[1], 1), node("0xnot-an-address", 2)}); }, &what) == PM_EINVAL);
  CHECK(what.find("'0xnot-an-address'") != std::string::npos);
  CHECK(p->known_nodes() == 1 && take_book_calls().empty() && engine_calls("append_workers").empty());
  // ... nor may a known address come back under another spelling
  CHECK(code_of([&] { p->sync_nodes({node(KAT[0], 0), node(lower(KAT[0]), 3)}); }, &what) == PM_EINVAL);
  CHECK(what.find("another spelling") != std::string::npos && p->known_nodes() == 1);
  CHECK(code_of([&] { p->sync_nodes({node(KAT[0], 0), node(KAT[2], 1), node(lower(KAT[2]), 2)}); }, &what) == PM_EINVAL && p->known_nodes() == 1);
  p->sync_nodes({node(KAT[0], 0), node(KAT[1], 1), node(KAT[1], 1)});  // (the same text twice: one row)
  CHECK(p->known_nodes() == 2);
  // enabling over rows that do not parse: refused, the book stays off
  auto q = make_plugin(false);
  q->sync_nodes({node("0x12", 0)});
  CHECK(code_of([&] { q->enable_address_book(); }, &what) == PM_EINVAL && !q->address_book_enabled());
}

static void what_sync_nodes_sends() {
  pm_mock_reset_calls();
  take_book_calls();
  auto p = make_plugin(true);
  CHECK((take_book_calls() == Calls{"enable 1"}));
  p->sync_nodes({node(lower(KAT[0]), 0), node(lower(KAT[1]), 1), node(lower(KAT[2]), 2)});
  CHECK((take_book_calls() == Calls{"set first=0 n=3", "rank", "text rows=[0,1,2]"}));
  // the rank went in through the engine's column: texts 5a.. < db.. < fB..
  CHECK((engine_calls("set_addr_ranks") == Calls{"set_addr_ranks [0,2,1]"}));
  pm_mock_reset_calls();
  p->sync_nodes({node(lower(KAT[0]), 0), node(lower(KAT[1]), 1), node(lower(KAT[2]), 2)});  // nothing new: no book call at all
  CHECK(take_book_calls().empty() && engine_calls("set_addr_ranks").empty());
  p->sync_nodes({node(lower(KAT[0]), 0), node(lower(KAT[1]), 1), node(lower(KAT[2]), 2), node(lower(KAT[3]), 3)});
  CHECK((take_book_calls() == Calls{"set first=3 n=1", "rank", "text rows=[3]"}));  // only the new row travels, one rank, one text
  CHECK((engine_calls("set_addr_ranks") == Calls{"set_addr_ranks [0,3,2,1]"}));      // "0x5a.." < "0xD1.." < "0xdb.." < "0xfB.."
  // a rewritten row goes with the rank it has
  pm_mock_reset_calls();
  p->sync_nodes({node(lower(KAT[0]), 0), node(lower(KAT[1]), 1, NodeStatus::Unhealthy), node(lower(KAT[2]), 2), node(lower(KAT[3]), 3)});
  CHECK(take_book_calls().empty());
  const Calls upd = engine_calls("update_workers");
  CHECK(upd.size() == 1 && upd[0].find("idx=[1]") != std::string::npos && upd[0].find("ranks=[3]") != std::string::npos);
  // a failed append: the next interval sends every row again, keeps the groups, and the book gets every row's bytes
  pm_mock_reset_calls();
  pm_mock_fail_appends(1);
  const std::string extra = "0x00000000000000000000000000000000000000aa";
  std::vector<OrchestratorNode> five = {node(lower(KAT[0]), 0), node(lower(KAT[1]), 1, NodeStatus::Unhealthy), node(lower(KAT[2]), 2),
                                        node(lower(KAT[3]), 3), node(extra, 4)};
  CHECK(code_of([&] { p->sync_nodes(five); }) != 0 && take_book_calls().empty());
  p->sync_nodes(five);
  CHECK((take_book_calls() == Calls{"set first=0 n=5", "rank", "text rows=[4]"}));
  CHECK((engine_calls("upload_workers") == Calls{"upload_workers n=5 keep=1"}));
  CHECK((engine_calls("set_addr_ranks") == Calls{"set_addr_ranks [1,4,3,2,0]"}));
}

static void the_rendered_texts_and_the_look_up() {
  auto p = make_plugin(true);
  p->sync_nodes({node(lower(KAT[0]), 0), node(lower(KAT[1]).substr(2), 1), node(lower(KAT[2]), 2)});  // (one without "0x")
  p->sync_tasks({pair_task()});
  CHECK(p->tick().n_formed == 1u);  // the toy engine pairs rows 0 and 1
  take_book_calls();
  const std::vector<NodeGroup> groups = p->get_all_groups();
  CHECK(groups.size() == 1 && (groups[0].nodes == std::vector<std::string>{KAT[0], KAT[1]}));  // the device's texts, in text order
  for (const std::string& spelling : {std::string(KAT[1]), lower(KAT[1]), lower(KAT[1]).substr(2)}) {
    const std::optional<NodeGroup> g = p->get_node_group(spelling);
    CHECK(g && g->id == groups[0].id && p->get_idx_in_group(*g, spelling) == 1);
  }
  CHECK(!p->get_node_group(KAT[2]) && !p->get_node_group("0xnonsense") && !p->get_node_group(KAT[3]));
  const auto map = p->get_all_node_group_mappings();
  CHECK(map.size() == 2 && map.count(KAT[0]) && map.count(KAT[1]));
  const std::vector<Task> got = p->filter_tasks({}, Address(lower(KAT[1]).substr(2)));  // (the heartbeat's key is the store's)
  CHECK(got.size() == 1 && got[0].env_vars->at("IDX") == "1/2" && got[0].env_vars->at("NEXT") == "p2p-0");
  // the shown text is a key beside the store's spelling: what was read from the plugin can be handed back to it
  CHECK(p->row_of(Address(KAT[1])) == std::optional<uint32_t>(1u) && p->row_of(Address(lower(KAT[1]).substr(2))) == std::optional<uint32_t>(1u));
  CHECK(p->filter_tasks({}, Address(KAT[0])).size() == 1 && !p->row_of(Address(lower(KAT[1]))));
  CHECK(take_book_calls().empty());  // all from the cache: no text is fetched twice
}

static void the_invite_digests() {
  auto p = make_plugin(true);
  p->sync_nodes({node(lower(KAT[0]), 0, NodeStatus::Discovered), node(lower(KAT[1]), 1), node(lower(KAT[2]), 2, NodeStatus::Discovered)});
  {
    std::lock_guard<std::mutex> lk(mock_directory::mu);
    mock_directory::on = true;
    mock_directory::rows.assign(3, pm_dir_row{});
    mock_directory::ranks.assign(3, 0u);
    const uint8_t st[3] = {PM_NS_DISCOVERED, PM_NS_HEALTHY, PM_NS_DISCOVERED};
    for (uint32_t w = 0; w < 3; ++w) {
      pm_dir_row& r = mock_directory::rows[w];
      r.worker = w, r.status = st[w], r.cls = st[w] == PM_NS_HEALTHY ? PM_DC_HEALTHY : PM_DC_DISCOVERED;
      r.state = uint8_t(PM_TS_NONE), r.group_slot = PM_NONE, r.group_id = PM_NONE, r.task = PM_NONE;
    }
  }
  CHECK((p->uninvited_nodes() == std::vector<std::string>{KAT[0], KAT[2]}));
  take_book_calls();
  uint8_t next = 0;
  const auto nonce = [&] {
    std::array<uint8_t, 32> n{};
    for (auto& b : n) b = next++;
    return n;
  };
  const std::vector<GpuMatchPlugin::InviteDigest> d = p->invite_digests(7u, 0x01020304u, nonce, 1700000000ull);
  CHECK((take_book_calls() == Calls{"invite n=2"}));
  CHECK(d.size() == 2 && d[0].address == KAT[0] && d[1].address == KAT[2] && d[0].nonce[31] == 31 && d[1].nonce[0] == 32);
  for (size_t k = 0; k < d.size(); ++k) {
    uint8_t msg[148] = {}, want[32], signed_msg[60], want_signing[32], addr[20];
    msg[31] = 7, msg[60] = 1, msg[61] = 2, msg[62] = 3, msg[63] = 4;
    CHECK(GpuMatchPlugin::parse_address_text(d[k].address, addr));
    std::memcpy(msg + 64, addr, 20);
    std::memcpy(msg + 84, d[k].nonce.data(), 32);
    const uint64_t exp = 1700000000ull;
    for (int j = 0; j < 8; ++j) msg[140 + j] = uint8_t(exp >> (8 * (7 - j)));
    pm_host_keccak256(msg, sizeof(msg), want);
    std::memcpy(signed_msg, "\x19" "Ethereum Signed Message:\n32", 28);
    std::memcpy(signed_msg + 28, want, 32);
    pm_host_keccak256(signed_msg, sizeof(signed_msg), want_signing);
    CHECK(std::memcmp(want, d[k].digest.data(), 32) == 0 && std::memcmp(want_signing, d[k].signing_hash.data(), 32) == 0);
  }
  // off: refused
  auto q = make_plugin(false);
  q->sync_nodes({node(lower(KAT[0]), 0, NodeStatus::Discovered)});
  CHECK(code_of([&] { (void)q->invite_digests(1u, 1u, nonce, 1ull); }) == PM_ESTATE);
}

static void digit_only_addresses_read_the_same_with_the_book_on() {
  std::vector<OrchestratorNode> snap;
  for (int k = 0; k < 9; ++k) snap.push_back(node(digits(k), k, k == 4 ? NodeStatus::Unhealthy : NodeStatus::Healthy));
  std::vector<std::string> shown[2];
  for (int book = 0; book < 2; ++book) {
    auto p = make_plugin(book != 0);
    p->sync_nodes(std::vector<OrchestratorNode>(snap.begin(), snap.begin() + 6));
    p->sync_tasks({pair_task()});
    p->tick();
    p->sync_nodes(snap);  // three more rows: the ranks of the standing groups' members move
    p->tick();
    std::vector<std::string>& out = shown[book];
    for (const NodeGroup& g : p->get_all_groups()) {
      std::string line = g.id + " " + g.configuration_name;
      for (const std::string& n : g.nodes) line += " " + n + "#" + std::to_string(p->get_idx_in_group(g, n));
      out.push_back(line);
    }
    for (int k = 0; k < 9; ++k) {
      const std::vector<Task> t = p->filter_tasks({}, Address(digits(k)));
      out.push_back(digits(k) + " -> " + (t.empty() ? std::string("-") : t[0].env_vars->at("IDX") + " " + t[0].env_vars->at("NEXT")));
    }
    CHECK(out.size() > 9);
  }
  CHECK(shown[0] == shown[1]);
  // enabling late, over rows the engine has: every row's bytes, one rank, every text
  auto p = make_plugin(false);
  p->sync_nodes(snap);
  take_book_calls();
  p->enable_address_book();
  CHECK((take_book_calls() == Calls{"enable 1", "set first=0 n=9", "rank", "text rows=[0,1,2,3,4,5,6,7,8]"}));
  CHECK(p->address_book_enabled() && p->get_node_group(digits(0)) == std::nullopt);
}

static void the_c_face() {
  pmx_plugin* h = nullptr;
  const pmx_config cfgs[2] = {{"pair", 2, 2, nullptr}, {"solo", 1, 1, nullptr}};
  CHECK(pmx_create(cfgs, 2, 0, &h) == 0 && h);
  if (!h) return;
  CHECK(pmx_enable_address_book(h) == 0);
  h->plugin->sync_nodes({node(lower(KAT[3]), 0, NodeStatus::Discovered)});
  {
    std::lock_guard<std::mutex> lk(mock_directory::mu);
    mock_directory::on = true;
    mock_directory::rows.assign(1, pm_dir_row{});
    mock_directory::ranks.assign(1, 0u);
    pm_dir_row& r = mock_directory::rows[0];
    r.status = PM_NS_DISCOVERED, r.cls = PM_DC_DISCOVERED, r.state = uint8_t(PM_TS_NONE), r.group_slot = PM_NONE, r.group_id = PM_NONE, r.task = PM_NONE;
  }
  size_t need = 0;
  CHECK(pmx_invite_digests(h, 1u, 2u, 99ull, 3ull, nullptr, 0, &need) == 0 && need == 42 + 3 * 65 + 1 + 1);
  std::string text(need, '\0');
  CHECK(pmx_invite_digests(h, 1u, 2u, 99ull, 3ull, text.data(), text.size(), &need) == 0);
  CHECK(text.compare(0, 43, std::string(KAT[3]) + "\t") == 0 && text[need - 2] == '\n');
  std::string again(need, '\0');
  CHECK(pmx_invite_digests(h, 1u, 2u, 99ull, 3ull, again.data(), again.size(), &need) == 0 && again == text);  // the seed decides
  CHECK(pmx_invite_digests(h, 1u, 2u, 98ull, 3ull, again.data(), again.size(), &need) == 0 && again != text);
  pmx_destroy(h);
}

int main() {
  struct {
    const char* name;
    void (*fn)();
  } tests[] = {{"the_parser_and_its_errors", the_parser_and_its_errors},
               {"what_sync_nodes_sends", what_sync_nodes_sends},
               {"the_rendered_texts_and_the_look_up", the_rendered_texts_and_the_look_up},
               {"the_invite_digests", the_invite_digests},
               {"digit_only_addresses_read_the_same_with_the_book_on", digit_only_addresses_read_the_same_with_the_book_on},
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
