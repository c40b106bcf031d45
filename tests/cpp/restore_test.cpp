// restore_test.cpp — GpuMatchPlugin::restore_groups (protocol_amd/plugin/gpu_match_restore.cpp) against
// tests/cpp/mock_engine.cpp + tests/cpp/mock_adopt.cpp: what the plugin hands pm_adopt_groups (rows resolved from the
// address text, ids parsed from the "{:x}" text, the store's order kept, claimed tasks as positions in the task list), one
// report entry for every reason a group is dropped and one for a group_task that names no task, and the call window.
#include <cstdio>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "gpu_match_plugin.hpp"

namespace mock_adopt {
struct AdoptCall {
  std::vector<pm_group> groups;
  std::vector<uint32_t> members;
  uint64_t id_state = 0;
};
extern std::vector<AdoptCall> adopt_calls;
extern uint32_t match_calls;
extern uint64_t id_state_answer;
}  // namespace mock_adopt

using namespace orchestrator;

static int g_failed = 0;
#define CHECK(cond)                                                                      \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      std::fprintf(stderr, "  CHECK failed at %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                                        \
    }                                                                                    \
  } while (0)

static std::string addr(int k) {
  char s[48];
  std::snprintf(s, sizeof(s), "0x%040x", 0x100 + k * 7);
  return s;
}
static OrchestratorNode node(int k) {
  OrchestratorNode n;
  n.address = Address(addr(k));
  n.status = NodeStatus::Healthy;
  n.p2p_id = "p2p-" + std::to_string(k);
  ComputeSpecs cs;
  GpuSpecs g;
  g.count = 8;
  g.memory_mb = 80000;
  cs.gpu = g;
  n.compute_specs = cs;
  return n;
}
static Task task(int k, int64_t created) {
  Task t;
  char id[40];
  std::snprintf(id, sizeof(id), "00000000-0000-4000-8000-%012x", 0x1000 + k);
  t.id = id;
  t.name = "task-" + std::to_string(k);
  t.image = "image";
  t.created_at = created;
  return t;
}
static NodeGroup group(const std::string& id, const std::string& cfg, std::vector<int> nodes, int64_t created_at) {
  NodeGroup g;
  g.id = id;
  g.configuration_name = cfg;
  for (int k : nodes) g.nodes.push_back(addr(k));
  g.created_at = created_at;
  return g;
}

static std::unique_ptr<GpuMatchPlugin> make_plugin(bool sync_nodes = true, bool sync_tasks = true) {
  std::vector<NodeGroupConfiguration> cfgs = {{"pair", 2, 2, std::nullopt}, {"solo", 1, 1, std::nullopt}, {"quad", 1, 4, std::nullopt}};
  auto p = std::make_unique<GpuMatchPlugin>(cfgs, 0, nullptr);
  if (sync_nodes) {
    std::vector<OrchestratorNode> snap;
    for (int k = 0; k < 12; ++k) snap.push_back(node(k));
    p->sync_nodes(snap);
  }
  if (sync_tasks) p->sync_tasks({task(2, 300), task(1, 200), task(0, 100)});
  return p;
}

static void restores_what_the_store_holds() {
  auto p = make_plugin();
  mock_adopt::adopt_calls.clear();
  mock_adopt::match_calls = 0;
  const std::vector<NodeGroup> store = {
      group("ab12", "pair", {3, 1}, 1111),
      group("7", "solo", {5}, 2222),
      group("ffffffffffffffff", "quad", {0, 8, 9}, 3333),
  };
  std::unordered_map<std::string, std::string> tasks = {{"ab12", task(0, 100).id}, {"ffffffffffffffff", task(2, 300).id}};
  const GpuMatchPlugin::RestoreReport r = p->restore_groups(store, tasks, 0x1234567890abcdefull);
  CHECK(r.dropped.empty() && r.task_cleared.empty());
  CHECK(mock_adopt::adopt_calls.size() == 1);
  CHECK(mock_adopt::match_calls == 1);  // heartbeats are served right after
  if (mock_adopt::adopt_calls.size() != 1) return;
  const auto& c = mock_adopt::adopt_calls[0];
  CHECK(c.id_state == 0x1234567890abcdefull);
  CHECK(c.groups.size() == 3 && c.members.size() == 6);
  if (c.groups.size() != 3 || c.members.size() != 6) return;
  CHECK(c.groups[0].id == 0xab12 && c.groups[1].id == 7 && c.groups[2].id == 0xffffffffffffffffull);  // store order kept
  CHECK(c.groups[0].config == 0 && c.groups[1].config == 1 && c.groups[2].config == 2);
  CHECK(c.groups[0].task == 2 && c.groups[1].task == PM_NONE && c.groups[2].task == 0);  // positions in get_all_tasks order
  CHECK(c.groups[0].member_begin == 0 && c.groups[0].n_members == 2);
  CHECK(c.groups[1].member_begin == 2 && c.groups[1].n_members == 1);
  CHECK(c.groups[2].member_begin == 3 && c.groups[2].n_members == 3);
  // rows: the order the nodes first appeared in (node k is row k here), in the group's order
  const std::vector<uint32_t> want = {3, 1, 5, 0, 8, 9};
  CHECK(c.members == want);
  // created_at is the store's, not the plugin's clock
  p->clock = [] { return int64_t(99); };
  mock_adopt::id_state_answer = 42;
  CHECK(p->group_id_state() == 42);
  // the engine reports nothing from the mock's pm_get_groups (it holds no group): the stamps wait in the plugin
}

static void reports_every_dropped_group() {
  auto p = make_plugin();
  mock_adopt::adopt_calls.clear();
  const std::vector<NodeGroup> store = {
      group("a1", "pair", {0, 1}, 1),
      group("0a", "solo", {2}, 2),               // leading zero: no "{:x}" text
      group("A2", "solo", {2}, 3),               // upper case
      group("", "solo", {2}, 4),                 // empty
      group("12345678901234567", "solo", {2}, 5),  // 17 digits
      group("b1", "no-such", {2}, 6),            // unknown configuration
      group("b2", "solo", {2}, 7),
      group("b3", "solo", {1}, 8),               // node of an earlier group
      group("b4", "pair", {3, 3}, 9),            // one node twice
      group("b5", "quad", {4, 5, 6, 7, 9}, 10),  // more than max_group_size
      group("b6", "quad", {}, 11),               // no nodes
      group("a1", "solo", {10}, 12),             // the id of an earlier group
      group("b7", "pair", {3, 4}, 13),
  };
  NodeGroup unknown = group("b8", "solo", {11}, 14);
  unknown.nodes[0] = "0xnot-a-node";
  std::vector<NodeGroup> all = store;
  all.push_back(unknown);
  std::unordered_map<std::string, std::string> tasks = {{"b7", "00000000-0000-4000-8000-00000000ffff"}, {"b2", task(1, 200).id}};
  const GpuMatchPlugin::RestoreReport r = p->restore_groups(all, tasks, 5);
  const std::vector<std::pair<std::string, std::string>> want_ids = {
      {"0a", "the id is not"}, {"A2", "the id is not"}, {"", "the id is not"}, {"12345678901234567", "the id is not"},
      {"b1", "unknown configuration"}, {"b3", "already in an earlier group"}, {"b4", "already in an earlier group"},
      {"b5", "more than max_group_size"}, {"b6", "no nodes"}, {"a1", "the id of an earlier group"},
      {"b8", "not in the node table"}};
  CHECK(r.dropped.size() == want_ids.size());
  for (size_t i = 0; i < std::min(r.dropped.size(), want_ids.size()); ++i) {
    CHECK(r.dropped[i].first == want_ids[i].first);
    if (r.dropped[i].second.find(want_ids[i].second) == std::string::npos) {
      std::fprintf(stderr, "  dropped %zu: %s: %s\n", i, r.dropped[i].first.c_str(), r.dropped[i].second.c_str());
      ++g_failed;
    }
  }
  CHECK(r.task_cleared == std::vector<std::string>{"b7"});
  CHECK(mock_adopt::adopt_calls.size() == 1);
  if (mock_adopt::adopt_calls.size() != 1) return;
  const auto& c = mock_adopt::adopt_calls[0];
  CHECK(c.groups.size() == 3);
  if (c.groups.size() != 3) return;
  CHECK(c.groups[0].id == 0xa1 && c.groups[1].id == 0xb2 && c.groups[2].id == 0xb7);
  CHECK(c.groups[1].task == 1 && c.groups[2].task == PM_NONE);
  CHECK((c.members == std::vector<uint32_t>{0, 1, 2, 3, 4}));
}

static void refuses_outside_its_window() {
  auto expect_estate = [](GpuMatchPlugin& p) {
    try {
      p.restore_groups({}, {}, 1);
    } catch (const EngineError& e) {
      return e.code() == PM_ESTATE;
    }
    return false;
  };
  auto no_nodes = make_plugin(false, true);
  CHECK(expect_estate(*no_nodes));
  auto no_tasks = make_plugin(true, false);
  CHECK(expect_estate(*no_tasks));
  auto ticked = make_plugin();
  ticked->tick();
  CHECK(expect_estate(*ticked));
  // a multi-GPU pool needs the id state handed over
  auto multi = make_plugin();
  multi->multi_gpu = true;
  bool threw = false;
  try {
    multi->restore_groups({}, {}, std::nullopt);
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  CHECK(threw);
  // without one, a single pool draws an id state of its own
  auto single = make_plugin();
  mock_adopt::adopt_calls.clear();
  single->restore_groups({}, {}, std::nullopt);
  CHECK(mock_adopt::adopt_calls.size() == 1);
}

int main() {
  const std::pair<const char*, void (*)()> tests[] = {{"restores_what_the_store_holds", restores_what_the_store_holds},
                                                      {"reports_every_dropped_group", reports_every_dropped_group},
                                                      {"refuses_outside_its_window", refuses_outside_its_window}};
  int n = 0;
  for (const auto& t : tests) {
    const int before = g_failed;
    t.second();
    std::printf("%s  %s\n", g_failed == before ? "ok" : "FAIL", t.first);
    ++n;
  }
  std::printf("%d tests, %d failed checks\n", n, g_failed);
  return g_failed ? 1 : 0;
}
