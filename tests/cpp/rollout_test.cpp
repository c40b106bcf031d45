// rollout_test.cpp — GpuMatchPlugin's rollout methods (protocol_amd/plugin/gpu_match_rollout.cpp) and their C face
// (pm_plugin_rollout_c.cpp) against tests/cpp/mock_engine.cpp + tests/cpp/mock_rollout.cpp: update_node_task's match, the id of a
// reported text, what is queued and the one ingest a flush sends, that every read flushes first, the id -> text map and its
// pruning, nodes_per_task as the sync service renders it, an engine refusal, the C face, writers racing a reader.
#include <cstdio>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "gpu_match_plugin.hpp"
#include "pm_plugin_c.h"
#include "pm_plugin_c_internal.hpp"

namespace mock_rollout {
struct Group {
  uint64_t id;
  uint32_t config, task;
  std::vector<uint32_t> members;
};
extern std::mutex mu;
extern bool on;
extern uint32_t W;
extern int32_t fail_ingest_with;
extern std::map<uint32_t, std::pair<uint64_t, uint32_t>> rows;
extern std::vector<Group> groups;
extern std::vector<uint64_t> task_uids;
extern std::vector<std::string> calls;
extern std::vector<pm_ro_report> last_reports;
}  // namespace mock_rollout

using namespace orchestrator;
using Opt = std::optional<std::string>;

static int g_failed = 0;
#define CHECK(cond)                                                                      \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      std::fprintf(stderr, "  CHECK failed at %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                                        \
    }                                                                                    \
  } while (0)

static const int N = 6;
static const std::string T1 = "00000000-0000-0000-0000-0000000000a1", T2 = "11111111-2222-3333-0000-0000000000b2";
static std::string addr(int k) {
  char s[48];
  std::snprintf(s, sizeof(s), "0x%040x", 0x900 + k * 7);
  return s;
}
static std::shared_ptr<GpuMatchPlugin> make_plugin() {
  std::vector<NodeGroupConfiguration> cfgs = {{"pair", 2, 2, std::nullopt}, {"solo", 1, 1, std::nullopt}};
  auto p = std::make_shared<GpuMatchPlugin>(cfgs, 0, nullptr, std::vector<std::shared_ptr<WebhookPlugin>>{});
  std::vector<OrchestratorNode> snap;
  for (int k = 0; k < N; ++k) {
    OrchestratorNode n;
    n.address = Address(addr(k));
    n.status = NodeStatus::Healthy;
    n.p2p_id = "p2p-" + std::to_string(k);
    snap.push_back(n);
  }
  p->sync_nodes(snap);
  Task a, b;
  a.id = T1, a.name = "first", a.image = "img", a.created_at = 20;
  b.id = T2, b.name = "second", b.image = "img", b.created_at = 10;
  p->sync_tasks({a, b});
  std::lock_guard<std::mutex> lk(mock_rollout::mu);
  mock_rollout::on = false;
  mock_rollout::W = uint32_t(N);
  mock_rollout::fail_ingest_with = PM_OK;
  mock_rollout::rows.clear(), mock_rollout::groups.clear(), mock_rollout::calls.clear(), mock_rollout::last_reports.clear();
  mock_rollout::task_uids = {0xa1ull, 0xb2ull};
  return p;
}
static std::vector<std::string> take_calls() {
  std::lock_guard<std::mutex> lk(mock_rollout::mu);
  std::vector<std::string> c;
  c.swap(mock_rollout::calls);
  return c;
}
static uint32_t row(const GpuMatchPlugin& p, int k) { return p.row_of(Address(addr(k))).value_or(PM_NONE); }
static uint64_t fnv(const std::string& s) {
  uint64_t h = 0xCBF29CE484222325ull;
  for (unsigned char c : s) h = (h ^ c) * 0x100000001B3ull;
  return h;
}

static void the_id_of_a_reported_text() {
  CHECK(GpuMatchPlugin::reported_task_uid(T1) == 0xa1ull && GpuMatchPlugin::reported_task_uid(T2) == 0xb2ull);
  CHECK(GpuMatchPlugin::reported_task_uid("FFFFFFFF-FFFF-FFFF-FFFF-FFFFFFFFFFFF") == ~0ull);
  CHECK(GpuMatchPlugin::reported_task_uid("0123456789abcdef0123456789ABCDEF") == 0x0123456789ABCDEFull);  // 32 digits, no hyphens
  for (const std::string s : {"", "long-task-1234", "00000000-0000-0000-0000-0000000000a", "00000000_0000-0000-0000-0000000000a1",
                              "g0000000-0000-0000-0000-0000000000a1"})
    CHECK(GpuMatchPlugin::reported_task_uid(s) == fnv(s));
  CHECK(fnv("") == 0xCBF29CE484222325ull && fnv("a") == 0xAF63DC4C8601EC8Cull);  // the published FNV-1a vectors
}

static void the_match_the_queue_and_one_flush() {
  auto p = make_plugin();
  bool threw = false;
  p->report_task(Address(addr(0)), T1, std::string("RUNNING"));
  try {  // the ledger is off: the engine's PM_ESTATE, and the refused batch is dropped
    p->flush_rollout();
  } catch (const EngineError& x) {
    threw = x.code() == PM_ESTATE;
  }
  CHECK(threw && p->queued_task_reports() == 0);
  p->enable_rollout();
  CHECK((take_calls() == std::vector<std::string>{"ingest n=1", "enable 1"}));
  CHECK(p->remembered_task_texts() == 0);  // enable starts the texts over
  // update_node_task's match: both present set, anything else clears; an unknown address queues nothing
  p->report_task(Address(addr(0)), T1, std::string("RUNNING"));
  p->report_task(Address(addr(1)), T1, std::string("running"));       // TaskState::from: UNKNOWN
  p->report_task(Address(addr(2)), std::string("long-task-1234"), std::string("FAILED"));
  p->report_task(Address(addr(3)), T2, std::nullopt);                 // (Some, None): clears
  p->report_task(Address(addr(4)), std::nullopt, std::string("RUNNING"));
  p->report_task(Address(addr(5)), std::nullopt, std::nullopt);
  p->report_task(Address("0x00000000000000000000000000000000000000ff"), T1, std::string("RUNNING"));
  p->report_task(Address(addr(0)), T2, std::string("PULLING"));       // the same node again: both travel, in order
  CHECK(p->queued_task_reports() == 7 && take_calls().empty());
  p->flush_rollout();
  CHECK((take_calls() == std::vector<std::string>{"ingest n=7"}) && p->queued_task_reports() == 0);
  p->flush_rollout();  // nothing queued: no call
  CHECK(take_calls().empty());
  {
    std::lock_guard<std::mutex> lk(mock_rollout::mu);
    const std::vector<pm_ro_report>& r = mock_rollout::last_reports;
    CHECK(r.size() == 7);
    CHECK(r[0].worker == row(*p, 0) && r[0].state == PM_TS_RUNNING && r[0].uid == 0xa1ull);
    CHECK(r[1].worker == row(*p, 1) && r[1].state == PM_TS_UNKNOWN && r[1].uid == 0xa1ull);
    CHECK(r[2].worker == row(*p, 2) && r[2].state == PM_TS_FAILED && r[2].uid == fnv("long-task-1234"));
    for (int k = 3; k < 6; ++k) CHECK(r[size_t(k)].worker == row(*p, k) && r[size_t(k)].state == PM_TS_NONE);
    CHECK(r[6].worker == row(*p, 0) && r[6].state == PM_TS_PULLING && r[6].uid == 0xb2ull);
    CHECK(mock_rollout::rows.size() == 3 && mock_rollout::rows.at(row(*p, 0)).first == 0xb2ull);
  }
  const auto stored = p->reported_tasks({row(*p, 0), row(*p, 3)});
  CHECK((stored.first == std::vector<uint64_t>{0xb2ull, 0ull}) && (stored.second == std::vector<uint8_t>{PM_TS_PULLING, uint8_t(PM_TS_NONE)}));
  // every read flushes first, with one ingest in front of its own call
  p->report_task(Address(addr(3)), T1, std::string("RUNNING"));
  p->rollout_summary();
  CHECK((take_calls() == std::vector<std::string>{"ingest n=1", "summary"}));
  p->report_task(Address(addr(3)), T1, std::string("RUNNING"));
  p->task_rollout();
  CHECK((take_calls() == std::vector<std::string>{"ingest n=1", "tasks", "tasks"}));
  p->report_task(Address(addr(3)), T1, std::string("RUNNING"));
  p->group_rollout();
  CHECK((take_calls() == std::vector<std::string>{"ingest n=1", "groups", "groups"}));
  p->report_task(Address(addr(3)), T1, std::string("RUNNING"));
  p->rollout_nodes(1u << PM_RO_STRAY);
  CHECK((take_calls() == std::vector<std::string>{"ingest n=1", "workers mask=2", "workers mask=2"}));
  // an engine refusal: the batch is dropped, the error travels
  {
    std::lock_guard<std::mutex> lk(mock_rollout::mu);
    mock_rollout::fail_ingest_with = PM_ERANGE;
  }
  p->report_task(Address(addr(4)), T1, std::string("RUNNING"));
  threw = false;
  try {
    p->nodes_per_task();
  } catch (const EngineError& x) {
    threw = x.code() == PM_ERANGE;
  }
  CHECK(threw && p->queued_task_reports() == 0);
}

static void the_texts_and_nodes_per_task() {
  auto p = make_plugin();
  p->enable_rollout();
  {
    std::lock_guard<std::mutex> lk(mock_rollout::mu);
    mock_rollout::groups = {{0x77ull, 0u, 0u, {row(*p, 0), row(*p, 1)}}, {0x78ull, 1u, PM_NONE, {row(*p, 2)}}};
  }
  p->report_task(Address(addr(0)), T1, std::string("RUNNING"));
  p->report_task(Address(addr(1)), T1, std::string("RUNNING"));
  p->report_task(Address(addr(2)), std::string("long-task-1234"), std::string("RUNNING"));
  p->report_task(Address(addr(3)), std::string("long-task-1234"), std::string("FAILED"));
  p->report_task(Address(addr(4)), std::string("gone"), std::string("RUNNING"));
  p->report_task(Address(addr(5)), T2, std::string("PENDING"));
  CHECK(p->remembered_task_texts() == 4);  // every reported id
  std::vector<GpuMatchPlugin::NodesPerTask> npt = p->nodes_per_task();
  CHECK(p->remembered_task_texts() == 4);  // ... which keeps the ids it lists
  std::map<std::string, std::pair<std::string, uint32_t>> by_id;
  for (const auto& t : npt) by_id[t.task_id] = {t.task_name, t.count};
  CHECK((by_id == std::map<std::string, std::pair<std::string, uint32_t>>{
                      {T1, {"first", 2}}, {T2, {"second", 1}}, {"long-task-1234", {"unknown", 2}}, {"gone", {"unknown", 1}}}));
  const std::vector<GpuMatchPlugin::TaskRollout> tr = p->task_rollout();
  CHECK(tr.size() == 4);
  for (size_t k = 1; k < tr.size(); ++k) CHECK(tr[k - 1].row.uid < tr[k].row.uid);
  for (const auto& t : tr)
    if (t.task_id == T1) CHECK(t.row.task == 0 && t.row.groups == 1 && t.row.groups_converged == 1 && t.row.assigned == 2 && t.row.converged == 2);
  const std::vector<GpuMatchPlugin::GroupRollout> gr = p->group_rollout();
  CHECK(gr.size() == 1 && gr[0].group_id == "77" && gr[0].configuration_name == "pair" && gr[0].task_id == T1 &&
        gr[0].row.same[PM_TS_RUNNING] == 2);
  const pm_ro_summary s = p->rollout_summary();
  CHECK(s.by_class[PM_RO_CONVERGED] == 2 && s.by_class[PM_RO_STRAY] == 4 && s.groups_with_task == 1 && s.groups_converged == 1 &&
        s.distinct_uids == 4 && s.by_state[PM_TS_N] == 0);
  const std::vector<GpuMatchPlugin::NodeRollout> stray = p->rollout_nodes(1u << PM_RO_STRAY);
  CHECK(stray.size() == 4 && stray[0].address == addr(2) && stray[0].task_id == Opt("long-task-1234") && stray[0].state == PM_TS_RUNNING);
  CHECK(stray[3].address == addr(5) && stray[3].task_id == Opt(T2) && stray[3].cls == PM_RO_STRAY);
  // the node that reported "gone" clears: the id leaves the report, and its text goes with the next one
  p->report_task(Address(addr(4)), std::nullopt, std::nullopt);
  npt = p->nodes_per_task();
  CHECK(npt.size() == 3 && p->remembered_task_texts() == 3);
  const std::vector<GpuMatchPlugin::NodeRollout> idle = p->rollout_nodes(1u << PM_RO_IDLE);
  CHECK(idle.size() == 1 && idle[0].address == addr(4) && !idle[0].task_id && idle[0].state == PM_TS_NONE);
  bool threw = false;
  try {
    p->rollout_nodes(0u);
  } catch (const EngineError& x) {
    threw = x.code() == PM_EINVAL;
  }
  CHECK(threw);
}

static std::string text_of(int32_t (*call)(pmx_plugin*, char*, size_t, size_t*), pmx_plugin* h) {
  size_t need = 0;
  CHECK(call(h, nullptr, 0, &need) == 0 && need > 0);
  std::string buf(need, '\0');
  CHECK(call(h, buf.data(), buf.size(), &need) == 0);
  buf.resize(need - 1);
  return buf;
}

static void the_c_face() {
  pmx_plugin h;
  h.plugin = make_plugin();
  const std::string a0 = addr(0), a1 = addr(1), a2 = addr(2);
  CHECK(pmx_report_task(&h, a0.c_str(), T1.c_str(), "RUNNING") == 0);
  CHECK(pmx_flush_rollout(&h) == -1 && std::string(pmx_last_error()).size() > 0);  // off
  CHECK(pmx_enable_rollout(&h) == 0 && mock_rollout::on);
  {
    std::lock_guard<std::mutex> lk(mock_rollout::mu);
    mock_rollout::groups = {{0xabcull, 0u, 0u, {row(*h.plugin, 0), row(*h.plugin, 1)}}};
  }
  CHECK(pmx_report_task(&h, a0.c_str(), T1.c_str(), "RUNNING") == 0);
  CHECK(pmx_report_task(&h, a1.c_str(), T1.c_str(), "PULLING") == 0);
  CHECK(pmx_report_task(&h, a2.c_str(), "side-job", "RUNNING") == 0);
  CHECK(pmx_report_task(&h, a2.c_str(), nullptr, "RUNNING") == 0);
  CHECK(pmx_report_task(&h, a2.c_str(), "side-job", "COMPLETED") == 0);
  take_calls();
  CHECK(pmx_flush_rollout(&h) == 0);
  CHECK((take_calls() == std::vector<std::string>{"ingest n=5"}));
  CHECK(text_of(pmx_nodes_per_task, &h) == (fnv("side-job") < 0xa1ull ? "side-job\tunknown\t1\n" + T1 + "\tfirst\t2\n"
                                                                      : T1 + "\tfirst\t2\nside-job\tunknown\t1\n"));
  const std::string tasks = text_of(pmx_task_rollout, &h);
  CHECK(tasks.find(T1 + "\tfirst\t0\t1\t0\t2\t1\t0\t1\t1\t0\t0\t0\t0\t0\n") != std::string::npos);
  CHECK(tasks.find("side-job\tunknown\t-\t0\t0\t0\t0\t0\t0\t0\t1\t0\t0\t0\t0\n") != std::string::npos);
  CHECK(text_of(pmx_group_rollout, &h) == "abc\tpair\t" + T1 + "\t2\t0\t1\t1\t0\t0\t0\t0\t0\t0\t0\n");
  pm_ro_summary s{};
  CHECK(pmx_rollout_summary(&h, &s) == 0 && s.by_class[PM_RO_CONVERGED] == 1 && s.by_class[PM_RO_BEHIND] == 1 &&
        s.by_class[PM_RO_STRAY] == 1 && s.by_class[PM_RO_IDLE] == 3);
  CHECK(pmx_rollout_summary(&h, nullptr) == -1);
  size_t need = 0;
  CHECK(pmx_rollout_nodes(&h, 1u << PM_RO_STRAY, nullptr, 0, &need) == 0 && need > 0);
  std::string buf(need, '\0'), small(need - 1, '\0');
  size_t need2 = 0;
  CHECK(pmx_rollout_nodes(&h, 1u << PM_RO_STRAY, small.data(), small.size(), &need2) == -2 && need2 == need);
  CHECK(pmx_rollout_nodes(&h, 1u << PM_RO_STRAY, buf.data(), buf.size(), &need2) == 0);
  buf.resize(need - 1);
  CHECK(buf == a2 + "\t1\t3\tside-job\n");
  CHECK(pmx_rollout_nodes(&h, 0u, nullptr, 0, &need) == -1);
}

static void writers_race_a_reader() {
  auto p = make_plugin();
  p->enable_rollout();
  std::vector<std::thread> th;
  for (int t = 0; t < 4; ++t)
    th.emplace_back([&, t] {
      for (int k = 0; k < 300; ++k) {
        if (k % 7 == 3) p->report_task(Address(addr((t + k) % N)), std::nullopt, std::nullopt);
        else p->report_task(Address(addr((t + k) % N)), "job-" + std::to_string(t), std::string(k % 2 ? "RUNNING" : "PULLING"));
      }
      p->report_task(Address(addr(t)), T1, std::string("RUNNING"));  // (each writer's last word on its own node)
    });
  th.emplace_back([&] {
    for (int k = 0; k < 60; ++k) {
      p->nodes_per_task();
      p->rollout_summary();
      p->group_rollout();
      p->rollout_nodes((1u << PM_RO_N) - 1u);
    }
  });
  for (auto& x : th) x.join();
  p->flush_rollout();
  CHECK(p->queued_task_reports() == 0);
  uint32_t total = 0;
  for (const auto& t : p->nodes_per_task()) total += t.count;
  CHECK(total >= 1 && total <= uint32_t(N));  // (every node's last word is a report or a clear; writer 3's last is a report)
  CHECK(p->remembered_task_texts() <= 4);
}

int main() {
  the_id_of_a_reported_text();
  the_match_the_queue_and_one_flush();
  the_texts_and_nodes_per_task();
  the_c_face();
  writers_race_a_reader();
  std::printf("5 tests, %d failed checks\n", g_failed);
  return g_failed ? 1 : 0;
}
