// metrics_test.cpp — GpuMatchPlugin's metrics methods (protocol_amd/plugin/gpu_match_metrics.cpp) and their C face
// (pm_plugin_metrics_c.cpp) against tests/cpp/mock_engine.cpp + tests/cpp/mock_metrics.cpp: the interner (task id or "manual",
// the cleaned label, the keep-the-maximum flag from the original label), what is queued and what one flush sends, in which
// order; that every read flushes first; the roll-ups to label names; the reference's own tests through the plugin; the sync
// service's list; an engine refusal; writers racing a reader.
#include <cmath>
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

namespace mock_metrics {
extern std::mutex mu;
extern bool on;
extern uint32_t W, n_series;
extern int32_t fail_ingest_with;
extern std::map<uint32_t, std::map<uint32_t, double>> rows;
extern std::map<uint32_t, std::pair<uint64_t, uint32_t>> group_of_row;
extern std::vector<std::string> calls;
extern std::vector<pm_mx_beat> last_beats;
extern std::vector<pm_mx_entry> last_entries;
}  // namespace mock_metrics

using namespace orchestrator;
using Entry = GpuMatchPlugin::MetricEntry;

static int g_failed = 0;
#define CHECK(cond)                                                                      \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      std::fprintf(stderr, "  CHECK failed at %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                                        \
    }                                                                                    \
  } while (0)

static const int N = 6;
static const std::string ZERO = "0x0000000000000000000000000000000000000000";
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
  std::lock_guard<std::mutex> lk(mock_metrics::mu);
  mock_metrics::on = false;
  mock_metrics::W = uint32_t(N);
  mock_metrics::n_series = 0;
  mock_metrics::fail_ingest_with = PM_OK;
  mock_metrics::rows.clear(), mock_metrics::group_of_row.clear(), mock_metrics::calls.clear();
  mock_metrics::last_beats.clear(), mock_metrics::last_entries.clear();
  return p;
}
static std::vector<std::string> take_calls() {
  std::lock_guard<std::mutex> lk(mock_metrics::mu);
  std::vector<std::string> c;
  c.swap(mock_metrics::calls);
  return c;
}
static uint32_t row(const GpuMatchPlugin& p, int k) { return p.row_of(Address(addr(k))).value_or(PM_NONE); }

static void the_interner_the_queue_and_one_flush() {
  auto p = make_plugin();
  bool threw = false;
  p->beat_metrics(Address(addr(0)), {Entry{"t1", "loss", 1.0}});
  try {  // the ledger is off: the engine's PM_ESTATE, and the refused batch is dropped
    p->flush_metrics();
  } catch (const EngineError& x) {
    threw = x.code() == PM_ESTATE;
  }
  CHECK(threw && p->queued_metric_beats() == 0);
  p->enable_metrics();
  CHECK((take_calls() == std::vector<std::string>{"ingest beats=1 entries=1 series=1", "enable 1"}));
  // five writes queue without a call; an unknown address, an empty store and the delete of a field nobody stored queue nothing
  p->beat_metrics(Address(addr(2)), {Entry{"t1", "dashboard-progress", 5.0}, Entry{"t1", "dashboard:-progress", 2.0}, Entry{"", "a:b", 3.0}});
  p->store_metrics(Address(addr(1)), {Entry{"t2", "dashboard-progress/x", 1.0}});
  p->store_manual_metric("ab", 9.0);
  p->delete_metric("t1", "dashboard-:progress", Address(addr(2)));
  p->beat_metrics(Address(addr(3)), {});
  p->beat_metrics(Address("0x00000000000000000000000000000000000000ff"), {Entry{"t1", "loss", 1.0}});
  p->store_metrics(Address(addr(1)), {});
  p->delete_metric("t1", "never", Address(addr(1)));
  p->delete_metric("", "ab", Address::zero());  // (the key is ":ab" as given, metrics_store.rs:100: no such field)
  CHECK(p->queued_metric_beats() == 5 && take_calls().empty());
  p->flush_metrics();
  CHECK((take_calls() == std::vector<std::string>{"ingest beats=5 entries=6 series=3"}));
  CHECK(p->queued_metric_beats() == 0);
  p->flush_metrics();  // nothing queued: no call
  CHECK(take_calls().empty());
  {
    std::lock_guard<std::mutex> lk(mock_metrics::mu);
    const std::vector<pm_mx_beat>& b = mock_metrics::last_beats;
    const std::vector<pm_mx_entry>& e = mock_metrics::last_entries;
    CHECK(b.size() == 5 && e.size() == 6);
    // in call order: REPLACE row 2 (three entries), MERGE row 1, MERGE the manual row, DELETE row 2, REPLACE row 3 (empty)
    CHECK(b[0].row == row(*p, 2) && b[0].kind == PM_MXB_REPLACE && b[0].first == 0 && b[0].n == 3);
    CHECK(b[1].row == row(*p, 1) && b[1].kind == PM_MXB_MERGE && b[1].first == 3 && b[1].n == 1);
    CHECK(b[2].row == PM_MX_MANUAL && b[2].kind == PM_MXB_MERGE && b[2].first == 4 && b[2].n == 1);
    CHECK(b[3].row == row(*p, 2) && b[3].kind == PM_MXB_DELETE && b[3].first == 5 && b[3].n == 1);
    CHECK(b[4].row == row(*p, 3) && b[4].kind == PM_MXB_REPLACE && b[4].n == 0);
    // "t1:dashboard-progress" twice: one series, the flag from the ORIGINAL label; "manual:ab" from ("", "a:b") and the manual
    // route's "ab": one series; "t2:dashboard-progress/x": its own, MAX
    CHECK(e[0].series == 0 && e[0].flags == PM_MXF_MAX && e[1].series == 0 && e[1].flags == 0);
    CHECK(e[2].series == 1 && e[2].flags == 0 && e[4].series == 1 && e[4].value == 9.0);
    CHECK(e[3].series == 2 && e[3].flags == PM_MXF_MAX);
    CHECK(e[5].series == 0);  // delete_metric cleans its label too
  }
  // the reads flush first, each with one ingest in front of its own call
  p->store_manual_metric("uptime", 4.0);
  GpuMatchPlugin::MetricsByName all = p->aggregate_metrics_for_all_tasks();
  CHECK((take_calls() == std::vector<std::string>{"ingest beats=1 entries=1 series=4", "totals", "totals"}));
  CHECK((all == GpuMatchPlugin::MetricsByName{{"ab", 12.0}, {"dashboard-progress/x", 1.0}, {"uptime", 4.0}}));  // row 2's series 0 was deleted
  p->store_metrics(Address(addr(2)), {Entry{"t1", "loss", 0.5}});
  GpuMatchPlugin::MetricsByTask node2 = p->metrics_for_node(Address(addr(2)));
  CHECK((take_calls() == std::vector<std::string>{"ingest beats=1 entries=1 series=5", "rows n=1", "rows n=1"}));
  CHECK((node2 == GpuMatchPlugin::MetricsByTask{{"manual", {{"ab", 3.0}}}, {"t1", {{"loss", 0.5}}}}));
  CHECK(p->metrics_for_node(Address("0x00000000000000000000000000000000000000ff")).empty());
  CHECK((p->metrics_for_node(Address::zero()) == GpuMatchPlugin::MetricsByTask{{"manual", {{"ab", 9.0}, {"uptime", 4.0}}}}));
  // enabling again: an empty ledger, and the interner starts over
  p->enable_metrics();
  p->store_manual_metric("fresh", 1.0);
  take_calls();
  p->flush_metrics();
  CHECK((take_calls() == std::vector<std::string>{"ingest beats=1 entries=1 series=1"}));
}

static void the_roll_ups() {
  auto p = make_plugin();
  p->enable_metrics();
  // one label under two tasks and the manual key, on three nodes: the aggregate over all tasks adds the series up in
  // ascending series order, the one for a task takes that task's series only
  p->beat_metrics(Address(addr(0)), {Entry{"t1", "loss", 1.0}, Entry{"t2", "loss", 10.0}, Entry{"t1", "lr", 0.5}});
  p->beat_metrics(Address(addr(4)), {Entry{"t1", "loss", 2.0}, Entry{"", "loss", 100.0}});
  p->store_manual_metric("loss", 1000.0);
  CHECK((p->aggregate_metrics_for_all_tasks() == GpuMatchPlugin::MetricsByName{{"loss", 1113.0}, {"lr", 0.5}}));
  CHECK((p->aggregate_metrics_for_task("t1") == GpuMatchPlugin::MetricsByName{{"loss", 3.0}, {"lr", 0.5}}));
  CHECK((p->aggregate_metrics_for_task("t2") == GpuMatchPlugin::MetricsByName{{"loss", 10.0}}));
  CHECK((p->aggregate_metrics_for_task("manual") == GpuMatchPlugin::MetricsByName{{"loss", 1100.0}}));
  CHECK(p->aggregate_metrics_for_task("t3").empty());
  const auto all = p->all_metrics();
  CHECK(all.size() == 3 && all.at("t1").at("loss").size() == 2 && all.at("t1").at("loss").at(addr(4)) == 2.0);
  CHECK(all.at("manual").at("loss").at(ZERO) == 1000.0 && all.at("manual").at("loss").at(addr(4)) == 100.0);
  // a series whose last holder dropped it is in no aggregate (the reference's map has no such key)
  p->beat_metrics(Address(addr(0)), {Entry{"t1", "loss", 1.0}});
  CHECK((p->aggregate_metrics_for_all_tasks() == GpuMatchPlugin::MetricsByName{{"loss", 1103.0}}));
  p->clear_metrics(Address(addr(4)));
  CHECK((p->aggregate_metrics_for_task("t1") == GpuMatchPlugin::MetricsByName{{"loss", 1.0}}));
  CHECK(p->metrics_for_node(Address(addr(4))).empty());
}

// metrics_store.rs:251-446 and heartbeat.rs:195-377 (tests/golden/metrics_store_kats.json holds the same as data)
static void the_references_tests() {
  const Address other("0x1234567890123456789012345678901234567890");
  {  // test_store_metrics
    auto p = make_plugin();
    p->enable_metrics();
    p->store_metrics(Address::zero(), {Entry{"task_1", "cpu_usage", 1.0}});
    p->store_metrics(Address::zero(), {Entry{"task_0", "cpu_usage", 2.0}});
    CHECK(p->aggregate_metrics_for_task("task_1").at("cpu_usage") == 1.0);
    CHECK(p->aggregate_metrics_for_all_tasks().at("cpu_usage") == 3.0);
  }
  {  // test_get_metrics_for_node (the second address is node 1 here)
    auto p = make_plugin();
    p->enable_metrics();
    p->store_metrics(Address::zero(), {Entry{"task_1", "cpu_usage", 1.0}});
    p->store_metrics(Address(addr(1)), {Entry{"task_1", "cpu_usage", 1.0}});
    p->store_metrics(Address(addr(1)), {Entry{"task_2", "cpu_usage", 1.0}});
    const auto m0 = p->metrics_for_node(Address::zero()), m1 = p->metrics_for_node(Address(addr(1)));
    CHECK(m0.at("task_1").at("cpu_usage") == 1.0 && !m0.count("task_2"));
    CHECK(m1.at("task_1").at("cpu_usage") == 1.0 && m1.at("task_2").at("cpu_usage") == 1.0);
  }
  {  // test_store_metrics_value_overwrite
    auto p = make_plugin();
    p->enable_metrics();
    const std::string label = "dashboard-progress/test/value";
    p->store_metrics(Address::zero(), {Entry{"task_1", label, 2.0}});
    p->store_metrics(Address::zero(), {Entry{"task_1", label, 1.0}});
    CHECK(p->metrics_for_node(Address::zero()).at("task_1").at(label) == 2.0);
    p->store_metrics(Address::zero(), {Entry{"task_1", label, 3.0}});
    CHECK(p->metrics_for_node(Address::zero()).at("task_1").at(label) == 3.0);
    p->store_metrics(Address::zero(), {Entry{"task_1", "cpu_usage", 2.0}});
    p->store_metrics(Address::zero(), {Entry{"task_1", "cpu_usage", 1.0}});
    CHECK(p->metrics_for_node(Address::zero()).at("task_1").at("cpu_usage") == 1.0);
  }
  {  // test_heartbeat: three beats of one node
    auto p = make_plugin();
    p->enable_metrics();
    const Address a(addr(0));
    p->beat_metrics(a, {Entry{"long-task-1234", "performance/batch_avg_seq_length", 1.0},
                        Entry{"long-task-1234", "performance/batch_min_seq_length", 5.0}});
    auto m = p->metrics_for_node(a);
    CHECK(m.count("long-task-1234") && m["long-task-1234"].count("performance/batch_avg_seq_length") &&
          m["long-task-1234"].count("performance/batch_min_seq_length"));
    p->beat_metrics(a, {Entry{"long-task-1235", "performance/batch_len", 10.0}, Entry{"long-task-1235", "performance/batch_min_len", 50.0}});
    m = p->metrics_for_node(a);
    CHECK(m.count("long-task-1235") && m["long-task-1235"].count("performance/batch_len") &&
          m["long-task-1235"].count("performance/batch_min_len") && !m.count("long-task-1234"));
    const auto agg = p->aggregate_metrics_for_all_tasks();
    CHECK(agg.size() == 2 && agg.at("performance/batch_len") == 10.0 && agg.at("performance/batch_min_len") == 50.0 &&
          !agg.count("performance/batch_avg_seq_length"));
    p->beat_metrics(a, {});
    CHECK(p->metrics_for_node(a).empty() && p->aggregate_metrics_for_all_tasks().empty());
  }
}

static void the_sync_services_list_and_a_refusal() {
  auto p = make_plugin();
  p->enable_metrics();
  {
    std::lock_guard<std::mutex> lk(mock_metrics::mu);
    mock_metrics::group_of_row[row(*p, 1)] = {0xabcdef12345ull, 1u};
  }
  p->store_manual_metric("uptime", 1.5);
  p->beat_metrics(Address(addr(1)), {Entry{"t1", "loss", 0.25}});
  p->beat_metrics(Address(addr(0)), {Entry{"t9", "loss", -0.0}});
  const auto list = p->synced_metrics({{"t1", "first task"}});
  CHECK(list.size() == 3);
  if (list.size() == 3) {
    const size_t i0 = row(*p, 0) < row(*p, 1) ? 1 : 2, i1 = 3 - i0;  // (the manual row first, then ascending row)
    CHECK(list[0].address == ZERO && list[0].task_id == "manual" && list[0].task_name == "unknown" && list[0].label == "uptime" &&
          list[0].value == 1.5 && !list[0].group_id && !list[0].group_config_name);
    CHECK(list[i1].address == addr(1) && list[i1].task_name == "first task" && list[i1].value == 0.25 && list[i1].group_id &&
          *list[i1].group_id == "abcdef12345" && list[i1].group_config_name && *list[i1].group_config_name == "solo");
    CHECK(list[i0].address == addr(0) && list[i0].task_id == "t9" && list[i0].task_name == "unknown" && std::signbit(list[i0].value) &&
          !list[i0].group_id);
  }
  // a refused batch (the row bound, say) reaches the caller once and is not sent again
  {
    std::lock_guard<std::mutex> lk(mock_metrics::mu);
    mock_metrics::fail_ingest_with = PM_ERANGE;
  }
  p->store_manual_metric("uptime", 2.5);
  bool threw = false;
  try {
    p->aggregate_metrics_for_all_tasks();
  } catch (const EngineError& x) {
    threw = x.code() == PM_ERANGE;
  }
  CHECK(threw && p->queued_metric_beats() == 0);
  CHECK(p->aggregate_metrics_for_task("manual").at("uptime") == 1.5);
  // a configuration the plugin has not
  {
    std::lock_guard<std::mutex> lk(mock_metrics::mu);
    mock_metrics::group_of_row[row(*p, 1)] = {7ull, 2u};
  }
  threw = false;
  try {
    p->synced_metrics({});
  } catch (const std::out_of_range&) {
    threw = true;
  }
  CHECK(threw);
}

static std::string text_of(int32_t (*call)(pmx_plugin*, const char*, char*, size_t, size_t*), pmx_plugin* h, const char* arg) {
  size_t need = 0;
  CHECK(call(h, arg, nullptr, 0, &need) == 0 && need > 0);
  std::string buf(need, '\0');
  CHECK(call(h, arg, buf.data(), buf.size(), &need) == 0);
  buf.resize(need - 1);
  return buf;
}

static void the_c_face() {
  pmx_plugin h;
  h.plugin = make_plugin();
  CHECK(pmx_store_manual_metric(&h, "uptime", 1.0) == 0);
  CHECK(pmx_flush_metrics(&h) == -1 && std::string(pmx_last_error()).size() > 0);  // off
  CHECK(pmx_enable_metrics(&h) == 0 && mock_metrics::on);
  const std::string a0 = addr(0), a1 = addr(1);
  const char* tasks[2] = {"t1", ""};
  const char* labels[2] = {"dashboard-progress", "a:b"};
  const double values[2] = {0.1, -2.0};
  CHECK(pmx_beat_metrics(&h, a0.c_str(), tasks, labels, values, 2) == 0);
  CHECK(pmx_store_metrics(&h, a1.c_str(), tasks, labels, values, 1) == 0);
  CHECK(pmx_store_manual_metric(&h, "uptime", 8.0) == 0);
  CHECK(pmx_delete_metric(&h, "manual", "ab", a0.c_str()) == 0);
  take_calls();
  CHECK(pmx_flush_metrics(&h) == 0);
  CHECK((take_calls() == std::vector<std::string>{"ingest beats=4 entries=5 series=3"}));
  char tenth[64];
  std::snprintf(tenth, sizeof(tenth), "%a", 0.1 + 0.1);  // (0.0 + 0.1) + 0.1
  CHECK(text_of(pmx_aggregate_metrics, &h, nullptr) == std::string("dashboard-progress\t") + tenth + "\nuptime\t0x1p+3\n");
  CHECK(text_of(pmx_aggregate_metrics, &h, "manual") == "uptime\t0x1p+3\n");
  std::snprintf(tenth, sizeof(tenth), "%a", 0.1);
  CHECK(text_of(pmx_metrics_for_node, &h, a0.c_str()) == std::string("t1\tdashboard-progress\t") + tenth + "\n");
  CHECK(pmx_clear_metrics(&h, a0.c_str()) == 0);
  const char* ids[1] = {"t1"};
  const char* names[1] = {"the task"};
  size_t need = 0;
  CHECK(pmx_synced_metrics(&h, ids, names, 1, nullptr, 0, &need) == 0 && need > 0);
  std::string buf(need, '\0'), small(need - 1, '\0');
  size_t need2 = 0;
  CHECK(pmx_synced_metrics(&h, ids, names, 1, small.data(), small.size(), &need2) == -2 && need2 == need);
  CHECK(pmx_synced_metrics(&h, ids, names, 1, buf.data(), buf.size(), &need2) == 0);
  buf.resize(need - 1);
  CHECK(buf == ZERO + "\tmanual\tunknown\tuptime\t0x1p+3\t-\t-\n" + a1 + "\tt1\tthe task\tdashboard-progress\t" + tenth + "\t-\t-\n");
}

static void writers_race_a_reader() {
  auto p = make_plugin();
  p->enable_metrics();
  std::vector<std::thread> th;
  for (int t = 0; t < 4; ++t)
    th.emplace_back([&, t] {
      for (int k = 0; k < 300; ++k) {
        p->beat_metrics(Address(addr((t + k) % N)), {Entry{"t" + std::to_string(t), "dashboard-progress", double(k)}, Entry{"", "lr", 1.0}});
        if (k % 50 == 0) p->store_manual_metric("uptime", double(k));
      }
    });
  th.emplace_back([&] {
    for (int k = 0; k < 60; ++k) {
      p->aggregate_metrics_for_all_tasks();
      p->metrics_for_node(Address(addr(k % N)));
      p->synced_metrics({});
    }
  });
  for (auto& x : th) x.join();
  p->flush_metrics();
  CHECK(p->queued_metric_beats() == 0);
  // every node's last beat named two series: one task's progress, and the learning rate
  for (int k = 0; k < N; ++k) {
    const auto m = p->metrics_for_node(Address(addr(k)));
    CHECK(m.size() == 2 && m.count("manual") && m.at("manual").at("lr") == 1.0);
  }
  CHECK(p->aggregate_metrics_for_all_tasks().at("lr") == double(N));
}

int main() {
  the_interner_the_queue_and_one_flush();
  the_roll_ups();
  the_references_tests();
  the_sync_services_list_and_a_refusal();
  the_c_face();
  writers_race_a_reader();
  std::printf("6 tests, %d failed checks\n", g_failed);
  return g_failed ? 1 : 0;
}
