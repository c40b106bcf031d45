// gpu_match_metrics.cpp — GpuMatchPlugin::enable_metrics / beat_metrics / store_metrics / store_manual_metric / delete_metric /
// clear_metrics / flush_metrics and the reads over them (see gpu_match_plugin.hpp): the engine's metrics ledger (pm_metrics_*)
// by node address, task id and label.  The twin of the same methods of rust/gpu_match_plugin.rs, statement for statement.  (A
// file of its own: the plugin's other methods are also linked against a mock engine that has not these exports.)
#include <algorithm>
#include <shared_mutex>
#include <stdexcept>

#include "group_id_text.hpp"
#include "gpu_match_plugin.hpp"

namespace orchestrator {

namespace {
std::string clean_label(const std::string& label) {  // metrics_store.rs:21-23
  std::string out;
  for (char c : label)
    if (c != ':') out += c;
  return out;
}
}  // namespace

void GpuMatchPlugin::enable_metrics() {
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);  // (LOCK ORDER: nodes, metrics, the engine)
  std::lock_guard<std::mutex> lk(metrics_mu_);
  check(pm_metrics_enable(engine_, 1u));
  metrics_ = MetricsQueue{};
}

// the series of "{task_id or "manual"}:{label without ':'}" (metrics_store.rs:43-49); a field seen for the first time gets the next
uint32_t GpuMatchPlugin::metric_series_locked(const std::string& task_id, const std::string& label) {
  const std::string task = task_id.empty() ? "manual" : task_id;
  const std::string cleaned = clean_label(label);
  const auto ins = metrics_.series.emplace(task + ":" + cleaned, uint32_t(metrics_.keys.size()));
  if (ins.second) metrics_.keys.emplace_back(task, cleaned);
  return ins.first->second;
}

void GpuMatchPlugin::queue_metrics(const Address& address, uint32_t kind, const std::vector<MetricEntry>& entries) {
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);
  uint32_t row = PM_MX_MANUAL;
  if (address != Address::zero()) {
    const auto it = nodes_.index.find(address);
    if (it == nodes_.index.end()) return;
    row = it->second;
  }
  std::lock_guard<std::mutex> lk(metrics_mu_);
  metrics_.beats.push_back(pm_mx_beat{row, kind, uint32_t(metrics_.entries.size()), uint32_t(entries.size())});
  for (const MetricEntry& e : entries) {
    // the rule is the ORIGINAL label's (metrics_store.rs:52): "dashboard:-progress" shares a series with "dashboard-progress"
    // and sets where that one keeps the maximum
    const uint32_t flags = e.label.find("dashboard-progress") != std::string::npos ? uint32_t(PM_MXF_MAX) : 0u;
    metrics_.entries.push_back(pm_mx_entry{metric_series_locked(e.task_id, e.label), flags, e.value});
  }
}

void GpuMatchPlugin::beat_metrics(const Address& address, const std::vector<MetricEntry>& entries) {
  queue_metrics(address, PM_MXB_REPLACE, entries);  // (an empty list is Some(vec![]): it empties the row)
}

void GpuMatchPlugin::store_metrics(const Address& address, const std::vector<MetricEntry>& entries) {
  if (entries.empty()) return;  // metrics_store.rs:34-36
  queue_metrics(address, PM_MXB_MERGE, entries);
}

void GpuMatchPlugin::store_manual_metric(const std::string& label, double value) {
  store_metrics(Address::zero(), {MetricEntry{"", label, value}});
}

void GpuMatchPlugin::delete_metric(const std::string& task_id, const std::string& label, const Address& address) {
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);
  uint32_t row = PM_MX_MANUAL;
  if (address != Address::zero()) {
    const auto it = nodes_.index.find(address);
    if (it == nodes_.index.end()) return;
    row = it->second;
  }
  std::lock_guard<std::mutex> lk(metrics_mu_);
  // (the key is "{task_id}:{cleaned}" as given, :100: no "manual" for an empty task id) a field nobody stored is in no row
  const auto it = metrics_.series.find(task_id + ":" + clean_label(label));
  if (it == metrics_.series.end()) return;
  metrics_.beats.push_back(pm_mx_beat{row, PM_MXB_DELETE, uint32_t(metrics_.entries.size()), 1u});
  metrics_.entries.push_back(pm_mx_entry{it->second, 0u, 0.0});
}

void GpuMatchPlugin::clear_metrics(const Address& address) { queue_metrics(address, PM_MXB_REPLACE, {}); }

void GpuMatchPlugin::flush_metrics_locked() {
  if (metrics_.beats.empty()) return;
  const uint32_t n_series = std::max<uint32_t>(uint32_t(metrics_.keys.size()), 1u);
  const int32_t rc = pm_metrics_ingest(engine_, metrics_.beats.data(), uint32_t(metrics_.beats.size()),
                                       metrics_.entries.empty() ? nullptr : metrics_.entries.data(), uint32_t(metrics_.entries.size()),
                                       n_series);
  metrics_.beats.clear();  // (a refused batch is dropped, not sent again and again)
  metrics_.entries.clear();
  check(rc);
}

void GpuMatchPlugin::flush_metrics() {
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);
  std::lock_guard<std::mutex> lk(metrics_mu_);
  flush_metrics_locked();
}

size_t GpuMatchPlugin::queued_metric_beats() const {
  std::lock_guard<std::mutex> lk(metrics_mu_);
  return metrics_.beats.size();
}

std::vector<pm_mx_row> GpuMatchPlugin::metric_rows_locked(const uint32_t* rows, uint32_t n) {
  uint32_t have = 0;
  const int32_t rc = pm_metrics_rows(engine_, rows, n, nullptr, 0u, &have);  // the size query: PM_ERANGE unless there is nothing
  if (rc != PM_ERANGE) check(rc);
  std::vector<pm_mx_row> out(have ? have : 1u);
  uint32_t got = 0;
  check(pm_metrics_rows(engine_, rows, n, out.data(), uint32_t(out.size()), &got));
  if (got > out.size()) throw std::out_of_range("metrics: the listing grew between two calls");
  out.resize(got);
  for (const pm_mx_row& r : out)
    if (r.series >= metrics_.keys.size() || (r.row != PM_MX_MANUAL && r.row >= nodes_.rows.size()))
      throw std::out_of_range("metrics: the engine lists an entry the plugin does not know");
  return out;
}

GpuMatchPlugin::MetricsByName GpuMatchPlugin::aggregate_metrics_for_all_tasks() {
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);
  std::lock_guard<std::mutex> lk(metrics_mu_);
  flush_metrics_locked();
  uint32_t n = 0;
  const int32_t rc = pm_metrics_totals(engine_, nullptr, nullptr, 0u, &n);
  if (rc != PM_ERANGE) check(rc);
  std::vector<double> sum(n ? n : 1u);
  std::vector<uint32_t> count(n ? n : 1u);
  check(pm_metrics_totals(engine_, sum.data(), count.data(), uint32_t(sum.size()), &n));
  MetricsByName out;
  for (uint32_t s = 0; s < n && s < metrics_.keys.size(); ++s)
    if (count[s]) out.emplace(metrics_.keys[s].second, 0.0).first->second += sum[s];  // :196
  return out;
}

GpuMatchPlugin::MetricsByName GpuMatchPlugin::aggregate_metrics_for_task(const std::string& task_id) {
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);
  std::lock_guard<std::mutex> lk(metrics_mu_);
  flush_metrics_locked();
  uint32_t n = 0;
  const int32_t rc = pm_metrics_totals(engine_, nullptr, nullptr, 0u, &n);
  if (rc != PM_ERANGE) check(rc);
  std::vector<double> sum(n ? n : 1u);
  std::vector<uint32_t> count(n ? n : 1u);
  check(pm_metrics_totals(engine_, sum.data(), count.data(), uint32_t(sum.size()), &n));
  MetricsByName out;
  for (uint32_t s = 0; s < n && s < metrics_.keys.size(); ++s)
    if (count[s] && metrics_.keys[s].first == task_id) out.emplace(metrics_.keys[s].second, 0.0).first->second += sum[s];  // :166-167
  return out;
}

GpuMatchPlugin::MetricsByTask GpuMatchPlugin::metrics_for_node(const Address& address) {
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);
  std::lock_guard<std::mutex> lk(metrics_mu_);
  flush_metrics_locked();
  uint32_t row = PM_MX_MANUAL;
  if (address != Address::zero()) {
    const auto it = nodes_.index.find(address);
    if (it == nodes_.index.end()) return {};
    row = it->second;
  }
  MetricsByTask out;
  for (const pm_mx_row& r : metric_rows_locked(&row, 1u)) out[metrics_.keys[r.series].first][metrics_.keys[r.series].second] = r.value;
  return out;
}

std::map<std::string, std::map<std::string, GpuMatchPlugin::MetricsByName>> GpuMatchPlugin::all_metrics() {
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);
  std::lock_guard<std::mutex> lk(metrics_mu_);
  flush_metrics_locked();
  std::map<std::string, std::map<std::string, MetricsByName>> out;
  for (const pm_mx_row& r : metric_rows_locked(nullptr, 0u)) {
    const std::string& address = r.row == PM_MX_MANUAL ? Address::zero().text : nodes_.address_strings[r.row];
    out[metrics_.keys[r.series].first][metrics_.keys[r.series].second][address] = r.value;
  }
  return out;
}

std::vector<GpuMatchPlugin::SyncedMetric> GpuMatchPlugin::synced_metrics(const std::map<std::string, std::string>& task_names) {
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);
  std::lock_guard<std::mutex> lk(metrics_mu_);
  flush_metrics_locked();
  std::vector<SyncedMetric> out;
  for (const pm_mx_row& r : metric_rows_locked(nullptr, 0u)) {
    SyncedMetric m;
    m.address = r.row == PM_MX_MANUAL ? Address::zero().text : nodes_.address_strings[r.row];
    m.task_id = metrics_.keys[r.series].first;
    const auto name = task_names.find(m.task_id);
    m.task_name = name == task_names.end() ? "unknown" : name->second;  // sync_service.rs:172-175
    m.label = metrics_.keys[r.series].second;
    m.value = r.value;
    if (r.group_id != uint64_t(PM_NONE)) {  // :179-182
      m.group_id = hex_lower(r.group_id);
      if (r.config >= config_names_.size()) throw std::out_of_range("metrics: the engine names a configuration the plugin has not");
      m.group_config_name = config_names_[r.config];
    }
    out.push_back(std::move(m));
  }
  return out;
}

}  // namespace orchestrator
