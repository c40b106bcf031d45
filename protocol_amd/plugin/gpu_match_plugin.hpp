// gpu_match_plugin.hpp — the host side of the drop-in, compiled: the orchestrator's scheduler types and the plugin that
// binds libpm_engine.so (include/pm_engine.h), in C++ because this image has no Rust toolchain.  It is the twin of
// rust/gpu_match_plugin.rs (the binding a maintainer adds to the reference; never compiled here), method for method and
// lock for lock, so that what the Rust source says is also said by something a compiler, the sanitizers and the tests
// have seen.  Names, argument meaning and error behaviour follow the reference (all paths relative to
// /root/reference/crates):
//
//   OrchestratorNode, NodeStatus          orchestrator/src/models/node.rs:11-37, :75-85 (the fields the path reads)
//   ComputeSpecs, GpuSpecs, CpuSpecs      shared/src/models/node.rs (compute_specs of a node)
//   Task, VolumeMount                     shared/src/models/task.rs:163-184, :60-98
//   NodeGroupConfiguration                orchestrator/src/plugins/node_groups/mod.rs:30-37
//   SchedulerPlugin::filter_tasks         orchestrator/src/plugins/mod.rs:60-79  (enum dispatch -> virtual call)
//   NewestTaskPlugin                      orchestrator/src/plugins/newest_task/mod.rs:8-20
//   Scheduler::get_task_for_node          orchestrator/src/scheduler/mod.rs:9-76, with the edit INTEGRATION.md shows
//                                         ("The task list per heartbeat": a chain headed by the engine's plugin does
//                                         not load the store's task list)
//   GpuMatchPlugin                        replaces NodeGroupsPlugin: new (mod.rs:113-175), the management loop's body
//                                         (tick = try_form_new_groups + try_merge_solo_groups, mod.rs:180-203),
//                                         filter_tasks (scheduler_impl.rs:11-205), handle_status_change
//                                         (status_update_impl.rs:8-39), the task observers (mod.rs:1224-1325)
//   WebhookPlugin                         orchestrator/src/plugins/webhook/mod.rs:240-266 (the two calls the path makes)
//   NodeGroup + the plugin's READ SURFACE  node_groups/mod.rs:63-69; get_node_group :324-337, get_node_groups_batch
//                                         :339-397, get_available_configurations :399-418,
//                                         get_all_configuration_templates :420-422, get_idx_in_group :424-434,
//                                         dissolve_group :1002-1004 (-> :1423-1487), get_all_groups :1006-1044,
//                                         get_group_by_id :1046-1055, get_all_node_group_mappings :1057-1065 — what the
//                                         API routes call on AppState.node_groups_plugin (api/routes/groups.rs:34-160,
//                                         :319-360, nodes.rs:68-90, storage.rs:147-156, metrics/sync_service.rs:57-75,
//                                         :273-274); get_task_topologies :1407-1421 (api/routes/task.rs:68-72)
//
// Errors: the Rust returns anyhow::Result and panics in the constructor; here every failed engine call throws
// EngineError (code + pm_last_error text) and the constructor's panics are std::invalid_argument with the reference's
// messages.  Rust's async is not mirrored: every method is a plain blocking call, as the FFI calls underneath are.
#ifndef PM_GPU_MATCH_PLUGIN_HPP
#define PM_GPU_MATCH_PLUGIN_HPP

#include <array>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <optional>
#include <shared_mutex>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "pm_engine.h"

namespace orchestrator {

// alloy::primitives::Address as the path uses it: a key, and `address.to_string()` (GROUP_INDEX is the rank of that
// string inside the group, node_groups/mod.rs:424-434; ${NODE_ADDRESS}).  Held as that string.
struct Address {
  std::string text;
  Address() = default;
  explicit Address(std::string s) : text(std::move(s)) {}
  const std::string& to_string() const { return text; }
  bool operator==(const Address& o) const { return text == o.text; }
  bool operator!=(const Address& o) const { return text != o.text; }
  static Address zero() { return Address("0x0000000000000000000000000000000000000000"); }
};
struct AddressHash {
  size_t operator()(const Address& a) const { return std::hash<std::string>()(a.text); }
};

enum class NodeStatus { Discovered, WaitingForHeartbeat, Healthy, Unhealthy, Dead, Ejected, Banned, LowBalance };

struct GpuSpecs {
  std::optional<uint32_t> count;
  std::optional<std::string> model;
  std::optional<uint32_t> memory_mb;
};
struct CpuSpecs {
  std::optional<uint32_t> cores;
};
struct ComputeSpecs {
  std::optional<GpuSpecs> gpu;
  std::optional<CpuSpecs> cpu;
  std::optional<uint32_t> ram_mb;
  std::optional<uint32_t> storage_gb;
};
struct NodeLocation {
  double latitude = 0.0, longitude = 0.0;
};
struct OrchestratorNode {
  Address address;
  NodeStatus status = NodeStatus::Discovered;
  std::optional<std::string> p2p_id;
  std::optional<ComputeSpecs> compute_specs;
  std::optional<NodeLocation> location;
};

struct VolumeMount {
  std::string host_path, container_path;
  // shared/src/models/task.rs:75-98 (${TIMESTAMP} takes `now`: the caller's clock, seconds)
  VolumeMount replace_labels(const std::string& task_id, const std::optional<std::string>& node_address, int64_t now) const;
};

struct Task {
  std::string id;    // Uuid, hyphenated lower-case hex (task.id.to_string())
  std::string name;
  std::string image;
  int64_t created_at = 0;
  // scheduling_config.plugins["node_groups"]["allowed_topologies"] (scheduler_impl.rs:44-59); nullopt = any None on the way
  std::optional<std::vector<std::string>> allowed_topologies;
  std::optional<std::map<std::string, std::string>> env_vars;
  std::optional<std::vector<std::string>> cmd;
  std::optional<std::vector<VolumeMount>> volume_mounts;
  bool operator==(const Task& o) const;
};
// task.id.as_u64_pair().1: the low 64 bits of the UUID — the identity the engine keeps a claim by
uint64_t task_uid(const Task& t);

struct NodeGroupConfiguration {
  std::string name;
  size_t min_group_size = 0, max_group_size = 0;
  // the reference holds a ComputeRequirements parsed by FromStr at deserialisation (shared/src/models/node.rs:180-374);
  // here the string travels and the library's parser (pm_host_parse_requirements) does that step
  std::optional<std::string> compute_requirements;
};

// NodeGroup (node_groups/mod.rs:63-69)
struct NodeGroup {
  std::string id;                  // generate_group_id: format!("{:x}", u64) (mod.rs:1489-1493)
  std::vector<std::string> nodes;  // BTreeSet<String>: address.to_string() in byte order
  int64_t created_at = 0;          // chrono::DateTime<Utc>, as milliseconds since the epoch: the plugin's clock when the
                                   // creation was reported to it (the reference stamps Utc::now() in the same loop pass, mod.rs:575)
  std::string configuration_name;
  bool operator==(const NodeGroup& o) const {
    return id == o.id && nodes == o.nodes && created_at == o.created_at && configuration_name == o.configuration_name;
  }
};

// the two calls of webhook/mod.rs the path makes; `nodes` in group.nodes (BTreeSet<String>) order
class WebhookPlugin {
 public:
  virtual ~WebhookPlugin() = default;
  virtual void send_group_created(const std::string& group_id, const std::string& configuration_name,
                                  const std::vector<std::string>& nodes) = 0;
  virtual void send_group_destroyed(const std::string& group_id, const std::string& configuration_name,
                                    const std::vector<std::string>& nodes) = 0;
};

class EngineError : public std::runtime_error {
 public:
  EngineError(int32_t code, const std::string& what) : std::runtime_error(what), code_(code) {}
  int32_t code() const { return code_; }

 private:
  int32_t code_;
};

// SchedulerPlugin (plugins/mod.rs:60-79): the reference's enum, as an interface
class SchedulerPlugin {
 public:
  virtual ~SchedulerPlugin() = default;
  virtual std::vector<Task> filter_tasks(const std::vector<Task>& tasks, const Address& node_address) = 0;
  // (true for the plugin that serves from its own task list — the scheduler then loads none)
  virtual bool serves_from_own_task_list() const { return false; }
};

class NewestTaskPlugin : public SchedulerPlugin {
 public:
  std::vector<Task> filter_tasks(const std::vector<Task>& tasks, const Address&) override;
};

// The collective of the multi-GPU tick (include/pm_engine.h "multi-GPU"): one process per GPU, every rank holds
// the whole swarm and runs the whole carve (replicated), the pair sweep + claim run for the OWNED workers, and the published
// rows are all-gathered ONCE per tick.  The plugin is handed the communicator; it owns none.
//   RcclAllGather (rccl_all_gather.hpp)   ncclAllGather over xGMI on the stream the engine's kernels run on
//   LocalAllGather (same header)          ranks that live in one process (tests; several ranks sharing a GPU)
class AllGather {
 public:
  virtual ~AllGather() = default;
  virtual uint32_t rank() const = 0;
  virtual uint32_t world() const = 0;
  // the hipStream_t the engine's kernels and the collective share (ordered without a host wait); nullptr = the engine's own
  virtual void* stream() const = 0;
  // device pointers; recv = [world][bytes_per_rank], send = this rank's segment (it may alias recv's own slot): enqueue on stream()
  virtual void all_gather(const void* send, void* recv, size_t bytes_per_rank) = 0;
};

// owner rank of a node: splitmix64 finaliser of the low 8 bytes of the address, mod world
uint32_t shard_of(const Address& a, uint32_t world);

// The third variant.  Thread-safe like the reference's Arc<NodeGroupsPlugin>: heartbeats (filter_tasks) from any
// thread beside the management loop (sync_nodes / tick), the status updater (handle_status_change) and the task
// store's observers (on_task_created / on_task_deleted).
// LOCK ORDER: `nodes_`, then `tasks_`, then the engine's own mutex (inside every pm_* call but the look-up) — the
// order rust/gpu_match_plugin.rs states; tests/cpp/plugin_test.cpp runs it under ThreadSanitizer.
class GpuMatchPlugin : public SchedulerPlugin {
 public:
  using UploadCounter = std::function<size_t(const Address&, const std::string& group_id)>;

  // NodeGroupsPlugin::new's contract (mod.rs:113-175): duplicate names -> "Configuration names must be unique",
  // max < min (or min == 0, which the engine refuses too) -> "Plugin configuration is invalid"; both
  // std::invalid_argument.  An unparsable requirement string is std::invalid_argument as well (the reference fails
  // earlier, at deserialisation).
  GpuMatchPlugin(std::vector<NodeGroupConfiguration> templates, int32_t device, UploadCounter upload_counter,
                 std::vector<std::shared_ptr<WebhookPlugin>> webhook_plugins = {});
  ~GpuMatchPlugin() override;
  GpuMatchPlugin(const GpuMatchPlugin&) = delete;
  GpuMatchPlugin& operator=(const GpuMatchPlugin&) = delete;

  // every management interval, with node_store.get_nodes() (any order): new nodes are appended, changed rows
  // rewritten, departed nodes tombstoned (their groups dissolve)
  void sync_nodes(const std::vector<OrchestratorNode>& snapshot);
  // task_store.get_all_tasks() (created_at descending): start-up, and the fallback when a delta does not apply
  void sync_tasks(std::vector<Task> tasks);
  // the task store's observers (mod.rs:1224-1243, :1245-1325)
  void on_task_created(const Task& task, const std::function<std::vector<Task>()>& all_tasks);
  void on_task_deleted(const Task& task);
  // one body of run_group_management_loop (mod.rs:180-203) + every worker's filter_tasks, then the webhooks
  pm_stats tick();
  // A process that serves several pools on one GPU (INTEGRATION.md "Several pools on one GPU"): one pm_tick_many call —
  // every pool's carve started before the first is waited for — then each pool's webhooks.  pools[i]->tick() K times
  // in a row matches one pool after the other.
  static std::vector<pm_stats> tick_many(const std::vector<GpuMatchPlugin*>& pools);
  // The management interval of ONE pool matched by several GPUs, one process (or thread) per GPU: this plugin is rank
  // comm.rank() of comm.world().  Every rank is fed every store event (sync_nodes, the task observers, status changes —
  // replicated calls) and calls tick_dist at the same point of its loop; every rank ends with the identical groups and
  // the full published table (any rank answers any heartbeat).  The five calls of INTEGRATION.md "Multi-GPU":
  // pm_dist_tick_begin, pm_dist_carve_wait, pm_dist_match_begin, the ONE all-gather, pm_dist_tick_end.  From its first
  // tick_dist on a plugin of rank > 0 delivers no webhooks (every rank sees every creation and dissolution: rank 0 reports
  // them; the others drain their feed and keep the created_at stamps).  Called by the management loop's thread only
  // (like tick); ownership is recomputed when the node table grew.
  pm_stats tick_dist(AllGather& comm);
  // SchedulerPlugin::filter_tasks: `tasks` is ignored (the plugin serves from its own list)
  std::vector<Task> filter_tasks(const std::vector<Task>& tasks, const Address& node_address) override;
  bool serves_from_own_task_list() const override { return true; }
  // StatusUpdatePlugin::handle_status_change (status_update_impl.rs:8-39)
  void handle_status_change(const OrchestratorNode& node);

  // ---- the read surface the API routes use (AppState.node_groups_plugin in the reference; INTEGRATION.md "The routes").
  // Host-side state of the engine only: no GPU work, any thread, also while a tick runs (it then waits for the tick).
  // get_all_groups (mod.rs:1006-1044): every group, sorted by id text (:1040)
  std::vector<NodeGroup> get_all_groups() const;
  // get_group_by_id (mod.rs:1046-1055): an id that is not the "{:x}" text of a live group's id is nullopt
  std::optional<NodeGroup> get_group_by_id(const std::string& group_id) const;
  // get_all_node_group_mappings (mod.rs:1057-1065): node address text -> group id text (HGETALL node_to_group)
  std::unordered_map<std::string, std::string> get_all_node_group_mappings() const;
  // get_node_group (mod.rs:324-337): the group of the node with this address TEXT (the key of the reference's hash)
  std::optional<NodeGroup> get_node_group(const std::string& node_addr) const;
  // get_node_groups_batch (mod.rs:339-397): every asked address is a key of the result; one snapshot of the engine's list
  std::unordered_map<std::string, std::optional<NodeGroup>> get_node_groups_batch(const std::vector<std::string>& node_addresses) const;
  // get_idx_in_group (mod.rs:424-434): position in group.nodes; "Node {} not found in group" -> std::out_of_range
  size_t get_idx_in_group(const NodeGroup& node_group, const std::string& node_addr) const;
  // get_available_configurations (mod.rs:399-418): the templates some task names, min_group_size descending (stable)
  std::vector<NodeGroupConfiguration> get_available_configurations() const;
  // get_all_configuration_templates (mod.rs:420-422): in the constructor's order (mod.rs:150-164)
  std::vector<NodeGroupConfiguration> get_all_configuration_templates() const;
  // dissolve_group (mod.rs:1002-1004 -> :1423-1487): by id text; an unknown id is not an error; sends the webhook
  void dissolve_group(const std::string& group_id);

  // ---- restart and switch-over (INTEGRATION.md "Restart and switch-over"; gpu_match_restore.cpp).
  struct RestoreReport {
    std::vector<std::pair<std::string, std::string>> dropped;  // (group id text, reason)
    std::vector<std::string> task_cleared;                     // group_task:<id> naming no known task
  };
  // The groups a store holds (orchestrator:groups_index / node_group:<id> in get_all_groups order, group_task:<id>) into the
  // engine: after sync_nodes and sync_tasks, before the first tick — EngineError(PM_ESTATE) at any other time.  A group is
  // dropped (and reported, not thrown) when its id is not the "{:x}" text of a u64, its configuration name is unknown, a node
  // address is not in the node table, a node is in an earlier group, it has no nodes, more than max_group_size nodes, or the
  // id of an earlier group.  A group_task naming an unknown task leaves the group without one (get_current_group_task,
  // mod.rs:436-469) and is listed in task_cleared.  created_at is kept.  An absent id_state is drawn from
  // std::random_device (the reference's ids are random, mod.rs:1489-1493) — std::invalid_argument on a multi-GPU pool
  // (multi_gpu below), whose ranks must draw the same ids.  Ends with one pm_match: heartbeats are served from the adopted
  // groups at once, and a taskless group claims a task there, as at its first filter_tasks.
  RestoreReport restore_groups(const std::vector<NodeGroup>& groups, const std::unordered_map<std::string, std::string>& group_tasks,
                               std::optional<uint64_t> id_state);
  // group id text -> task id of every group that holds a task (what group_task:<id> holds), for the store's write-through
  std::unordered_map<std::string, std::string> group_tasks() const;
  // the state of the group id stream, for a successor's restore_groups (persisted under a key of the plugin's own)
  uint64_t group_id_state() const;
  // this plugin is one rank of a pool that runs tick_dist: restore_groups needs an id_state (set before calling it)
  bool multi_gpu = false;

  // ---- diagnostics (INTEGRATION.md "Diagnostics"; gpu_match_report.cpp): the engine's three read-only reports by name.
  // Reason names, PM_WHY_* order: "ok", "no_specs", "cpu", "ram", "storage", "gpu_none", "gpu_count", "gpu_model", "gpu_mem",
  // "gpu_total"; states: "in_group", "unhealthy", "no_p2p", "idle".
  struct NodeExplanation {
    std::string state;
    std::vector<std::pair<std::string, std::string>> configs;  // (configuration name, reason name), constructor order
  };
  // why a node sits idle: nullopt when the node table does not hold the address
  std::optional<NodeExplanation> explain_node(const std::string& address) const;
  struct ConfigurationReport {
    std::string name;
    bool enabled = false;
    uint32_t eligible_meets = 0, idle_meets = 0;
    std::array<uint32_t, 10> why{};  // Healthy nodes with a p2p id by reason code (why[0] == eligible_meets)
    uint32_t groups = 0, members = 0, groups_without_task = 0, tasks_allowing = 0;
  };
  // how much room each configuration has left, constructor order
  std::vector<ConfigurationReport> configuration_report() const;
  struct TaskReport {
    uint32_t groups_running = 0;   // get_groups_for_task (mod.rs:1350-1386)
    uint32_t workers_running = 0;  // nodes_per_task (metrics/sync_service.rs:243-267)
    uint32_t groups_allowed = 0;   // live groups whose configuration the task's topologies allow
  };
  // by task id, every task of the last sync_tasks / on_task_created / on_task_deleted
  std::unordered_map<std::string, TaskReport> task_report() const;
  static const char* why_name(uint32_t code);
  static const char* state_name(uint32_t state);

  // ---- group geography (INTEGRATION.md "Diagnostics"; gpu_match_spread.cpp): pm_group_spread / pm_config_spread by name, and
  // POST /groups/force-regroup (api/routes/groups.rs:319-380) as one call with a selection.
  struct GroupSpread {
    uint32_t located = 0, ring_hops = 0;
    std::string far_a, far_b, hop_from;  // node addresses; empty = none (fewer than two located nodes / no measured hop)
    double diameter_km = 0.0, ring_km = 0.0, longest_hop_km = 0.0;
  };
  // every live group by id text ("{:x}")
  std::unordered_map<std::string, GroupSpread> group_spread() const;
  struct ConfigurationSpread {
    std::string name;
    uint32_t groups = 0, measured = 0;
    std::array<uint32_t, PM_SPREAD_BUCKETS> hist{};  // measured groups by diameter (PM_SPREAD_EDGES_KM)
    double max_diameter_km = 0.0, max_hop_km = 0.0;
    uint64_t sum_diameter_m = 0, sum_ring_m = 0;
  };
  // constructor order
  std::vector<ConfigurationSpread> configuration_spread() const;
  struct ForceRegroupResult {
    uint32_t dissolved_groups = 0, affected_nodes = 0;
  };
  // metric: PM_REGROUP_ALL (the route as the reference has it), PM_REGROUP_DIAMETER or PM_REGROUP_LONGEST_HOP with
  // threshold_km.  nullopt: no configuration has this name (the route's 404).  Sends the destroyed webhooks, in
  // get_all_groups order.
  std::optional<ForceRegroupResult> force_regroup(const std::string& configuration_name, uint32_t metric = PM_REGROUP_ALL,
                                                  double threshold_km = 0.0);

  // ---- nearest candidates (INTEGRATION.md "Diagnostics: nearest candidates"; gpu_match_near.cpp): pm_nearest_workers by
  // address and configuration name.
  struct NearestNodes {
    std::string origin;       // the node the list is measured from; empty: the seed rule found no candidate
    uint32_t candidates = 0;  // nodes of the pool that meet the configuration, the origin excluded
    uint32_t located = 0;     // of them with a location
    std::vector<std::pair<std::string, double>> nodes;  // (address, km), nearest first; km = DBL_MAX: not measured
  };
  // address nullopt: from the seed try_form_new_groups would take for the configuration now (PM_NEAR_SEED).  pool:
  // PM_NEAR_IDLE (the next carve's candidates) or PM_NEAR_ELIGIBLE (Healthy with a p2p id, grouped or not); k in
  // [1, PM_NEAR_MAX_K].  nullopt: the node table does not hold the address.  std::invalid_argument: no configuration has
  // this name.
  std::optional<NearestNodes> nearest_nodes(const std::optional<std::string>& address, const std::string& configuration_name,
                                            uint32_t pool = PM_NEAR_IDLE, uint32_t k = 16) const;

  // ---- probing configurations (INTEGRATION.md "Diagnostics: probing configurations"; gpu_match_probe.cpp): pm_probe_configs /
  // pm_config_overlap by name.  What a configuration that is NOT installed — or a task's requirements — would find in the
  // swarm right now, and which installed configurations compete for the same idle nodes.
  struct ProbeResult {
    std::string name;
    std::array<uint32_t, 10> why{};  // Healthy nodes with a p2p id by reason code (why[0] == eligible_meets)
    uint32_t eligible_meets = 0, idle_meets = 0, idle_located = 0, idle_exclusive = 0;
    uint32_t groups_max = 0, groups_exclusive = 0;  // bounds from counts (/ min_group_size), not what a carve would form
    // (installed configuration name, idle nodes that meet the probe AND it), constructor order
    std::vector<std::pair<std::string, uint32_t>> overlap;
  };
  // name, sizes and requirement string of every probe, packed exactly as the constructor packs the installed ones, the model
  // rule against the node table's interned spec models.  A requirement string that does not parse: the constructor's
  // std::invalid_argument, before any engine call.  One result per probe, in the given order.
  std::vector<ProbeResult> probe_configurations(const std::vector<NodeGroupConfiguration>& probes) const;
  struct ConfigurationOverlap {
    std::vector<std::string> names;  // constructor order
    std::vector<uint32_t> idle;      // [a * names.size() + b]: idle nodes that meet both a and b (symmetric)
  };
  ConfigurationOverlap configuration_overlap() const;

  // ---- change feed (INTEGRATION.md "Change feed"; gpu_match_changes.cpp): pm_enable_assignment_changes /
  // pm_drain_assignment_changes by address — the nodes whose published row (task, GROUP_ID, GROUP_INDEX, GROUP_SIZE,
  // NEXT_P2P_ADDRESS: scheduler_impl.rs:33-128) a tick changed since the last call.
  struct ChangedNodes {
    std::vector<std::pair<std::string, uint32_t>> nodes;  // (address, OR of PM_CHG_*), in row order
    bool resync = false;  // the engine lost track (include/pm_engine.h "RESYNC"): every node is listed, render them all
  };
  void enable_change_feed(bool on) const;  // off also clears; on = resync
  // drains the feed.  std::out_of_range: the engine lists a row the node table does not hold.
  ChangedNodes changed_nodes() const;

  // ---- liveness (INTEGRATION.md "Liveness"; gpu_match_liveness.cpp): NodeStatusUpdater::process_nodes
  // (status_update/mod.rs:144-372) as pm_liveness_sweep over the plugin's rows, and the heartbeat route's
  // heartbeat_store.beat (routes/heartbeat.rs:54-93) as a store into a column of atomics indexed by the node's row.
  struct StatusTransition {
    std::string address;
    NodeStatus old_status, new_status;
  };
  // pm_liveness_enable(on = 1): the ledger starts from the rows' Healthy bit; from here on handle_status_change also
  // writes the ledger (pm_liveness_set: the status; the counter kept, cleared by WaitingForHeartbeat as the invite does)
  void enable_liveness(uint32_t missing_heartbeat_threshold = 3);
  // no engine call: under the shared node lock.  An address the node table does not hold is ignored (the route answers
  // such a node before it gets here).
  void beat(const Address& address, uint64_t now_ms) const;
  // one process_nodes pass: the engine sweeps with apply = 1 (flags, dissolutions and webhooks as handle_status_change would
  // have them), the rows' Healthy bits follow, and the transitions come back in row order for the host's metric clean-up
  // and chain sync (mod.rs:314-350, :118-142).  out_of_pool: the nodes is_node_in_pool (mod.rs:380-390) is false for;
  // empty = the cfg(test) stub.
  std::vector<StatusTransition> sweep_statuses(uint64_t now_ms, const std::vector<Address>& out_of_pool = {});

  // ---- discovery sync (INTEGRATION.md "Discovery sync"; gpu_match_discovery.cpp): DiscoveryMonitor::get_nodes ->
  // sync_single_node_with_discovery (discovery/monitor.rs:218-435) as pm_discovery_sync over the plugin's rows.  Needs
  // enable_liveness (the statuses are the ledger's).  The plugin keeps the store's ip and port per row (the endpoint column;
  // OrchestratorNode does not carry them: set_endpoint tells them, and a sync's own ip rewrites follow), the interning map
  // "ip:port" -> endpoint id, and last_status_change per row (set by handle_status_change, sweep_statuses and sync_discovery).
  struct DiscoverySighting {       // what sync_single_node_with_discovery reads of a DiscoveryNode
    Address address;
    std::string ip_address;
    uint16_t port = 0;
    bool is_validated = false, is_provider_whitelisted = false, is_active = false;
    bool location_new = false;     // the store's location is None and discovery's is Some (monitor.rs:345)
    bool specs_differ = false;     // existing_node.compute_specs != discovery_node.compute_specs (:367)
    bool balance_zero = false;     // latest_balance == Some(0) (:385-386)
    uint64_t last_updated_ms = 0;  // discovery.last_updated, 0 = None
  };
  struct DiscoveryOutcome {        // one per sighting, in order
    enum class Kind { Admitted, Skipped, Synced } kind = Kind::Synced;
    std::string address;
    uint32_t healthy_same_endpoint = 0;
    NodeStatus old_status = NodeStatus::Discovered, final_status = NodeStatus::Discovered;  // (Synced)
    std::vector<std::pair<NodeStatus, NodeStatus>> updates;                                // (old, new) as the handlers saw them
    bool ip_rewritten = false, location_new = false, specs_rewritten = false, stamped_now = false;
  };
  // the store's ip and port of a node the plugin has a row for (start-up, add_node by another writer); unknown addresses are
  // remembered until sync_nodes brings their row
  void set_endpoint(const Address& address, const std::string& ip_address, uint16_t port);
  // one get_nodes pass, applied (flags, dissolutions, webhooks as handle_status_change would have them; the rows' Healthy bits,
  // stamps and endpoints follow).  A sighting whose address has no present row is the reference's Ok(None): admitted or
  // skipped.  ADMITTED NODES ARE RETURNED, NOT APPENDED: the caller adds them to its store and the next sync_nodes brings their
  // rows (their endpoint is remembered from the sighting).  The store writes of location and specs are the caller's.
  std::vector<DiscoveryOutcome> sync_discovery(uint64_t now_ms, const std::vector<DiscoverySighting>& sightings,
                                               uint32_t max_same_endpoint);
  std::optional<std::pair<std::string, uint16_t>> endpoint_of(const Address& address) const;  // (what the tests look at)
  uint64_t last_status_change_ms(const Address& address) const;                               // 0 = None

  // ---- metrics (INTEGRATION.md "Metrics"; gpu_match_metrics.cpp): MetricsStore (store/domains/metrics_store.rs), the heartbeat
  // route's metric block (api/routes/heartbeat.rs:94-151) and the sync service's list (metrics/sync_service.rs:127-200) over the
  // engine's metrics ledger.  The plugin interns the reference's hash field "{task_id or "manual"}:{label without ':'}" to a
  // series, takes the keep-the-maximum flag from the ORIGINAL label ("dashboard-progress", metrics_store.rs:52), queues the
  // writes and sends them in one pm_metrics_ingest per flush; every read flushes first.  Address::ZERO is the manual row; an
  // address the node table does not hold is ignored (the route answers such a node before it gets here).
  struct MetricEntry {  // shared::models::metric::MetricEntry
    std::string task_id, label;
    double value = 0.0;
  };
  struct SyncedMetric {  // one record_compute_task_gauge call of sync_metrics_from_redis
    std::string address, task_id, task_name, label;
    double value = 0.0;
    std::optional<std::string> group_id, group_config_name;
  };
  using MetricsByName = std::map<std::string, double>;
  using MetricsByTask = std::map<std::string, MetricsByName>;
  void enable_metrics();  // pm_metrics_enable(on = 1): an empty ledger; the queue and the interner start over
  void beat_metrics(const Address& address, const std::vector<MetricEntry>& entries);   // heartbeat.rs:94-151 (Some(metrics))
  void store_metrics(const Address& address, const std::vector<MetricEntry>& entries);  // metrics_store.rs:25-75
  void store_manual_metric(const std::string& label, double value);                     // :77-89
  void delete_metric(const std::string& task_id, const std::string& label, const Address& address);  // :91-109
  void clear_metrics(const Address& address);  // the clean-up of an Ejected / Banned node (status_update/mod.rs:314-343)
  void flush_metrics();
  MetricsByName aggregate_metrics_for_all_tasks();                          // :176-202, rolled up in ascending series order
  MetricsByName aggregate_metrics_for_task(const std::string& task_id);     // :143-174
  MetricsByTask metrics_for_node(const Address& address);                   // :111-131
  std::map<std::string, std::map<std::string, MetricsByName>> all_metrics();  // :204-240: task -> name -> address -> value
  // sync_service.rs:127-200: every entry with its task's name ("unknown" where the map has none) and its node's group
  std::vector<SyncedMetric> synced_metrics(const std::map<std::string, std::string>& task_names);
  size_t queued_metric_beats() const;  // (what the tests look at)

  // ---- rollout (INTEGRATION.md "Rollout"; gpu_match_rollout.cpp): the task fields the heartbeat route stores per node
  // (api/routes/heartbeat.rs:54-73 -> NodeStore::update_node_task, node_store.rs:339-377) over the engine's rollout ledger, and the
  // reads that join them with the standing groups.  report_task applies update_node_task's match: both options present set the
  // report, anything else clears it.  The state goes through pm_host_task_state (TaskState::from); the id is task_uid of the text
  // when it is a UUID, else a 64-bit FNV-1a of its bytes — A DEVIATION: two texts whose 64-bit ids collide are one id to the
  // ledger (the reference keys by the text).  The plugin remembers the text of every reported id, so that ids its task list does
  // not carry (never, or no longer) render with their text; an entry goes when a task report no longer lists the id.  The writes queue
  // under the plugin's lock and go out in one pm_rollout_ingest per flush; every read flushes first.  An address the node table
  // does not hold is ignored (the route answers such a node before it gets here).
  struct NodesPerTask {  // one set_nodes_per_task call of the sync service (metrics/sync_service.rs:258-266)
    std::string task_id, task_name;  // "unknown" where the task list has no such id
    uint32_t count = 0;
  };
  struct TaskRollout {
    std::string task_id, task_name;
    pm_ro_task_row row;
  };
  struct GroupRollout {
    std::string group_id, configuration_name, task_id;
    pm_ro_group_row row;
  };
  struct NodeRollout {
    std::string address;
    uint32_t cls = 0, state = PM_TS_NONE;
    std::optional<std::string> task_id;  // the reported id's text (hex where the plugin has none), nullopt: no report
  };
  void enable_rollout();  // pm_rollout_enable(on = 1): empty columns; the queue and the texts start over
  void report_task(const Address& address, const std::optional<std::string>& task_id, const std::optional<std::string>& task_state);
  void flush_rollout();
  std::vector<NodesPerTask> nodes_per_task();  // ascending by the 64-bit id (the reference's order is a HashMap's)
  pm_ro_summary rollout_summary();
  std::vector<TaskRollout> task_rollout();
  std::vector<GroupRollout> group_rollout();
  std::vector<NodeRollout> rollout_nodes(uint32_t class_mask);
  size_t queued_task_reports() const;  // (what the tests look at)
  std::pair<std::vector<uint64_t>, std::vector<uint8_t>> reported_tasks(const std::vector<uint32_t>& rows);  // the ledger's rows as stored
  size_t remembered_task_texts() const;
  static uint64_t reported_task_uid(const std::string& task_id);

  // ---- node directory (INTEGRATION.md "Node directory"; gpu_match_directory.cpp): the store's ordered listing
  // (NodeStore::get_nodes, store/domains/node_store.rs:163-209: Healthy, Discovered, everything else, Dead) over the engine's
  // pm_directory, for its callers: GET /nodes (api/routes/nodes.rs:29-105), the sync service's gauge (metrics/sync_service.rs:
  // 209-225), the inviter (node_store.rs:247-282) and sync_chain_with_nodes (status_update/mod.rs:118-142).  Needs
  // enable_liveness: the statuses are the ledger's.  Inside a class the order is the row's (PM_DIR_BY_ROW) or the address
  // text's (PM_DIR_BY_ADDRESS: the rank column sync_nodes keeps) — A DEVIATION: the reference's is SMEMBERS', which nothing
  // pins.  Only the asked window and the counters leave the device.  LOCK ORDER: nodes, the engine.
  struct ListedGroup {  // the route's "group" object (nodes.rs:83-88)
    std::string id;
    uint32_t size = 0;
    int64_t created_at = 0;
    std::string topology_config;  // the configuration's NAME
  };
  struct ListedNode {
    std::string address;
    NodeStatus status = NodeStatus::Discovered;
    uint32_t unhealthy_counter = 0;
    uint32_t task_state = PM_TS_NONE;  // the reported state (PM_TS_*), PM_TS_NONE: no report or rollout off
    std::optional<ListedGroup> group;
  };
  struct NodeListing {
    uint32_t total = 0;                      // the whole filtered list's length, not the window's
    std::map<std::string, uint32_t> counts;  // per status name as `{:?}` prints it, over the whole filtered list; present ones only
    std::vector<ListedNode> nodes;           // the window
  };
  NodeListing list_nodes(bool include_dead, uint32_t order = PM_DIR_BY_ROW, uint32_t offset = 0, uint32_t limit = 0xFFFFFFFFu) const;
  std::map<std::string, uint32_t> status_counts() const;  // every node, lowercase names (sync_service.rs:220), present ones only
  std::vector<std::string> uninvited_nodes() const;       // the Discovered nodes' addresses, in row order
  std::vector<std::string> dead_nodes() const;            // the Dead nodes' addresses, in row order (the pool test stays the host's)
  static const char* status_name(uint32_t status);        // NodeStatus as `{:?}` prints it

  // ---- group directory (INTEGRATION.md "Group directory"; gpu_match_groupdir.cpp): GET /groups joined, filtered and paged —
  // the groups as the reference's route lists them (api/routes/groups.rs:32-66, get_all_groups' id-text order), each with the
  // health class of its members (the liveness ledger), its rollout class (the rollout ledger) and its claimed task; the
  // groups_count gauge (metrics/sync_service.rs:272-286); the groups that stand on a member that is not Healthy.  Only the
  // asked window and the counters leave the device.  A class filter other than "all" needs its ledger (enable_liveness /
  // enable_rollout), else EngineError(PM_ESTATE).  Two deviations: a group's nodes on equal ranks are ordered by row (the
  // ranks sync_nodes keeps are a permutation, so: none in practice), and created_at is the plugin's clock, as in
  // get_all_groups.  LOCK ORDER: nodes, tasks, the engine.  get_all_groups stays as it is.
  struct GroupFilter {
    uint64_t config_mask = ~0ull;  // bit c: the configuration of constructor index c
    uint32_t holds = PM_GDIR_ANY;
    uint32_t size_min = 0, size_max = 0xFFFFFFFFu;
    uint32_t health_mask = (1u << PM_GH_N) - 1u, rollout_mask = (1u << PM_GR_N) - 1u;
  };
  struct ListedNodeGroup {
    NodeGroup group;                     // id text, node address texts in member order, the plugin's created_at, the configuration name
    uint32_t health = PM_GH_NONE;        // PM_GH_*, PM_GH_NONE: liveness is off
    uint32_t rollout = PM_GR_NONE;       // PM_GR_*, PM_GR_NONE: rollout is off
    std::optional<std::string> task_id;  // the claimed task
    pm_gdir_row row{};                   // the counters per status and per rollout relation
  };
  struct GroupListing {
    uint32_t total = 0;        // the whole filtered list's length, not the window's
    pm_gdir_totals totals{};
    std::vector<ListedNodeGroup> groups;  // the window
  };
  GroupListing list_groups(const GroupFilter& filter, uint32_t order = PM_GDIR_BY_ID_TEXT, uint32_t offset = 0,
                           uint32_t limit = 0xFFFFFFFFu) const;
  std::map<std::string, uint32_t> group_counts() const;  // configuration name -> groups, present ones only: one counters-only query
  std::vector<ListedNodeGroup> degraded_groups() const;  // health LOST or DEGRADED, in id-text order

  // ---- task directory (INTEGRATION.md "Task directory"; gpu_match_taskdir.cpp): GET /tasks joined, filtered and paged — the
  // tasks as TaskStore::get_all_tasks lists them (store/domains/task_store.rs:57-82, newest first; api/routes/task.rs:20-39), each
  // with what get_groups_for_task would count (node_groups/mod.rs:1350-1386), what its nodes report and its two classes: can it
  // run on a standing group, has every member of its groups picked it up.  Ids and names are the plugin's own, by the position
  // the engine reports.  Only the asked window and the counters leave the device.  A rollout filter other than "all" and the
  // order by reporters need enable_rollout, else EngineError(PM_ESTATE); queued task reports are not flushed here (flush_rollout,
  // or any rollout read, does).  LOCK ORDER: nodes, tasks, the engine.
  struct TaskFilter {
    uint64_t config_mask = ~0ull;  // ~0: no filter; else bit c: tasks that allow the configuration of constructor index c
    uint32_t serve_mask = (1u << PM_TKS_N) - 1u, rollout_mask = (1u << PM_TKR_N) - 1u;
    uint32_t workers_min = 0, workers_max = 0xFFFFFFFFu;
  };
  struct ListedTask {
    std::string id, name;
    uint32_t serve = PM_TKS_STARVED;   // PM_TKS_*
    uint32_t rollout = PM_TKR_NONE;    // PM_TKR_*, PM_TKR_NONE: rollout is off
    pm_tdir_row row{};                 // the assigned and the reported columns
  };
  struct TaskListing {
    uint32_t total = 0;        // the whole filtered list's length, not the window's
    pm_tdir_totals totals{};
    std::vector<ListedTask> tasks;  // the window
  };
  struct TaskCounts {
    pm_tdir_totals totals{};
    std::map<std::string, uint32_t> by_config;  // configuration name -> tasks that allow it, present ones only
  };
  // what sync_orchestrator_statistics sets (metrics/sync_service.rs:209-286); the gauges themselves stay the host's
  struct OrchestratorStatistics {
    std::map<std::string, uint32_t> nodes_by_status;  // lowercase status name -> nodes, present ones only
    uint32_t tasks_count = 0;
    std::vector<NodesPerTask> nodes_per_task;         // (id, name or "unknown", count) of the tasks with reporters
    std::map<std::string, uint32_t> groups_count;     // configuration name -> groups, present ones only
  };
  TaskListing list_tasks(const TaskFilter& filter, uint32_t order = PM_TDIR_BY_LIST, uint32_t offset = 0,
                         uint32_t limit = 0xFFFFFFFFu) const;
  TaskCounts task_counts() const;                  // one counters-only query
  std::vector<ListedTask> starved_tasks() const;   // serving class STARVED, in list order
  // counters-only queries of the three directories and the rollout task table, one after the other (each under the locks it
  // needs: not one snapshot); needs enable_liveness and enable_rollout
  OrchestratorStatistics orchestrator_statistics();

  // ---- address book (INTEGRATION.md "Address book"; gpu_match_addresses.cpp): pm_addresses_* / pm_invite_digests.  Off by
  // default: the texts the callers passed are ranked on the host and rendered as they came.  With the book on, sync_nodes
  // parses each NEW node's address text to its 20 bytes (an optional "0x", 40 hex digits of either case; anything else, or a
  // second spelling of an address that has a row, is EngineError(PM_EINVAL) naming the text, before anything changed), sends
  // only the new rows' bytes and calls pm_addresses_rank where it kept `by_address` sorted and replaced the whole rank column;
  // every address text the read surface renders is the device's EIP-55 text (`Address: Display`), fetched once per new row.
  // Texts passed IN are looked up by their bytes, so any spelling finds the node.
  void enable_address_book();  // with rows already known: parses and sends them all, ranks, fetches their texts
  bool address_book_enabled() const;
  static bool parse_address_text(const std::string& text, uint8_t out20[20]);
  // NodeInviter::generate_invite up to the signature (node/invite.rs:86-115), for the nodes uninvited_nodes() lists, in its order:
  // `nonce` is asked once per node (rand::random there), expiration_s is the caller's clock; the ECDSA step stays with the wallet
  struct InviteDigest {
    std::string address;
    std::array<uint8_t, 32> nonce{}, digest{}, signing_hash{};
  };
  std::vector<InviteDigest> invite_digests(uint32_t domain_id, uint32_t pool_id, const std::function<std::array<uint8_t, 32>()>& nonce,
                                           uint64_t expiration_s) const;

  // ---- request gate (INTEGRATION.md "Request gate"; gpu_match_gate.cpp): pm_verify_requests.  ValidateSignature
  // (auth_signature_middleware.rs:374-422) and the heartbeat handler's ban check (routes/heartbeat.rs:38-52) for a batch of
  // requests in ONE engine call: `message` is path + payload string as the middleware formats it, `signature` and `address` the
  // two header texts.  A signature text that is not an optional "0x" and 130 hex digits is PM_RQ_BAD_SIGNATURE (it travels with
  // v = 0xFF, so the device's census counts it); an address text the book's parser refuses sets PM_RQ_FLAG_BAD_ADDRESS.  The
  // verdict's row is the plugin's row: beat, report_task and beat_metrics can be fed from it.  The rate limit, the request's age
  // and the nonce (:424-483) stay with the caller.  Needs enable_address_book: EngineError(PM_ESTATE) without.
  struct GateRequest {
    std::string message, signature, address;
  };
  struct GateVerdict {
    uint32_t code = PM_RQ_BAD_SIGNATURE;
    uint32_t row = 0xFFFFFFFFu;
    uint8_t status = 0xFF;  // PM_NS_*, 0xFF: no row, or liveness is off
    std::array<uint8_t, 20> address{};
  };
  struct GateResult {
    std::vector<GateVerdict> verdicts;
    std::array<uint32_t, PM_RQ_N_CODES> counts{};
  };
  GateResult verify_requests(const std::vector<GateRequest>& requests) const;
  static bool parse_signature_text(const std::string& text, uint8_t out65[65]);

  // ---- request gate: admission (INTEGRATION.md "Request gate: admission"; gpu_match_admission.cpp): pm_admit_requests.  The
  // whole of the middleware behind its signature check (auth_signature_middleware.rs:424-483: rate limit, age, nonce) and the
  // heartbeat handler's stamp, for a batch in ONE engine call, handled as if one after another in batch order, all at now_ms.
  // `timestamp` and `nonce` are what the middleware reads from the payload or the query (:301-372; none, or a timestamp that is
  // no u64: the middleware skips the age / answers MISSING_NONCE).  `heartbeat`: the route is /heartbeat — an OK stamps the row's beat on the device.  enable_admission needs enable_address_book
  // (EngineError(PM_ESTATE) without); from then on sweep_statuses sweeps over the later of the device's column and the plugin's
  // own (pm_liveness_sweep_beats), so beat() keeps working.
  struct AdmitRequest {
    std::string message, signature, address;
    std::optional<std::string> timestamp, nonce;
    bool heartbeat = false;
  };
  struct AdmitResult {
    std::vector<GateVerdict> verdicts;
    std::array<uint32_t, PM_AD_N_CODES> counts{};
  };
  void enable_admission();
  AdmitResult admit_requests(const std::vector<AdmitRequest>& requests, uint64_t now_ms) const;

  // chrono::Utc::now() for NodeGroup.created_at, milliseconds since the epoch (tests inject their own)
  std::function<int64_t()> clock = [] {
    return int64_t(std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::system_clock::now().time_since_epoch()).count());
  };

  // on_task_created also re-matches the standing groups (pm_tasks_insert_front_ex, republish = 1)
  std::atomic<bool> republish_on_insert{false};

  pm_engine* engine_ptr() const { return engine_; }   // (a process that serves several pools: pm_tick_many)
  // what the tests look at
  size_t known_nodes() const;
  std::optional<uint32_t> row_of(const Address& a) const;

 private:
  struct Row {
    uint32_t flags = 0, gpu_count = 0, gpu_mem = 0, gpu_class = 0, cpu_cores = 0, ram = 0, storage = 0;
    double lat = 0.0, lon = 0.0;
    bool operator==(const Row& o) const;
    bool operator!=(const Row& o) const { return !(*this == o); }
  };
  struct RowColumns {
    std::vector<uint32_t> flags, gpu_count, gpu_mem, gpu_class, cpu_cores, ram, storage, addr_rank;
    std::vector<double> lat, lon;
    void push(const Row& r, uint32_t rank);
    pm_worker_soa soa() const;
  };
  struct NodeTable {
    std::unordered_map<Address, uint32_t, AddressHash> index;
    std::vector<Address> addresses;
    std::vector<std::string> address_strings, p2p_ids;
    std::vector<Row> rows;
    std::vector<bool> present;
    std::vector<uint32_t> by_address;   // rows in address-string order (kept sorted: a new node is one binary search)
    std::vector<std::string> spec_models;
    std::unordered_map<std::string, uint32_t> spec_model_index;
  };

  void check(int32_t rc) const;
  // templates -> rows and alternatives appended to `alts`, requirement model strings appended to `req_models` (alt.model_row
  // indexes it); std::invalid_argument on a requirement string that does not parse
  static void pack_templates(const std::vector<NodeGroupConfiguration>& templates, std::vector<pm_config_row>& rows,
                             std::vector<pm_gpu_alt_row>& alts, std::vector<std::string>& req_models);
  void set_configs(const std::vector<NodeGroupConfiguration>& templates);
  void push_model_table(const NodeTable& nodes) const;
  static Row project(const OrchestratorNode& node, NodeTable& table, bool* new_model);
  static std::vector<uint32_t> address_ranks(const std::vector<uint32_t>& by_address, size_t known);
  std::optional<uint64_t> topology_mask(const Task& t) const;
  uint64_t engine_mask(const Task& t) const;
  void push_enabled(const std::vector<Task>& tasks);
  void sync_tasks_locked(std::vector<Task>& guard, std::vector<Task> tasks);
  void emit_group_webhooks();
  struct GroupSnapshot {
    std::vector<int32_t> group_of;   // per row: index into `groups` or -1
    std::vector<pm_group> groups;
    std::vector<uint32_t> members;
  };
  GroupSnapshot snapshot_groups(bool want_group_of) const;
  NodeGroup make_group(const NodeTable& t, const pm_group& g, const uint32_t* members) const;
  std::optional<uint32_t> row_of_address_text(const NodeTable& t, const std::string& text) const;

  pm_engine* engine_ = nullptr;
  // restore_groups' window: after a node and a task snapshot, before the first tick
  std::atomic<bool> nodes_synced_{false}, tasks_synced_{false}, ticked_{false};
  std::vector<NodeGroupConfiguration> templates_;   // caller order: the engine's configuration index
  std::vector<pm_config_row> config_rows_;          // what pm_set_configs was given (pm_host_config_order reads sizes + PM_R_HAS_REQ)
  std::atomic<uint64_t> enabled_mask_{0};           // "available_node_group_configs" as last pushed (push_enabled)
  mutable std::mutex group_meta_mu_;                // LEAF lock: never held across an engine call or another lock
  mutable std::unordered_map<uint64_t, int64_t> group_created_at_;
  std::vector<std::string> config_names_;
  std::vector<std::string> req_models_;   // requirement model strings, one per pm_gpu_alt_row.model_row
  mutable std::shared_mutex nodes_mu_;
  NodeTable nodes_;
  bool engine_rows_stale_ = false;   // an engine call of sync_nodes failed half-way: the next one re-sends every row
  // liveness: the beat column (last beat in ms per row, 0 = never): stored under the SHARED node lock, grown and read whole
  // under the exclusive one (sync_nodes, sweep_statuses)
  std::unique_ptr<std::atomic<uint64_t>[]> beats_;
  size_t beats_cap_ = 0;
  void grow_beats_locked(size_t rows);
  // set by enable_liveness to liveness_note (gpu_match_liveness.cpp; a pointer, so that gpu_match_plugin.cpp stays linkable
  // against an engine without the liveness exports): handle_status_change's write to the ledger
  void (*liveness_note_)(const GpuMatchPlugin&, uint32_t row, NodeStatus status) = nullptr;
  static void liveness_note(const GpuMatchPlugin& self, uint32_t row, NodeStatus status);
  // set by enable_admission to pm_liveness_sweep_beats (gpu_match_admission.cpp; a pointer, so that gpu_match_liveness.cpp stays
  // linkable against an engine without the admission exports): what sweep_statuses calls instead of pm_liveness_sweep
  int32_t (*sweep_call_)(pm_engine*, uint64_t, const uint64_t*, const uint64_t*, uint32_t, uint32_t*, uint32_t*) = nullptr;
  bool admission_on_ = false;  // (under the node lock)
  // address book (gpu_match_addresses.cpp; under the node lock): the rows' 20 bytes, bytes -> row, and how many rows render the
  // device's text.  book_sync_ is set by enable_address_book to book_sync (a pointer, as liveness_note_ is): sync_nodes' engine
  // calls — the bytes of the rows [first, end) or of every row, the rank, the texts of the rows that have none yet
  struct AddressBookState {
    bool on = false;
    std::vector<uint8_t> bytes;                         // 20 a row
    std::unordered_map<std::string, uint32_t> by_bytes; // (the 20 bytes as a string)
    size_t texts = 0;                                   // address_strings[0, texts) are the device's
    std::vector<uint32_t> ranks;                        // what pm_addresses_rank gave last
  };
  AddressBookState book_;
  void (*book_sync_)(GpuMatchPlugin&, uint32_t first, bool all) = nullptr;
  static void book_sync(GpuMatchPlugin& self, uint32_t first, bool all);
  // the new addresses of a snapshot, parsed (EngineError(PM_EINVAL) before anything changed); in the snapshot's order
  std::vector<std::array<uint8_t, 20>> book_parse_new_locked(const std::vector<OrchestratorNode>& snapshot) const;
  void book_admit_locked(uint32_t row, const std::array<uint8_t, 20>& bytes);
  // discovery sync (exclusive node lock): the endpoint column by row (ip empty = unknown: PM_EP_NONE), the interning map, the
  // endpoints of addresses without a row yet; last_status_change per row in ms, 0 = None.  Both grow lazily to the rows.
  struct EndpointColumn {
    std::vector<std::string> ip;
    std::vector<uint16_t> port;
    std::vector<uint32_t> id;
    std::unordered_map<std::string, uint32_t> intern;
    std::unordered_map<Address, std::pair<std::string, uint16_t>, AddressHash> pending;
  };
  EndpointColumn endpoints_;
  std::vector<uint64_t> stamps_;
  void note_stamp_locked(uint32_t row, uint64_t ms);
  uint32_t intern_endpoint_locked(const std::string& ip, uint16_t port);
  void fit_endpoints_locked();
  // metrics (gpu_match_metrics.cpp): the queue and the interner under metrics_mu_ (LOCK ORDER: nodes, metrics, the engine)
  struct MetricsQueue {
    std::vector<pm_mx_beat> beats;
    std::vector<pm_mx_entry> entries;
    std::unordered_map<std::string, uint32_t> series;                 // field -> series
    std::vector<std::pair<std::string, std::string>> keys;            // series -> (task id or "manual", cleaned label)
  };
  mutable std::mutex metrics_mu_;
  MetricsQueue metrics_;
  uint32_t metric_series_locked(const std::string& task_id, const std::string& label);
  void queue_metrics(const Address& address, uint32_t kind, const std::vector<MetricEntry>& entries);
  void flush_metrics_locked();
  std::vector<pm_mx_row> metric_rows_locked(const uint32_t* rows, uint32_t n);
  // rollout (gpu_match_rollout.cpp): the queue and the texts under rollout_mu_ (LOCK ORDER: nodes, tasks, rollout, the engine)
  struct RolloutQueue {
    std::vector<pm_ro_report> reports;
    std::unordered_map<uint64_t, std::string> texts;  // id -> reported text, of every id the last task report listed or reported since
  };
  mutable std::mutex rollout_mu_;
  RolloutQueue rollout_;
  void flush_rollout_locked();
  std::vector<pm_ro_task_row> rollout_task_rows_locked();
  std::string rollout_text_locked(uint64_t uid, uint32_t task) const;
  // node directory (gpu_match_directory.cpp): one window through the size query, checked against the node table
  std::vector<pm_dir_row> directory_locked(const pm_dir_query& q, uint32_t* total, uint32_t* counts) const;
  std::vector<std::string> nodes_of_status_locked(uint32_t status) const;
  // group directory (gpu_match_groupdir.cpp): the counters-only query, then one sized call; checked against the plugin's tables
  struct GroupWindow {
    pm_gdir_totals totals{};
    std::vector<pm_gdir_row> rows;
    std::vector<uint32_t> members;
  };
  GroupWindow group_directory_locked(const pm_gdir_query& q, uint32_t* by_config) const;
  std::vector<ListedNodeGroup> listed_groups_locked(const GroupWindow& w) const;
  // task directory (gpu_match_taskdir.cpp): the counters-only query, then one sized call; checked against the plugin's task list
  struct TaskWindow {
    pm_tdir_totals totals{};
    std::vector<pm_tdir_row> rows;
  };
  TaskWindow task_directory_locked(const pm_tdir_query& q, uint32_t* by_config) const;
  std::vector<ListedTask> listed_tasks_locked(const TaskWindow& w) const;
  // tick_dist's (the management loop's thread only): what pm_dist_configure was last told
  std::atomic<uint32_t> dist_rank_{0};   // (read by emit_group_webhooks on any thread)
  uint32_t dist_world_ = 1;
  size_t dist_rows_ = size_t(-1);
  void* dist_stream_ = nullptr;
  mutable std::shared_mutex tasks_mu_;
  std::vector<Task> tasks_;               // get_all_tasks order: the engine reports positions in this list
  UploadCounter upload_counter_;
  std::vector<std::shared_ptr<WebhookPlugin>> webhook_plugins_;
};

// store_context.task_store, as far as the scheduler uses it (task_store.rs:57-82)
class TaskStore {
 public:
  virtual ~TaskStore() = default;
  virtual std::vector<Task> get_all_tasks() = 0;
};

// get_task_topologies (node_groups/mod.rs:1407-1421): what create_task checks when the grouping plugin is active
// ("No topology found for task but grouping plugin is active", api/routes/task.rs:68-75): the task's allowed_topologies,
// empty when any Option on the way is None
std::vector<std::string> get_task_topologies(const Task& task);

// The storage route's file name (api/routes/storage.rs:147-185, after generate_file_name): ${NODE_GROUP_ID},
// ${NODE_GROUP_SIZE}, ${NODE_GROUP_INDEX} through get_node_group + get_idx_in_group when the node is in a group, then
// ${TOTAL_UPLOAD_COUNT_AFTER} / ${CURRENT_FILE_INDEX} from count_uploads(address, group id or "no-group") — the number of
// `upload:<address>:<group|no-group>:*` keys, which stays with the store (storage.rs:170-199).
// *group_id_out (may be null) = the group id the route keys its upload counter by, empty when the node is in no group.
std::string upload_file_name(const GpuMatchPlugin& plugin, const std::string& file_name, const std::string& address,
                             const std::function<uint64_t(const std::string& address, const std::string& group_or_no_group)>& count_uploads,
                             std::string* group_id_out = nullptr);

class Scheduler {
 public:
  // Scheduler::new (scheduler/mod.rs:14-24): an empty chain gets the NewestTaskPlugin
  Scheduler(std::shared_ptr<TaskStore> task_store, std::vector<std::shared_ptr<SchedulerPlugin>> plugins);
  // scheduler/mod.rs:26-76; `now` feeds ${TIMESTAMP} in volume mounts (chrono::Utc::now() in the reference)
  std::optional<Task> get_task_for_node(const Address& node_address, int64_t now = 0);

 private:
  std::shared_ptr<TaskStore> task_store_;
  std::vector<std::shared_ptr<SchedulerPlugin>> plugins_;
};

}  // namespace orchestrator
#endif
