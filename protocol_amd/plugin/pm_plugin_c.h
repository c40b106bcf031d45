/* pm_plugin_c.h — a flat C face of the compiled host side (gpu_match_plugin.hpp), so that the Python test harness can
 * drive the C++ GpuMatchPlugin + Scheduler with the scenarios it drives tests/shim_replay.py with, against the oracle
 * on a GPU and against tests/cpp/mock_engine.cpp without one.  Not part of the drop-in boundary (that is
 * include/pm_engine.h below the plugin, and the reference's own Rust interface above it): a test driver's handle on a
 * C++ object.  One pmx_plugin = a GpuMatchPlugin, a recording WebhookPlugin, a TaskStore whose list the caller sets,
 * and a Scheduler whose chain is headed by the plugin.  Every call returns 0 or -1 (pmx_last_error says why); strings
 * are NUL-terminated UTF-8; text results follow the two-call convention of the pm_host_* helpers (*needed = strlen + 1;
 * -2 when cap is too small, nothing written). */
#ifndef PM_PLUGIN_C_H
#define PM_PLUGIN_C_H

#include <stddef.h>
#include <stdint.h>

#include "pm_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pmx_plugin pmx_plugin;

typedef struct {
  const char* name;
  uint32_t min_group_size, max_group_size;
  const char* compute_requirements; /* NULL = None */
} pmx_config;

/* NodeStatus, in the reference's order (orchestrator/src/models/node.rs:75-85) */
enum { PMX_DISCOVERED = 0, PMX_WAITING_FOR_HEARTBEAT, PMX_HEALTHY, PMX_UNHEALTHY, PMX_DEAD, PMX_EJECTED, PMX_BANNED, PMX_LOW_BALANCE };

/* one OrchestratorNode: `has` says which Options are Some — the PM_W_* bits of include/pm_engine.h minus PM_W_HEALTHY
 * (the status says that) */
typedef struct {
  const char* address; /* address.to_string() */
  uint32_t status;     /* PMX_* */
  uint32_t has;        /* PM_W_HAS_SPECS | PM_W_HAS_GPU | ... | PM_W_HAS_P2P | PM_W_HAS_LOC */
  const char* p2p_id;
  uint32_t gpu_count, gpu_memory_mb;
  const char* gpu_model;
  uint32_t cpu_cores, ram_mb, storage_gb;
  double latitude, longitude;
} pmx_node;

typedef struct {
  const char* id; /* Uuid text */
  const char* name;
  int64_t created_at;
  int32_t n_topologies; /* -1 = no allowed_topologies (any None on the way) */
  const char* const* topologies;
  uint32_t n_env;
  const char* const* env_keys;
  const char* const* env_values;
  int32_t n_cmd; /* -1 = None */
  const char* const* cmd;
  int32_t n_mounts; /* -1 = None */
  const char* const* mount_host;
  const char* const* mount_container;
} pmx_task;

const char* pmx_last_error(void);
int32_t pmx_create(const pmx_config* cfgs, uint32_t n, int32_t device, pmx_plugin** out);
void pmx_destroy(pmx_plugin*);
pm_engine* pmx_engine(pmx_plugin*); /* the plugin's engine (borrowed): pm_get_groups & co. for the parity checks */
void pmx_set_upload_count(pmx_plugin*, uint64_t n); /* what the upload counter answers (the Redis key count) */
void pmx_set_republish_on_insert(pmx_plugin*, uint32_t on);

int32_t pmx_sync_nodes(pmx_plugin*, const pmx_node* nodes, uint32_t n);
/* the store's list := tasks (get_all_tasks order), then GpuMatchPlugin::sync_tasks */
int32_t pmx_sync_tasks(pmx_plugin*, const pmx_task* tasks, uint32_t n);
/* TaskStore::add_task: the store's list gets the task at its created_at-descending place, then the observer runs */
int32_t pmx_on_task_created(pmx_plugin*, const pmx_task* task);
/* TaskStore::delete_task by id, then the observer (unknown id: -1) */
int32_t pmx_on_task_deleted(pmx_plugin*, const char* task_id);
int32_t pmx_handle_status_change(pmx_plugin*, const char* address, uint32_t status);
int32_t pmx_tick(pmx_plugin*, pm_stats* stats);
int32_t pmx_row_of(pmx_plugin*, const char* address, uint32_t* row); /* -1 if the plugin does not know the address */
uint32_t pmx_known_nodes(pmx_plugin*);
uint32_t pmx_store_loads(pmx_plugin*); /* how often the scheduler asked the store for its task list */

/* Scheduler::get_task_for_node.  Text: empty = None; else lines "id\t<id>", "name\t<name>", "env\t<key>\t<value>" (key
 * order), "cmd\t<arg>", "mount\t<host>\t<container>"; backslash, tab and newline inside a field are \\ \t \n. */
int32_t pmx_get_task_for_node(pmx_plugin*, const char* address, int64_t now, char* out, size_t cap, size_t* needed);
/* the webhooks sent since the last successful call, one per line: "created|destroyed\t<group id>\t<configuration
 * name>\t<node>\t<node>..." */
int32_t pmx_take_webhooks(pmx_plugin*, char* out, size_t cap, size_t* needed);

/* ---- the plugin's read surface (node_groups/mod.rs:324-434, :1002-1065: what the API routes call).  A group is one line
 * "<id>\t<configuration name>\t<created_at ms>\t<node>\t<node>..." (nodes in BTreeSet<String> order). */
void pmx_set_clock(pmx_plugin*, int64_t now_ms); /* what the plugin's clock answers from now on (NodeGroup.created_at) */
int32_t pmx_get_all_groups(pmx_plugin*, char* out, size_t cap, size_t* needed);               /* sorted by id text */
int32_t pmx_get_group_by_id(pmx_plugin*, const char* group_id, char* out, size_t cap, size_t* needed); /* empty = None */
/* get_node_group + get_idx_in_group: empty = None, else "<idx>\t" in front of the group line */
int32_t pmx_get_node_group(pmx_plugin*, const char* address, char* out, size_t cap, size_t* needed);
/* one line per asked address, in the order asked: "<address>\t-" (None) or "<address>\t" + the group line */
int32_t pmx_get_node_groups_batch(pmx_plugin*, const char* const* addresses, uint32_t n, char* out, size_t cap, size_t* needed);
int32_t pmx_get_all_node_group_mappings(pmx_plugin*, char* out, size_t cap, size_t* needed); /* "<address>\t<group id>", by address */
/* get_all_configuration_templates (available_only = 0) / get_available_configurations (1): "<name>\t<min>\t<max>\t<requirements or ->" */
int32_t pmx_get_configurations(pmx_plugin*, uint32_t available_only, char* out, size_t cap, size_t* needed);
int32_t pmx_dissolve_group(pmx_plugin*, const char* group_id);
/* the storage route's file name (api/routes/storage.rs:147-207) through get_node_group + get_idx_in_group; the key count is
 * pmx_set_upload_count's value.  Two lines: the name, then the group id the route keys its counter by ("no-group" if none). */
int32_t pmx_upload_file_name(pmx_plugin*, const char* file_name, const char* address, char* out, size_t cap, size_t* needed);

/* ---- restart and switch-over (pm_plugin_restore_c.cpp): GpuMatchPlugin::restore_groups / group_tasks / group_id_state.
 * groups: group lines in the pmx_get_all_groups format, one per line; group_tasks: lines "<group id>\t<task id>";
 * has_id_state = 0: no id_state (None).  The report waits for pmx_take_restore_report: "dropped\t<id>\t<reason>" lines,
 * then "task_cleared\t<id>" lines. */
int32_t pmx_restore_groups(pmx_plugin*, const char* groups, const char* group_tasks, uint32_t has_id_state, uint64_t id_state);
int32_t pmx_take_restore_report(pmx_plugin*, char* out, size_t cap, size_t* needed);
int32_t pmx_group_tasks(pmx_plugin*, char* out, size_t cap, size_t* needed); /* "<group id>\t<task id>" lines, by group id */
int32_t pmx_group_id_state(pmx_plugin*, uint64_t* state);
void pmx_set_multi_gpu(pmx_plugin*, uint32_t on); /* GpuMatchPlugin::multi_gpu */

/* ---- diagnostics (pm_plugin_report_c.cpp): GpuMatchPlugin::explain_node / configuration_report / task_report.
 *   pmx_explain_node           empty = the node table does not hold the address; else "state\t<state>", then one line
 *                              "<configuration name>\t<reason name>" per configuration (constructor order)
 *   pmx_configuration_report   one line per configuration: "<name>\t<enabled 0|1>\t<eligible_meets>\t<idle_meets>\t<groups>\t
 *                              <members>\t<groups_without_task>\t<tasks_allowing>\t<why[0]>\t...\t<why[9]>"
 *   pmx_task_report            "<task id>\t<groups_running>\t<workers_running>\t<groups_allowed>", by task id */
int32_t pmx_explain_node(pmx_plugin*, const char* address, char* out, size_t cap, size_t* needed);
int32_t pmx_configuration_report(pmx_plugin*, char* out, size_t cap, size_t* needed);
int32_t pmx_task_report(pmx_plugin*, char* out, size_t cap, size_t* needed);

/* ---- group geography (pm_plugin_spread_c.cpp): GpuMatchPlugin::group_spread / configuration_spread / force_regroup.
 *   pmx_group_spread           one line per live group, by group id text: "<group id>\t<located>\t<ring_hops>\t<far_a>\t<far_b>\t
 *                              <hop_from>\t<diameter_km>\t<ring_km>\t<longest_hop_km>" (addresses, "-" = none; %.17g)
 *   pmx_configuration_spread   one line per configuration: "<name>\t<groups>\t<measured>\t<hist[0]>\t...\t<hist[4]>\t
 *                              <max_diameter_km>\t<max_hop_km>\t<sum_diameter_m>\t<sum_ring_m>"
 *   pmx_force_regroup          *found = 0: no configuration has this name (the route's 404), nothing done */
int32_t pmx_group_spread(pmx_plugin*, char* out, size_t cap, size_t* needed);
int32_t pmx_configuration_spread(pmx_plugin*, char* out, size_t cap, size_t* needed);
int32_t pmx_force_regroup(pmx_plugin*, const char* configuration_name, uint32_t metric, double threshold_km, int32_t* found,
                          uint32_t* dissolved_groups, uint32_t* affected_nodes);

/* ---- nearest candidates (pm_plugin_near_c.cpp): GpuMatchPlugin::nearest_nodes.  address NULL: from the seed the next carve
 * would take for the configuration.  *found = 0: the node table does not hold the address (empty text).  Else the first line
 * is "origin\t<address, "-" = the seed rule found no candidate>\t<candidates>\t<located>", then one line "<address>\t<km>"
 * per node, nearest first (%.17g; "-" = not measured).  An unknown configuration name is an error (-1). */
int32_t pmx_nearest_nodes(pmx_plugin*, const char* address, const char* configuration_name, uint32_t pool, uint32_t k,
                          int32_t* found, char* out, size_t cap, size_t* needed);

/* ---- probing configurations (pm_plugin_probe_c.cpp): GpuMatchPlugin::probe_configurations / configuration_overlap.
 *   pmx_probe_configurations   one line per probe, in the given order: "<name>\t<eligible_meets>\t<idle_meets>\t<idle_located>\t
 *                              <idle_exclusive>\t<groups_max>\t<groups_exclusive>\t<why[0]>\t...\t<why[9]>", then one field
 *                              "\t<installed configuration name>=<idle nodes that meet both>" per installed configuration
 *                              (constructor order).  A requirement string that does not parse is an error (-1).
 *   pmx_configuration_overlap  one line per installed configuration a: "<name of a>\t<idle[a][0]>\t...\t<idle[a][C - 1]>" */
int32_t pmx_probe_configurations(pmx_plugin*, const pmx_config* probes, uint32_t n, char* out, size_t cap, size_t* needed);
int32_t pmx_configuration_overlap(pmx_plugin*, char* out, size_t cap, size_t* needed);

/* ---- change feed (pm_plugin_changes_c.cpp): GpuMatchPlugin::enable_change_feed / changed_nodes.  The text of
 * pmx_changed_nodes: the first line is "resync\t<0|1>", then one line "<address>\t<what>" per node whose published row changed
 * since the last drain, in row order (what: the OR of PM_CHG_GROUP = 1, PM_CHG_RING = 2, PM_CHG_TASK = 4, decimal).  The drain
 * empties the feed, so its text is held until a call's buffer has taken it: the size query (out NULL, cap 0) and the call
 * behind it hand over one drain. */
int32_t pmx_enable_change_feed(pmx_plugin*, int32_t on);
int32_t pmx_changed_nodes(pmx_plugin*, char* out, size_t cap, size_t* needed);

/* ---- liveness (pm_plugin_liveness_c.cpp): GpuMatchPlugin::enable_liveness / beat / sweep_statuses.  out_of_pool: the addresses
 * is_node_in_pool is false for (none = every node in the pool).  The text of pmx_sweep_statuses: one line
 * "<address>\t<old status>\t<new status>" per transition, in row order (NodeStatus as its number, models/node.rs:75-85).  A
 * sweep commits, so its text is held until a call's buffer has taken it: the size query (out NULL, cap 0) and the call behind
 * it hand over one sweep. */
int32_t pmx_enable_liveness(pmx_plugin*, uint32_t missing_heartbeat_threshold);
int32_t pmx_beat(pmx_plugin*, const char* address, uint64_t now_ms);
int32_t pmx_sweep_statuses(pmx_plugin*, uint64_t now_ms, const char* const* out_of_pool, uint32_t n_out_of_pool, char* out,
                           size_t cap, size_t* needed);

/* ---- metrics (pm_plugin_metrics_c.cpp): GpuMatchPlugin::enable_metrics / beat_metrics / store_metrics / store_manual_metric /
 * delete_metric / clear_metrics / flush_metrics and the reads.  A beat's entries come as three parallel arrays (task id, label,
 * value); address "0x000...0" is the manual row.  The writes queue; pmx_flush_metrics and every read send the queue in one ingest.
 * The texts, values as C's "%a" (every bit): pmx_aggregate_metrics (task_id NULL = all tasks) "<label>\t<sum>" per label in label
 * order; pmx_metrics_for_node "<task id>\t<label>\t<value>"; pmx_synced_metrics "<address>\t<task id>\t<task name>\t<label>\t
 * <value>\t<group id or ->\t<configuration name or ->" per entry, the manual row's first, then ascending (row, series), the task
 * names from the two parallel arrays ("unknown" where they have none). */
int32_t pmx_enable_metrics(pmx_plugin*);
int32_t pmx_beat_metrics(pmx_plugin*, const char* address, const char* const* task_ids, const char* const* labels,
                         const double* values, uint32_t n);
int32_t pmx_store_metrics(pmx_plugin*, const char* address, const char* const* task_ids, const char* const* labels,
                          const double* values, uint32_t n);
int32_t pmx_store_manual_metric(pmx_plugin*, const char* label, double value);
int32_t pmx_delete_metric(pmx_plugin*, const char* task_id, const char* label, const char* address);
int32_t pmx_clear_metrics(pmx_plugin*, const char* address);
int32_t pmx_flush_metrics(pmx_plugin*);
int32_t pmx_aggregate_metrics(pmx_plugin*, const char* task_id, char* out, size_t cap, size_t* needed);
int32_t pmx_metrics_for_node(pmx_plugin*, const char* address, char* out, size_t cap, size_t* needed);
int32_t pmx_synced_metrics(pmx_plugin*, const char* const* task_ids, const char* const* task_names, uint32_t n_tasks, char* out,
                           size_t cap, size_t* needed);

/* ---- rollout (pm_plugin_rollout_c.cpp): GpuMatchPlugin::enable_rollout / report_task / flush_rollout and the reads.  task_id and
 * task_state may be NULL (None): update_node_task's match — both present set the report, anything else clears it.  The writes
 * queue; pmx_flush_rollout and every read send the queue in one ingest.  The texts, numbers in decimal:
 * pmx_nodes_per_task "<task id>\t<task name or unknown>\t<count>" per reported id; pmx_task_rollout "<task id>\t<task name>\t
 * <position or ->\t<groups>\t<groups converged>\t<assigned>\t<converged>" and the eight reporter counts; pmx_group_rollout
 * "<group id>\t<configuration name>\t<task id>\t<size>", the eight same counts, other, silent; pmx_rollout_nodes "<address>\t
 * <class>\t<state or ->\t<reported task id or ->" ascending by row.  pmx_rollout_summary fills the engine's struct. */
int32_t pmx_enable_rollout(pmx_plugin*);
int32_t pmx_report_task(pmx_plugin*, const char* address, const char* task_id /* NULL = None */, const char* task_state /* NULL = None */);
int32_t pmx_flush_rollout(pmx_plugin*);
int32_t pmx_nodes_per_task(pmx_plugin*, char* out, size_t cap, size_t* needed);
int32_t pmx_rollout_summary(pmx_plugin*, pm_ro_summary* out);
int32_t pmx_task_rollout(pmx_plugin*, char* out, size_t cap, size_t* needed);
int32_t pmx_group_rollout(pmx_plugin*, char* out, size_t cap, size_t* needed);
int32_t pmx_rollout_nodes(pmx_plugin*, uint32_t class_mask, char* out, size_t cap, size_t* needed);

/* ---- node directory (pm_plugin_directory_c.cpp): GpuMatchPlugin::list_nodes / status_counts / uninvited_nodes / dead_nodes
 * (needs pmx_enable_liveness).  The texts, numbers in decimal: pmx_list_nodes "total\t<total>", then "count\t<status name>\t
 * <count>" per status that occurs (in name order), then "<address>\t<status name>\t<unhealthy counter>\t<task state or ->\t<group
 * id or ->\t<group size or ->\t<configuration name or ->" per node of the window, in listing order; pmx_status_counts "<lowercase
 * status name>\t<count>" per status that occurs; pmx_uninvited_nodes / pmx_dead_nodes one address a line, in row order.
 * order: 0 = by row, 1 = by address; limit UINT32_MAX = to the end. */
int32_t pmx_list_nodes(pmx_plugin*, uint32_t include_dead, uint32_t order, uint32_t offset, uint32_t limit, char* out, size_t cap,
                       size_t* needed);
int32_t pmx_status_counts(pmx_plugin*, char* out, size_t cap, size_t* needed);
int32_t pmx_uninvited_nodes(pmx_plugin*, char* out, size_t cap, size_t* needed);
int32_t pmx_dead_nodes(pmx_plugin*, char* out, size_t cap, size_t* needed);

/* ---- group directory (pm_plugin_groupdir_c.cpp): GpuMatchPlugin::list_groups / group_counts / degraded_groups.  The texts,
 * numbers in decimal: pmx_list_groups "total\t<total>\t<members total>", then per group of the window, in listing order,
 * "<group id>\t<configuration name>\t<size>\t<health: lost, degraded, sound or ->\t<rollout: no_task, converged, rolling or ->\t
 * <task id or ->\t<created_at>\t<address>,<address>,..." (the nodes in member order); pmx_degraded_groups the same lines without
 * the first; pmx_group_counts "<configuration name>\t<count>" per configuration that has a group.  order: 0 = by slot, 1 = by
 * id text, 2 = by size, largest first; limit UINT32_MAX = to the end; a class mask other than 7 needs its ledger. */
int32_t pmx_list_groups(pmx_plugin*, uint64_t config_mask, uint32_t holds, uint32_t size_min, uint32_t size_max, uint32_t health_mask,
                        uint32_t rollout_mask, uint32_t order, uint32_t offset, uint32_t limit, char* out, size_t cap, size_t* needed);
int32_t pmx_group_counts(pmx_plugin*, char* out, size_t cap, size_t* needed);
int32_t pmx_degraded_groups(pmx_plugin*, char* out, size_t cap, size_t* needed);

/* ---- task directory (pm_plugin_taskdir_c.cpp): GpuMatchPlugin::list_tasks / task_counts / starved_tasks /
 * orchestrator_statistics.  The texts, numbers in decimal: pmx_list_tasks "total\t<total>\t<tasks>", then per task of the window, in
 * listing order, "<task id>\t<name>\t<serve: running, waiting, starved>\t<rollout: unheld, converged, rolling or ->\t<groups
 * allowed>\t<groups running>\t<workers running>\t<groups converged>\t<converged>\t<reporters>"; pmx_starved_tasks the same lines
 * without the first; pmx_task_counts "tasks\t<n>", "serve\t<running>\t<waiting>\t<starved>", "rollout\t<unheld>\t<converged>\t
 * <rolling>", "unrestricted\t<n>", "workers_running\t<n>", "reporters\t<n>", "orphans\t<ids>\t<reporters>", then
 * "<configuration name>\t<tasks allowing it>" per configuration some task allows; pmx_orchestrator_statistics "nodes\t<status>\t
 * <count>" per status some node has, "tasks_count\t<n>", "nodes_per_task\t<task id>\t<name or unknown>\t<count>" per task with
 * reporters, "groups_count\t<configuration name>\t<count>" per configuration that has a group (needs pmx_enable_liveness and
 * pmx_enable_rollout).  order: 0 = the list's, newest first, 1 = oldest first, 2 = by assigned workers, 3 = by reporters, largest
 * first; limit UINT32_MAX = to the end; a rollout mask other than 7 and order 3 need the rollout ledger. */
int32_t pmx_list_tasks(pmx_plugin*, uint64_t config_mask, uint32_t serve_mask, uint32_t rollout_mask, uint32_t workers_min,
                       uint32_t workers_max, uint32_t order, uint32_t offset, uint32_t limit, char* out, size_t cap, size_t* needed);
int32_t pmx_task_counts(pmx_plugin*, char* out, size_t cap, size_t* needed);
int32_t pmx_starved_tasks(pmx_plugin*, char* out, size_t cap, size_t* needed);
int32_t pmx_orchestrator_statistics(pmx_plugin*, char* out, size_t cap, size_t* needed);

/* ---- address book (pm_plugin_addresses_c.cpp): GpuMatchPlugin::enable_address_book / invite_digests.  With the book on every
 * address text of this face is the EIP-55 text the device computed, and an address passed in is found under any spelling.  The
 * text of pmx_invite_digests (needs pmx_enable_liveness: the nodes are pmx_uninvited_nodes', in its order): "<address>\t<nonce>\t
 * <digest>\t<signing hash>" per node, 64 lower-case hex digits each; this face draws the nonces itself — a test driver's
 * plumbing: splitmix64 from nonce_seed, four little-endian words a nonce — where the C++ method takes the caller's source. */
int32_t pmx_enable_address_book(pmx_plugin*);
int32_t pmx_invite_digests(pmx_plugin*, uint32_t domain_id, uint32_t pool_id, uint64_t nonce_seed, uint64_t expiration_s, char* out,
                           size_t cap, size_t* needed);

/* ---- request gate (pm_plugin_gate_c.cpp): GpuMatchPlugin::verify_requests (needs pmx_enable_address_book).  requests: one line
 * per request, "<signature text>\t<x-address text>\t<message>" (the message is path + payload string; it holds no line break in
 * this face).  The text: per request "<code>\t<row or ->\t<status or ->\t0x<recovered address, 40 lower-case hex digits>", code
 * one of bad_signature, no_key, bad_address, mismatch, unknown, ejected, banned, ok; then "counts" and the eight census words
 * in that order. */
int32_t pmx_verify_requests(pmx_plugin*, const char* requests, char* out, size_t cap, size_t* needed);

/* ---- request gate: admission (pm_plugin_admission_c.cpp): GpuMatchPlugin::enable_admission / admit_requests (needs
 * pmx_enable_address_book).  requests: one line per request, "<signature text>\t<x-address text>\t<timestamp or ->\t<nonce
 * or ->\t<1 = /heartbeat, else 0>\t<message>".  The text: pmx_verify_requests' lines, the code one of its eight or
 * rate_limited, expired, bad_nonce, replay, no_nonce; then "counts" and the thirteen census words in that order. */
int32_t pmx_enable_admission(pmx_plugin*);
int32_t pmx_admit_requests(pmx_plugin*, const char* requests, uint64_t now_ms, char* out, size_t cap, size_t* needed);

/* ---- discovery sync (pm_plugin_discovery_c.cpp): GpuMatchPlugin::set_endpoint / sync_discovery (needs pmx_enable_liveness).  The
 * text of pmx_sync_discovery: one line per sighting, in order: "<address>\tadmitted\t<cnt>", "<address>\tskipped\t<cnt>" or
 * "<address>\tsynced\t<cnt>\t<old status>\t<final status>\t<ops>\t<old>><new>,..." — cnt = the Healthy other nodes on the sighting's
 * endpoint, ops = the letters of i (ip rewritten), l (location new), s (specs rewritten), n (last_status_change is now), the
 * updates as the handlers saw them.  Admitted nodes are returned, not appended: the next pmx_sync_nodes brings their rows.  A sync
 * commits, so its text is held until a call's buffer has taken it, as pmx_sweep_statuses' is. */
typedef struct pmx_sighting {
  const char* address;
  const char* ip_address;
  uint16_t port;
  uint8_t is_validated, is_provider_whitelisted, is_active, location_new, specs_differ, balance_zero;
  uint64_t last_updated_ms; /* 0 = None */
} pmx_sighting;
int32_t pmx_set_endpoint(pmx_plugin*, const char* address, const char* ip_address, uint16_t port);
int32_t pmx_sync_discovery(pmx_plugin*, uint64_t now_ms, const pmx_sighting* sightings, uint32_t n, uint32_t max_same_endpoint,
                           char* out, size_t cap, size_t* needed);

#ifdef __cplusplus
}
#endif
#endif
