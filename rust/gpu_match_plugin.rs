//! GpuMatchPlugin — the third `SchedulerPlugin` variant: binds libpm_engine.so (include/pm_engine.h, ABI v3).
//!
//! SOURCE ONLY: this image has no cargo/rustc, so this file has never been compiled.  It is the binding a
//! maintainer adds under crates/orchestrator/src/plugins/gpu_match/mod.rs, next to
//! crates/orchestrator/src/plugins/mod.rs:60-79 (see INTEGRATION.md for the enum arms and build.rs).
//!
//! The plugin owns an opaque `pm_engine*`.  The group-management loop calls `tick()` instead of
//! `try_form_new_groups` + `try_merge_solo_groups` (node_groups/mod.rs:180-203); `filter_tasks` becomes a
//! lock-free lookup of the table published by the last tick (scheduler_impl.rs:11-110).
//!
//! The READ SURFACE the API routes call on `AppState.node_groups_plugin` (node_groups/mod.rs:324-434, :1002-1065) is
//! here with the reference's names, signatures and result types, so the routes compile unchanged against
//! `Option<Arc<GpuMatchPlugin>>` (INTEGRATION.md "The routes"): get_all_groups, get_group_by_id,
//! get_all_node_group_mappings, get_node_group, get_node_groups_batch, get_idx_in_group,
//! get_available_configurations, get_all_configuration_templates, dissolve_group.  The engine's host-side group list
//! is the store behind them (the reference reads Redis).
//!
//! Row identity.  The engine keys workers, groups and claims by ROW INDEX.  `NodeStore::get_nodes` is Redis
//! SMEMBERS order followed by a status sort (node_store.rs:195-206), so the position of a node in that Vec moves
//! whenever anybody's status changes.  The plugin therefore keeps a stable `address -> row` map: a node seen for the
//! first time is APPENDED (pm_append_workers), a known node whose projection changed is rewritten in place
//! (pm_update_workers), a node that left the store is tombstoned (PM_W_HEALTHY cleared + dissolve, never removed).
//! The order in which nodes first appear is the engine's input order (the reference's own tie-break is the
//! unspecified SMEMBERS order).
#![allow(non_camel_case_types, dead_code)]

use std::collections::{BTreeSet, HashMap};
use std::ffi::{c_char, CStr, CString};
use std::os::raw::c_void;
use std::sync::atomic::{AtomicBool, AtomicU32, AtomicU64, Ordering};

use alloy::primitives::Address;
use anyhow::{anyhow, Error, Result};
use shared::models::node::{ComputeRequirements, ComputeSpecs};
use shared::models::task::Task;

use crate::models::node::{NodeStatus, OrchestratorNode};
use crate::plugins::node_groups::{NodeGroup, NodeGroupConfiguration};
use crate::plugins::webhook::WebhookPlugin;

pub const PM_NONE: u32 = 0xFFFF_FFFF;
pub const PM_ABI_VERSION: u32 = 3;
const PM_EINVAL: i32 = -1;
const PM_ESTATE: i32 = -4;
const PM_ERANGE: i32 = -5;

#[repr(C)]
pub struct pm_engine_config {
    pub abi_version: u32,
    pub device: i32,
    pub proximity_enabled: u32,
    pub switching_enabled: u32,
    pub prefer_larger_groups: u32,
    pub chooser: u32,
    pub chooser_seed: u64,
    pub group_id_seed: u64,
    pub debug_uncertain_every: u32,
    pub sweep_variant: u32,
    pub carve_variant: u32,
    pub time_proposer: u32,
}

#[repr(C)]
pub struct pm_worker_soa {
    pub n: u32,
    pub flags: *const u32,
    pub gpu_count: *const u32,
    pub gpu_mem_mb: *const u32,
    pub gpu_model_class: *const u32,
    pub cpu_cores: *const u32,
    pub ram_mb: *const u32,
    pub storage_gb: *const u32,
    pub price: *const u32,
    pub addr_rank: *const u32,
    pub lat: *const f64,
    pub lon: *const f64,
}

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct pm_config_row {
    pub flags: u32,
    pub cpu_cores: u32,
    pub ram_mb: u32,
    pub storage_gb: u32,
    pub alt_begin: u32,
    pub alt_count: u32,
    pub min_group_size: u32,
    pub max_group_size: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct pm_gpu_alt_row {
    pub flags: u32,
    pub count: u32,
    pub memory_mb: u32,
    pub memory_mb_min: u32,
    pub memory_mb_max: u32,
    pub total_memory_min: u32,
    pub total_memory_max: u32,
    pub model_row: u32,
}

#[repr(C)]
pub struct pm_task_soa {
    pub n: u32,
    pub topo_mask: *const u64,
    pub created_at: *const i64,
    pub uid: *const u64,
}

/// include/pm_engine.h: one entry of the group life-cycle feed (kind 1 = created, 2 = destroyed)
/// pm_verify_requests' answer for one request (include/pm_engine.h "request gate")
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct pm_rq_verdict {
    pub code: u32,
    pub row: u32,
    pub status: u8,
    pub _pad: [u8; 3],
    pub address: [u8; 20],
}
pub const RQ_BAD_SIGNATURE: u32 = 0;
pub const RQ_NO_KEY: u32 = 1;
pub const RQ_BAD_ADDRESS: u32 = 2;
pub const RQ_MISMATCH: u32 = 3;
pub const RQ_UNKNOWN: u32 = 4;
pub const RQ_EJECTED: u32 = 5;
pub const RQ_BANNED: u32 = 6;
pub const RQ_OK: u32 = 7;
pub const RQ_N_CODES: usize = 8;
// ... and what pm_admit_requests appends (include/pm_engine.h "request gate: admission")
pub const RQ_RATE_LIMITED: u32 = 8;
pub const RQ_EXPIRED: u32 = 9;
pub const RQ_BAD_NONCE: u32 = 10;
pub const RQ_REPLAY: u32 = 11;
pub const RQ_NO_NONCE: u32 = 12;
pub const AD_N_CODES: usize = 13;
pub const RQ_FLAG_NO_TIMESTAMP: u8 = 2;
pub const RQ_FLAG_NO_NONCE: u8 = 4;
pub const RQ_FLAG_BEAT: u8 = 8;

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct pm_group_event {
    pub group_id: u64,
    pub kind: u32,
    pub config: u32,
    pub member_begin: u32,
    pub n_members: u32,
}

/// include/pm_engine.h: one group of pm_get_groups / pm_get_group_by_id / pm_get_group_of_worker
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct pm_group {
    pub id: u64,
    pub config: u32,
    pub n_members: u32,
    pub member_begin: u32,
    pub task: u32,
}

#[repr(C)]
#[derive(Default)]
pub struct pm_assignment {
    pub task: u32,
    pub group_slot: u32,
    pub group_index: u32,
    pub group_size: u32,
    pub next_worker: u32,
    pub group_id: u64,
}

#[repr(C)]
#[derive(Default)]
pub struct pm_stats {
    pub ms_compat: f32, pub ms_carve: f32, pub ms_merge: f32, pub ms_sweep: f32, pub ms_publish: f32,
    pub ms_total: f32, pub ms_compat_kernel: f32, pub ms_carve_kernel: f32, pub ms_sweep_kernel: f32,
    pub n_groups: u32, pub n_formed: u32, pub n_merged: u32, pub carve_steps: u32, pub carve_fast_steps: u32,
    pub host_resolved_steps: u32, pub carve_launches: u32, pub pair_evals: u64, pub carve_cand_sum: u64,
    pub ms_propose_kernel: f32, pub proposals: u32, pub propose_keys: u64,
}

/// pm_config_report_row (include/pm_engine.h)
#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct pm_config_report_row {
    pub enabled: u32,
    pub eligible_meets: u32,
    pub idle_meets: u32,
    pub why: [u32; 10],
    pub groups: u32,
    pub members: u32,
    pub groups_without_task: u32,
    pub tasks_allowing: u32,
}

/// pm_group_spread_row (include/pm_engine.h)
#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct pm_group_spread_row {
    pub located: u32,
    pub ring_hops: u32,
    pub far_a: u32,
    pub far_b: u32,
    pub hop_from: u32,
    pub _pad: u32,
    pub diameter_km: f64,
    pub ring_km: f64,
    pub longest_hop_km: f64,
}

/// pm_config_spread_row (include/pm_engine.h)
#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct pm_config_spread_row {
    pub groups: u32,
    pub measured: u32,
    pub hist: [u32; 5],
    pub _pad: u32,
    pub max_diameter_km: f64,
    pub max_hop_km: f64,
    pub sum_diameter_m: u64,
    pub sum_ring_m: u64,
}

/// pm_near_query / pm_near_row (include/pm_engine.h)
#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct pm_near_query {
    pub origin: u32,
    pub config: u32,
}

#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct pm_near_row {
    pub origin: u32,
    pub n: u32,
    pub candidates: u32,
    pub located: u32,
}

/// pm_nearest_workers' pools (PM_NEAR_*), the seed origin and the largest k
pub const NEAR_IDLE: u32 = 0;
pub const NEAR_ELIGIBLE: u32 = 1;
pub const NEAR_SEED: u32 = 0xFFFF_FFFE;
pub const NEAR_MAX_K: u32 = 256;

/// pm_probe_row (include/pm_engine.h): what a configuration that is not installed would find right now
#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct pm_probe_row {
    pub why: [u32; 10],
    pub eligible_meets: u32,
    pub idle_meets: u32,
    pub idle_located: u32,
    pub idle_exclusive: u32,
    pub groups_max: u32,
    pub groups_exclusive: u32,
}

/// pm_change_row (include/pm_engine.h): a worker whose published row changed, and how
#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct pm_change_row {
    pub worker: u32,
    pub what: u32,
}

/// the bits of pm_change_row.what (PM_CHG_*) and pm_drain_assignment_changes' flag
pub const CHG_GROUP: u32 = 1;
pub const CHG_RING: u32 = 2;
pub const CHG_TASK: u32 = 4;
pub const CHANGES_RESYNC: u32 = 1;

/// pm_live_row (include/pm_engine.h): a row the last liveness sweep listed
#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct pm_live_row {
    pub worker: u32,
    pub old_status: u8,
    pub new_status: u8,
    pub _pad: u16,
    pub counter: u32,
}

/// pm_mx_beat / pm_mx_entry / pm_mx_row (include/pm_engine.h): the metrics ledger's batch and its listing
#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct pm_mx_beat {
    pub row: u32,
    pub kind: u32,
    pub first: u32,
    pub n: u32,
}

#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct pm_mx_entry {
    pub series: u32,
    pub flags: u32,
    pub value: f64,
}

#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct pm_mx_row {
    pub row: u32,
    pub series: u32,
    pub value: f64,
    pub group_id: u64,
    pub config: u32,
    pub _pad: u32,
}

/// PM_MX_MANUAL, PM_MX_ROW_MAX, PM_MXB_*, PM_MXF_MAX
pub const MX_MANUAL: u32 = 0xFFFF_FFFF;
pub const MX_ROW_MAX: u32 = 1024;
pub const MXB_REPLACE: u32 = 0;
pub const MXB_MERGE: u32 = 1;
pub const MXB_DELETE: u32 = 2;
pub const MXF_MAX: u32 = 1;

/// pm_ro_report / pm_ro_summary / pm_ro_task_row / pm_ro_group_row / pm_ro_worker_row (include/pm_engine.h): the rollout ledger's
/// batch and its reads
#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct pm_ro_report {
    pub worker: u32,
    pub state: u32,
    pub uid: u64,
}

#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct pm_ro_summary {
    pub by_class: [u32; 6],
    pub by_state: [u32; 9],
    pub groups_with_task: u32,
    pub groups_converged: u32,
    pub distinct_uids: u32,
}

#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct pm_ro_task_row {
    pub uid: u64,
    pub task: u32,
    pub groups: u32,
    pub groups_converged: u32,
    pub assigned: u32,
    pub converged: u32,
    pub reporters: [u32; 8],
    pub _pad: u32,
}

#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct pm_ro_group_row {
    pub group_id: u64,
    pub slot: u32,
    pub config: u32,
    pub task: u32,
    pub size: u32,
    pub same: [u32; 8],
    pub other: u32,
    pub silent: u32,
}

#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct pm_ro_worker_row {
    pub worker: u32,
    pub group_slot: u32,
    pub uid: u64,
    pub cls: u8,
    pub state: u8,
    pub _pad: u16,
    pub _pad2: u32,
}

/// pm_dir_query / pm_dir_row (include/pm_engine.h): the node directory's query and its joined row
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct pm_dir_query {
    pub status_mask: u32,
    pub membership: u32,
    pub order: u32,
    pub offset: u32,
    pub limit: u32,
}

#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct pm_dir_row {
    pub worker: u32,
    pub status: u8,
    pub cls: u8,
    pub state: u8,
    pub _pad: u8,
    pub counter: u32,
    pub group_slot: u32,
    pub group_id: u64,
    pub group_size: u32,
    pub config: u32,
    pub task: u32,
    pub _pad2: u32,
    pub uid: u64,
}

/// PM_DIR_* (membership, order), PM_DC_* (the listing's four classes)
pub const DIR_ANY: u32 = 0;
pub const DIR_GROUPED: u32 = 1;
pub const DIR_UNGROUPED: u32 = 2;
pub const DIR_BY_ROW: u32 = 0;
pub const DIR_BY_ADDRESS: u32 = 1;
pub const DC_HEALTHY: u32 = 0;
pub const DC_DISCOVERED: u32 = 1;
pub const DC_OTHER: u32 = 2;
pub const DC_DEAD: u32 = 3;
pub const DC_N: u32 = 4;

/// pm_gdir_query / pm_gdir_totals / pm_gdir_row (include/pm_engine.h): the group directory's query, counters and joined row
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct pm_gdir_query {
    pub config_mask: u64,
    pub holds: u32,
    pub size_min: u32,
    pub size_max: u32,
    pub health_mask: u32,
    pub rollout_mask: u32,
    pub order: u32,
    pub offset: u32,
    pub limit: u32,
}

#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct pm_gdir_totals {
    pub total: u32,
    pub members_total: u32,
    pub by_health: [u32; 3],
    pub by_rollout: [u32; 3],
    pub n_cfgs: u32,
}

#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct pm_gdir_row {
    pub group_id: u64,
    pub slot: u32,
    pub config: u32,
    pub size: u32,
    pub task: u32,
    pub member_begin: u32,
    pub health: u8,
    pub rollout: u8,
    pub _pad: u16,
    pub by_status: [u32; 8],
    pub converged: u32,
    pub behind: u32,
    pub other: u32,
    pub silent: u32,
}

/// PM_GDIR_* (holds, order), PM_GH_* (health classes), PM_GR_* (rollout classes)
pub const GDIR_ANY: u32 = 0;
pub const GDIR_WITH_TASK: u32 = 1;
pub const GDIR_WITHOUT_TASK: u32 = 2;
pub const GDIR_BY_SLOT: u32 = 0;
pub const GDIR_BY_ID_TEXT: u32 = 1;
pub const GDIR_BY_SIZE_DESC: u32 = 2;
pub const GH_LOST: u32 = 0;
pub const GH_DEGRADED: u32 = 1;
pub const GH_SOUND: u32 = 2;
pub const GH_N: u32 = 3;
pub const GH_NONE: u32 = 255;
pub const GR_NO_TASK: u32 = 0;
pub const GR_CONVERGED: u32 = 1;
pub const GR_ROLLING: u32 = 2;
pub const GR_N: u32 = 3;
pub const GR_NONE: u32 = 255;

/// pm_tdir_query / pm_tdir_totals / pm_tdir_row (include/pm_engine.h): the task directory's query, counters and joined row
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct pm_tdir_query {
    pub config_mask: u64,
    pub serve_mask: u32,
    pub rollout_mask: u32,
    pub workers_min: u32,
    pub workers_max: u32,
    pub order: u32,
    pub offset: u32,
    pub limit: u32,
    pub _pad: u32,
}

#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct pm_tdir_totals {
    pub tasks: u32,
    pub total: u32,
    pub by_serve: [u32; 3],
    pub by_rollout: [u32; 3],
    pub unrestricted: u32,
    pub workers_running: u32,
    pub reporters: u32,
    pub orphan_uids: u32,
    pub orphan_reporters: u32,
    pub n_cfgs: u32,
}

#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct pm_tdir_row {
    pub uid: u64,
    pub created_at: i64,
    pub topo_mask: u64,
    pub task: u32,
    pub groups_allowed: u32,
    pub groups_running: u32,
    pub workers_running: u32,
    pub groups_converged: u32,
    pub converged: u32,
    pub reporters: [u32; 8],
    pub serve: u8,
    pub rollout: u8,
    pub _pad: u16,
    pub _pad2: u32,
}

/// PM_TDIR_* (order), PM_TKS_* (serving classes), PM_TKR_* (rollout classes)
pub const TDIR_BY_LIST: u32 = 0;
pub const TDIR_BY_OLDEST: u32 = 1;
pub const TDIR_BY_WORKERS_DESC: u32 = 2;
pub const TDIR_BY_REPORTERS_DESC: u32 = 3;
pub const TKS_RUNNING: u32 = 0;
pub const TKS_WAITING: u32 = 1;
pub const TKS_STARVED: u32 = 2;
pub const TKS_N: u32 = 3;
pub const TKR_UNHELD: u32 = 0;
pub const TKR_CONVERGED: u32 = 1;
pub const TKR_ROLLING: u32 = 2;
pub const TKR_N: u32 = 3;
pub const TKR_NONE: u32 = 255;

/// PM_TS_* (TaskState, shared/src/models/task.rs:12-22, in its order), PM_TS_NONE, PM_RO_*
pub const TS_PENDING: u32 = 0;
pub const TS_PULLING: u32 = 1;
pub const TS_RUNNING: u32 = 2;
pub const TS_COMPLETED: u32 = 3;
pub const TS_FAILED: u32 = 4;
pub const TS_PAUSED: u32 = 5;
pub const TS_RESTARTING: u32 = 6;
pub const TS_UNKNOWN: u32 = 7;
pub const TS_N: usize = 8;
pub const TS_NONE: u32 = 255;
pub const RO_IDLE: u32 = 0;
pub const RO_STRAY: u32 = 1;
pub const RO_SILENT: u32 = 2;
pub const RO_OTHER: u32 = 3;
pub const RO_BEHIND: u32 = 4;
pub const RO_CONVERGED: u32 = 5;
pub const RO_N: u32 = 6;

/// PM_NS_* (NodeStatus, models/node.rs:75-85, in its order), PM_LIVE_TTL_MS, PM_LIVE_GIVE_UP
pub const NS_DISCOVERED: u8 = 0;
pub const NS_WAITING: u8 = 1;
pub const NS_HEALTHY: u8 = 2;
pub const NS_UNHEALTHY: u8 = 3;
pub const NS_DEAD: u8 = 4;
pub const NS_EJECTED: u8 = 5;
pub const NS_BANNED: u8 = 6;
pub const NS_LOWBALANCE: u8 = 7;
pub const NS_N: u8 = 8;
pub const LIVE_TTL_MS: u32 = 90000;
pub const LIVE_GIVE_UP: u32 = 360;

/// pm_disc_row (include/pm_engine.h): one row of the de-duplicated discovery list
#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct pm_disc_row {
    pub row: u32,
    pub endpoint: u32,
    pub endpoint_after: u32,
    pub flags: u32,
    pub last_change_ms: u64,
    pub last_updated_ms: u64,
}

/// pm_disc_result (include/pm_engine.h): what pm_discovery_sync made of a row
#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct pm_disc_result {
    pub healthy_same_endpoint: u32,
    pub old_status: u8,
    pub final_status: u8,
    pub n_updates: u8,
    pub ops: u8,
    pub upd_old: [u8; 3],
    pub upd_new: [u8; 3],
    pub _pad: u16,
}

/// PM_DISC_NEW, PM_EP_NONE, PM_DISC_GRACE_MS, PM_DF_*, PM_DO_*
pub const DISC_NEW: u32 = 0xFFFF_FFFF;
pub const EP_NONE: u32 = 0xFFFF_FFFF;
pub const DISC_GRACE_MS: u32 = 300000;
pub const DF_VALIDATED: u32 = 1;
pub const DF_WHITELISTED: u32 = 2;
pub const DF_ACTIVE: u32 = 4;
pub const DF_LOCATION_NEW: u32 = 8;
pub const DF_SPECS_DIFFER: u32 = 16;
pub const DF_BALANCE_ZERO: u32 = 32;
pub const DO_ADMIT: u32 = 1;
pub const DO_SKIP: u32 = 2;
pub const DO_IP_REWRITE: u32 = 4;
pub const DO_LOCATION: u32 = 8;
pub const DO_SPECS_REWRITE: u32 = 16;
pub const DO_STAMP_NOW: u32 = 32;

/// what sync_single_node_with_discovery reads of a DiscoveryNode (GpuMatchPlugin::sync_discovery)
#[derive(Clone, Debug, Default)]
pub struct DiscoverySighting {
    pub address: Address,
    pub ip_address: String,
    pub port: u16,
    pub is_validated: bool,
    pub is_provider_whitelisted: bool,
    pub is_active: bool,
    pub location_new: bool,        // the store's location is None and discovery's is Some (monitor.rs:345)
    pub specs_differ: bool,        // existing_node.compute_specs != discovery_node.compute_specs (:367)
    pub balance_zero: bool,        // latest_balance == Some(0) (:385-386)
    pub last_updated_ms: u64,      // discovery.last_updated, 0 = None
}

#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum DiscoveryKind { Admitted, Skipped, Synced }

/// one per sighting, in order
#[derive(Clone, Debug)]
pub struct DiscoveryOutcome {
    pub kind: DiscoveryKind,
    pub address: String,
    pub healthy_same_endpoint: u32,
    pub old_status: NodeStatus,                     // (Synced)
    pub final_status: NodeStatus,
    pub updates: Vec<(NodeStatus, NodeStatus)>,     // (old, new) as the handlers saw them
    pub ip_rewritten: bool,
    pub location_new: bool,
    pub specs_rewritten: bool,
    pub stamped_now: bool,
}

fn node_status_code(s: &NodeStatus) -> u8 {
    match s {
        NodeStatus::Discovered => NS_DISCOVERED,
        NodeStatus::WaitingForHeartbeat => NS_WAITING,
        NodeStatus::Healthy => NS_HEALTHY,
        NodeStatus::Unhealthy => NS_UNHEALTHY,
        NodeStatus::Dead => NS_DEAD,
        NodeStatus::Ejected => NS_EJECTED,
        NodeStatus::Banned => NS_BANNED,
        NodeStatus::LowBalance => NS_LOWBALANCE,
    }
}

fn node_status_of(code: u8) -> NodeStatus {
    match code {
        NS_DISCOVERED => NodeStatus::Discovered,
        NS_WAITING => NodeStatus::WaitingForHeartbeat,
        NS_HEALTHY => NodeStatus::Healthy,
        NS_UNHEALTHY => NodeStatus::Unhealthy,
        NS_DEAD => NodeStatus::Dead,
        NS_EJECTED => NodeStatus::Ejected,
        NS_BANNED => NodeStatus::Banned,
        _ => NodeStatus::LowBalance,          // (NS_LOWBALANCE: sweep_statuses has refused codes >= NS_N)
    }
}

/// pm_force_regroup's metrics (PM_REGROUP_*)
pub const REGROUP_ALL: u32 = 0;
pub const REGROUP_DIAMETER: u32 = 1;
pub const REGROUP_LONGEST_HOP: u32 = 2;

#[repr(C)]
pub struct pm_group_vars {
    pub group_index: u32,
    pub group_size: u32,
    pub next_p2p_address: *const c_char,
    pub group_id: *const c_char,
    pub total_upload_count: *const c_char,
}

/// One all-gather of the multi-GPU tick (device pointers; recv = [world][bytes_per_rank]).
#[repr(C)]
#[derive(Default)]
pub struct pm_dist_xfer {
    pub send_ptr: u64,
    pub recv_ptr: u64,
    pub bytes_per_rank: u64,
}

#[link(name = "pm_engine")]
extern "C" {
    fn pm_engine_config_default(cfg: *mut pm_engine_config);
    fn pm_engine_create(cfg: *const pm_engine_config, out: *mut *mut c_void) -> i32;
    fn pm_engine_destroy(e: *mut c_void);
    fn pm_last_error() -> *const c_char;
    fn pm_set_configs(e: *mut c_void, cfgs: *const pm_config_row, n: u32, alts: *const pm_gpu_alt_row, n_alts: u32) -> i32;
    fn pm_set_model_table(e: *mut c_void, bits: *const u32, n_rows: u32, n_classes: u32) -> i32;
    fn pm_set_enabled_mask(e: *mut c_void, enabled: u64) -> i32;
    fn pm_upload_workers(e: *mut c_void, w: *const pm_worker_soa, keep_groups: u32) -> i32;
    fn pm_append_workers(e: *mut c_void, rows: *const pm_worker_soa, first_index: *mut u32) -> i32;
    fn pm_update_workers(e: *mut c_void, idx: *const u32, rows: *const pm_worker_soa) -> i32;
    fn pm_set_addr_ranks(e: *mut c_void, ranks: *const u32, n: u32) -> i32;
    fn pm_upload_tasks(e: *mut c_void, t: *const pm_task_soa) -> i32;
    fn pm_tasks_insert_front(e: *mut c_void, rows: *const pm_task_soa) -> i32;
    fn pm_tasks_insert_front_ex(e: *mut c_void, rows: *const pm_task_soa, republish: u32) -> i32;
    fn pm_tasks_delete(e: *mut c_void, uids: *const u64, n: u32, n_deleted: *mut u32) -> i32;
    fn pm_on_worker_status(e: *mut c_void, worker: u32, flags_new: u32, dead: u32) -> i32;
    fn pm_on_worker_status_many(e: *mut c_void, workers: *const u32, flags_new: *const u32, dead: *const u32, n: u32) -> i32;
    fn pm_enable_group_events(e: *mut c_void, on: u32) -> i32;
    fn pm_drain_group_events(e: *mut c_void, events: *mut pm_group_event, cap_events: u32, members: *mut u32,
                             cap_members: u32, n_events: *mut u32, n_members: *mut u32) -> i32;
    fn pm_dissolve_group(e: *mut c_void, group_slot: u32) -> i32;
    fn pm_dissolve_group_by_id(e: *mut c_void, group_id: u64, dissolved: *mut u32) -> i32;
    fn pm_get_groups(e: *mut c_void, group_of_worker: *mut i32, groups: *mut pm_group, cap_groups: u32, n_groups: *mut u32,
                     members: *mut u32, cap_members: u32, n_members: *mut u32) -> i32;
    fn pm_get_group_by_id(e: *mut c_void, group_id: u64, out: *mut pm_group, members: *mut u32, cap_members: u32, slot: *mut u32) -> i32;
    fn pm_get_group_of_worker(e: *mut c_void, worker: u32, out: *mut pm_group, members: *mut u32, cap_members: u32, slot: *mut u32) -> i32;
    fn pm_host_config_order(cfgs: *const pm_config_row, n_cfgs: u32, enabled: u64, order_out: *mut u32, n_out: *mut u32) -> i32;
    fn pm_tick(e: *mut c_void, stats: *mut pm_stats) -> i32;
    fn pm_lookup_task_for_worker(e: *mut c_void, worker: u32, out: *mut pm_assignment) -> i32;
    fn pm_host_group_vars(input: *const c_char, v: *const pm_group_vars, out: *mut c_char, cap: usize, needed: *mut usize) -> i32;
    fn pm_host_volume_vars(input: *const c_char, group_id: *const c_char, out: *mut c_char, cap: usize, needed: *mut usize) -> i32;
    fn pm_host_build_model_table(req_models: *const *const c_char, n_rows: u32,
                                 spec_models: *const *const c_char, n_classes: u32, bits_out: *mut u32) -> i32;
    // multi-GPU (one process per GPU; the all-gathers are ncclAllGather on the stream handed to pm_set_stream)
    fn pm_set_stream(e: *mut c_void, hip_stream: *mut c_void) -> i32;
    fn pm_set_carve_workgroups(e: *mut c_void, n: u32) -> i32;
    // (several pools served by one orchestrator process: one match per engine in one call — not used by the one-pool plugin below)
    fn pm_tick_many(engines: *const *mut c_void, n: u32, stats: *mut pm_stats, flags: u32) -> i32;
    fn pm_dist_configure(e: *mut c_void, rank: u32, world: u32, shard_of_worker: *const u8) -> i32;
    fn pm_dist_tick_begin(e: *mut c_void) -> i32;
    fn pm_dist_carve_wait(e: *mut c_void) -> i32;
    fn pm_dist_match_begin(e: *mut c_void, x: *mut pm_dist_xfer) -> i32;
    fn pm_dist_tick_end(e: *mut c_void, stats: *mut pm_stats) -> i32;
    fn pm_match(e: *mut c_void, task_of_worker: *mut u32, applicable_count: *mut u32) -> i32;
    fn pm_adopt_groups(e: *mut c_void, groups: *const pm_group, n_groups: u32, members: *const u32, n_members: u32,
                       id_state: u64) -> i32;
    fn pm_group_id_state(e: *mut c_void, state: *mut u64) -> i32;
    fn pm_explain_workers(e: *mut c_void, workers: *const u32, n: u32, why: *mut u8, state: *mut u32) -> i32;
    fn pm_config_report(e: *mut c_void, out: *mut pm_config_report_row, cap: u32, n_cfgs: *mut u32) -> i32;
    fn pm_task_report(e: *mut c_void, groups_running: *mut u32, workers_running: *mut u32, groups_allowed: *mut u32) -> i32;
    fn pm_group_spread(e: *mut c_void, out: *mut pm_group_spread_row, cap: u32, n_groups: *mut u32) -> i32;
    fn pm_config_spread(e: *mut c_void, out: *mut pm_config_spread_row, cap: u32, n_cfgs: *mut u32) -> i32;
    fn pm_force_regroup(e: *mut c_void, config: u32, metric: u32, threshold_km: f64, dissolved_groups: *mut u32,
                        affected_workers: *mut u32) -> i32;
    fn pm_nearest_workers(e: *mut c_void, q: *const pm_near_query, n_q: u32, pool: u32, k: u32, rows: *mut pm_near_row,
                          workers: *mut u32, km: *mut f64) -> i32;
    fn pm_probe_configs(e: *mut c_void, probes: *const pm_config_row, n_probes: u32, alts: *const pm_gpu_alt_row, n_alts: u32,
                        model_bits: *const u32, n_model_rows: u32, n_classes: u32, rows: *mut pm_probe_row,
                        overlap: *mut u32, mask_out: *mut u64) -> i32;
    fn pm_config_overlap(e: *mut c_void, overlap: *mut u32, cap: u32, n_cfgs: *mut u32) -> i32;
    fn pm_enable_assignment_changes(e: *mut c_void, on: u32) -> i32;
    fn pm_drain_assignment_changes(e: *mut c_void, rows: *mut pm_change_row, cap: u32, n: *mut u32, flags: *mut u32) -> i32;
    fn pm_liveness_enable(e: *mut c_void, on: u32, missing_heartbeat_threshold: u32) -> i32;
    fn pm_liveness_set(e: *mut c_void, idx: *const u32, status: *const u8, counter: *const u32, n: u32) -> i32;
    fn pm_liveness_get(e: *mut c_void, idx: *const u32, n: u32, status: *mut u8, counter: *mut u32) -> i32;
    fn pm_liveness_sweep(e: *mut c_void, now_ms: u64, last_beat_ms: *const u64, in_pool_bits: *const u64, apply: u32,
                         n_transitions: *mut u32, census: *mut u32) -> i32;
    fn pm_liveness_transitions(e: *mut c_void, rows: *mut pm_live_row, cap: u32, n: *mut u32) -> i32;
    fn pm_discovery_sync(e: *mut c_void, now_ms: u64, row_endpoint: *const u32, n_endpoints: u32, max_healthy_same_endpoint: u32,
                         rows: *const pm_disc_row, n_rows: u32, apply: u32, out: *mut pm_disc_result,
                         n_updates_total: *mut u32) -> i32;
    fn pm_metrics_enable(e: *mut c_void, on: u32) -> i32;
    fn pm_metrics_ingest(e: *mut c_void, beats: *const pm_mx_beat, n_beats: u32, entries: *const pm_mx_entry, n_entries: u32,
                         n_series: u32) -> i32;
    fn pm_metrics_totals(e: *mut c_void, sum: *mut f64, count: *mut u32, cap: u32, n_series: *mut u32) -> i32;
    fn pm_metrics_rows(e: *mut c_void, rows: *const u32, n: u32, out: *mut pm_mx_row, cap: u32, n_out: *mut u32) -> i32;
    fn pm_rollout_enable(e: *mut c_void, on: u32) -> i32;
    fn pm_rollout_ingest(e: *mut c_void, reports: *const pm_ro_report, n: u32) -> i32;
    fn pm_rollout_get(e: *mut c_void, idx: *const u32, n: u32, uid: *mut u64, state: *mut u8) -> i32;
    fn pm_rollout_summary(e: *mut c_void, out: *mut pm_ro_summary) -> i32;
    fn pm_rollout_tasks(e: *mut c_void, rows: *mut pm_ro_task_row, cap: u32, n: *mut u32) -> i32;
    fn pm_rollout_groups(e: *mut c_void, rows: *mut pm_ro_group_row, cap: u32, n: *mut u32) -> i32;
    fn pm_rollout_workers(e: *mut c_void, class_mask: u32, rows: *mut pm_ro_worker_row, cap: u32, n: *mut u32) -> i32;
    fn pm_directory(e: *mut c_void, q: *const pm_dir_query, total: *mut u32, counts: *mut u32, rows: *mut pm_dir_row, cap: u32,
                    n_rows: *mut u32) -> i32;
    fn pm_group_directory(e: *mut c_void, q: *const pm_gdir_query, totals: *mut pm_gdir_totals, by_config: *mut u32, cap_cfgs: u32,
                          rows: *mut pm_gdir_row, cap_rows: u32, n_rows: *mut u32, members: *mut u32, cap_members: u32,
                          n_members: *mut u32) -> i32;
    fn pm_task_directory(e: *mut c_void, q: *const pm_tdir_query, totals: *mut pm_tdir_totals, by_config: *mut u32, cap_cfgs: u32,
                         rows: *mut pm_tdir_row, cap_rows: u32, n_rows: *mut u32) -> i32;
    fn pm_host_task_state(s: *const c_char) -> u32;
    // address book (include/pm_engine.h "address book")
    fn pm_addresses_enable(e: *mut c_void, on: u32) -> i32;
    fn pm_addresses_set(e: *mut c_void, first_row: u32, addr20: *const u8, n: u32) -> i32;
    fn pm_addresses_rank(e: *mut c_void, rank_out: *mut u32) -> i32;
    fn pm_addresses_text(e: *mut c_void, rows: *const u32, n: u32, out: *mut c_char) -> i32;
    fn pm_keccak256_many(e: *mut c_void, bytes: *const u8, offsets: *const u32, n: u32, out: *mut u8) -> i32;
    fn pm_invite_digests(e: *mut c_void, domain_id: u32, pool_id: u32, rows: *const u32, n: u32, nonce: *const u8,
                         expiration_s: *const u64, digest: *mut u8, signing_hash: *mut u8) -> i32;
    fn pm_host_keccak256(bytes: *const u8, len: usize, out32: *mut u8) -> i32;
    fn pm_host_eip55(addr20: *const u8, out43: *mut c_char) -> i32;
    // request gate (include/pm_engine.h "request gate")
    fn pm_ecrecover_many(e: *mut c_void, hash32: *const u8, sig65: *const u8, n: u32, addr20_out: *mut u8, pub64_out: *mut u8,
                         ok_out: *mut u8) -> i32;
    fn pm_verify_requests(e: *mut c_void, bytes: *const u8, offsets: *const u32, sig65: *const u8, claimed20: *const u8,
                          flags: *const u8, n: u32, out: *mut pm_rq_verdict, counts: *mut u32) -> i32;
    fn pm_host_ecrecover(hash32: *const u8, sig65: *const u8, addr20: *mut u8) -> i32;
    // request gate: admission (include/pm_engine.h "request gate: admission")
    fn pm_admission_enable(e: *mut c_void, on: u32) -> i32;
    fn pm_admit_requests(e: *mut c_void, now_ms: u64, bytes: *const u8, offsets: *const u32, sig65: *const u8, claimed20: *const u8,
                         flags: *const u8, timestamp_s: *const u64, nonce_bytes: *const u8, nonce_offsets: *const u32, n: u32,
                         out: *mut pm_rq_verdict, counts: *mut u32) -> i32;
    fn pm_liveness_sweep_beats(e: *mut c_void, now_ms: u64, last_beat_ms: *const u64, in_pool_bits: *const u64, apply: u32,
                               n_transitions: *mut u32, census: *mut u32) -> i32;
}

/// RCCL (librccl.so, rccl/rccl.h): the one collective the multi-GPU tick issues
#[link(name = "rccl")]
extern "C" {
    fn ncclAllGather(sendbuff: *const c_void, recvbuff: *mut c_void, sendcount: usize, datatype: i32,
                     comm: *mut c_void, stream: *mut c_void) -> i32;
    fn ncclGetErrorString(result: i32) -> *const c_char;
}
const NCCL_UINT8: i32 = 1;      // ncclUint8 (rccl.h: ncclInt8 = 0, ncclUint8 = 1)

/// The collective of the multi-GPU tick (include/pm_engine.h "multi-GPU"): one process per GPU, every rank holds
/// the whole swarm and runs the whole carve (replicated), the pair sweep + claim run for the OWNED workers, and the
/// published rows are all-gathered ONCE per tick.  The plugin is handed the communicator; it owns none.
pub trait AllGather: Send + Sync {
    fn rank(&self) -> u32;
    fn world(&self) -> u32;
    /// the hipStream_t the engine's kernels and the collective share (ordered without a host wait); null = the engine's own
    fn stream(&self) -> *mut c_void;
    /// device pointers; recv = [world][bytes_per_rank], send = this rank's slot of it: enqueue on stream()
    fn all_gather(&self, send: *const c_void, recv: *mut c_void, bytes_per_rank: usize) -> Result<()>;
}

/// ncclAllGather over xGMI on a communicator and a stream the host owns (`ncclComm_t`, `hipStream_t`: created by
/// `main()` with ncclCommInitRank after the launcher's rendezvous — protocol_amd/plugin/rccl_all_gather.cpp shows one
/// through an id file).  The tick's one collective moves world x cap x 32 bytes (8 ranks x 100k workers: 3.2 MB landed
/// per GPU): latency-bound, a single call on the compute stream.
pub struct RcclAllGather { pub comm: *mut c_void, pub stream: *mut c_void, pub rank: u32, pub world: u32 }
unsafe impl Send for RcclAllGather {}
unsafe impl Sync for RcclAllGather {}
impl AllGather for RcclAllGather {
    fn rank(&self) -> u32 { self.rank }
    fn world(&self) -> u32 { self.world }
    fn stream(&self) -> *mut c_void { self.stream }
    fn all_gather(&self, send: *const c_void, recv: *mut c_void, bytes_per_rank: usize) -> Result<()> {
        // (send is this rank's slot of recv: RCCL's in-place form, no staging copy)
        let rc = unsafe { ncclAllGather(send, recv, bytes_per_rank, NCCL_UINT8, self.comm, self.stream) };
        if rc == 0 { return Ok(()); }
        Err(anyhow!("ncclAllGather: {}", unsafe { CStr::from_ptr(ncclGetErrorString(rc)) }.to_string_lossy()))
    }
}

/// owner rank of a node: splitmix64 finaliser of the low 8 bytes of the address, mod world
pub fn shard_of(a: &Address, world: u32) -> u32 {
    let mut low = [0u8; 8];
    low.copy_from_slice(&a.as_slice()[12..20]);
    let mut z = u64::from_be_bytes(low).wrapping_add(0x9E37_79B9_7F4A_7C15);
    z = (z ^ (z >> 30)).wrapping_mul(0xBF58_476D_1CE4_E5B9);
    z = (z ^ (z >> 27)).wrapping_mul(0x94D0_49BB_1331_11EB);
    z ^= z >> 31;
    if world == 0 { 0 } else { (z % world as u64) as u32 }
}

/// what pm_dist_configure was last told (tick_dist's; the management loop's thread only)
struct DistState { world: u32, rows: usize, stream: *mut c_void }

// worker flag bits (include/pm_engine.h)
const W_HAS_SPECS: u32 = 1 << 0; const W_HAS_GPU: u32 = 1 << 1; const W_GPU_COUNT: u32 = 1 << 2;
const W_GPU_MEM: u32 = 1 << 3; const W_GPU_MODEL: u32 = 1 << 4; const W_HAS_CPU: u32 = 1 << 5;
const W_CPU_CORES: u32 = 1 << 6; const W_RAM: u32 = 1 << 7; const W_STORAGE: u32 = 1 << 8;
const W_HEALTHY: u32 = 1 << 9; const W_HAS_P2P: u32 = 1 << 10; const W_HAS_LOC: u32 = 1 << 11;
// requirement flag bits
const R_HAS_REQ: u32 = 1 << 0; const R_CPU: u32 = 1 << 1; const R_CPU_CORES: u32 = 1 << 2;
const R_RAM: u32 = 1 << 3; const R_STORAGE: u32 = 1 << 4;
const G_COUNT: u32 = 1 << 0; const G_MODEL: u32 = 1 << 1; const G_MEM: u32 = 1 << 2; const G_MEM_MIN: u32 = 1 << 3;
const G_MEM_MAX: u32 = 1 << 4; const G_TOT_MIN: u32 = 1 << 5; const G_TOT_MAX: u32 = 1 << 6;

fn check(rc: i32) -> Result<()> {
    if rc == 0 { return Ok(()); }
    let msg = unsafe { CStr::from_ptr(pm_last_error()) }.to_string_lossy().into_owned();
    Err(anyhow!("pm_engine error {rc}: {msg}"))
}

/// One worker row as the engine sees it; `PartialEq` is what decides whether a known node is rewritten.
#[derive(Clone, PartialEq, Default)]
struct Row {
    flags: u32, gpu_count: u32, gpu_mem: u32, gpu_class: u32, cpu_cores: u32, ram: u32, storage: u32,
    lat: f64, lon: f64,
}

/// Columns of a batch of rows, kept alive for the duration of one FFI call.
#[derive(Default)]
struct RowColumns {
    flags: Vec<u32>, gpu_count: Vec<u32>, gpu_mem: Vec<u32>, gpu_class: Vec<u32>, cpu_cores: Vec<u32>,
    ram: Vec<u32>, storage: Vec<u32>, addr_rank: Vec<u32>, lat: Vec<f64>, lon: Vec<f64>,
}
impl RowColumns {
    fn push(&mut self, r: &Row, rank: u32) {
        self.flags.push(r.flags); self.gpu_count.push(r.gpu_count); self.gpu_mem.push(r.gpu_mem);
        self.gpu_class.push(r.gpu_class); self.cpu_cores.push(r.cpu_cores); self.ram.push(r.ram);
        self.storage.push(r.storage); self.addr_rank.push(rank); self.lat.push(r.lat); self.lon.push(r.lon);
    }
    fn soa(&self) -> pm_worker_soa {
        pm_worker_soa { n: self.flags.len() as u32, flags: self.flags.as_ptr(), gpu_count: self.gpu_count.as_ptr(),
            gpu_mem_mb: self.gpu_mem.as_ptr(), gpu_model_class: self.gpu_class.as_ptr(),
            cpu_cores: self.cpu_cores.as_ptr(), ram_mb: self.ram.as_ptr(), storage_gb: self.storage.as_ptr(),
            price: std::ptr::null(), addr_rank: self.addr_rank.as_ptr(), lat: self.lat.as_ptr(), lon: self.lon.as_ptr() }
    }
}

/// The plugin's mirror of the engine's worker table (rows never move, never disappear).
#[derive(Default)]
struct NodeTable {
    index: HashMap<Address, u32>,
    addresses: Vec<Address>,
    address_strings: Vec<String>,   // address.to_string(): GROUP_INDEX is the rank of this string (mod.rs:424-434)
    p2p_ids: Vec<String>,           // node.p2p_id.unwrap_or_default() (scheduler_impl.rs:118-128)
    rows: Vec<Row>,
    present: Vec<bool>,             // still in the node store
    by_address: Vec<u32>,           // rows in address-string order (kept sorted: a new node is one binary search)
    spec_models: Vec<String>,       // interned gpu.model strings; the index is gpu_model_class
    spec_model_index: HashMap<String, u32>,
    /// address book (enable_address_book): the rows' 20 bytes, bytes -> row, how many rows render the device's text, and the
    /// ranks pm_addresses_rank gave last (a rewritten row is sent with the rank it has).  by_address is not kept then.
    book_on: bool,
    admission_on: bool,
    book_bytes: Vec<u8>,
    book_by_bytes: HashMap<[u8; 20], u32>,
    book_texts: usize,
    book_ranks: Vec<u32>,
    /// an engine call of sync_nodes failed half-way: the row map above is ahead of the engine's worker table (tombstones
    /// recorded here and never sent, rows appended here the engine does not have) — the next interval re-sends every row
    engine_rows_stale: bool,
    /// liveness: the last beat per row in ms, 0 = never — stored under the READ lock (beat), grown and read whole under the
    /// write lock (sync_nodes, sweep_statuses)
    beats: Vec<AtomicU64>,
    /// enable_liveness was called: handle_status_change also writes the engine's ledger
    liveness_on: bool,
    /// discovery sync: the endpoint column by row (ip empty = unknown: EP_NONE), the interning map "ip:port" -> id, the
    /// endpoints of addresses without a row yet; last_status_change per row in ms, 0 = None.  Both grow lazily to the rows.
    ep_ip: Vec<String>,
    ep_port: Vec<u16>,
    ep_id: Vec<u32>,
    ep_intern: HashMap<String, u32>,
    ep_pending: HashMap<Address, (String, u16)>,
    stamps: Vec<u64>,
}

/// the metrics writes queued since the last flush, and the interner: field "{task_id or "manual"}:{label without ':'}" -> series
#[derive(Default)]
struct MetricsQueue {
    beats: Vec<pm_mx_beat>,
    entries: Vec<pm_mx_entry>,
    series: HashMap<String, u32>,
    keys: Vec<(String, String)>,   // series -> (task id or "manual", cleaned label)
}

/// the task reports queued since the last flush, and the text of every reported id (pruned to what the last task report listed)
#[derive(Default)]
struct RolloutQueue {
    reports: Vec<pm_ro_report>,
    texts: HashMap<u64, String>,
}

/// one set_nodes_per_task call of the sync service (metrics/sync_service.rs:258-266)
#[derive(Default, Debug, Clone, PartialEq)]
pub struct NodesPerTask {
    pub task_id: String,
    pub task_name: String,   // "unknown" where the task list has no such id
    pub count: u32,
}

#[derive(Default, Debug, Clone)]
pub struct TaskRollout {
    pub task_id: String,
    pub task_name: String,
    pub row: pm_ro_task_row,
}

#[derive(Default, Debug, Clone)]
pub struct GroupRollout {
    pub group_id: String,
    pub configuration_name: String,
    pub task_id: String,
    pub row: pm_ro_group_row,
}

#[derive(Default, Debug, Clone)]
pub struct NodeRollout {
    pub address: String,
    pub cls: u32,
    pub state: u32,
    pub task_id: Option<String>,   // the reported id's text (hex where the plugin has none), None: no report
}

/// the "group" object GET /nodes attaches to a node (api/routes/nodes.rs:83-88)
#[derive(Debug, Clone)]
pub struct ListedGroup {
    pub id: String,
    pub size: u32,
    pub created_at: chrono::DateTime<chrono::Utc>,
    pub topology_config: String,   // the configuration's NAME
}

#[derive(Debug, Clone)]
pub struct ListedNode {
    pub address: String,
    pub status: NodeStatus,
    pub unhealthy_counter: u32,
    pub task_state: u32,           // the reported state (TS_*), TS_NONE: no report or rollout off
    pub group: Option<ListedGroup>,
}

/// the filter of list_groups (gpu_match_groupdir.cpp's GroupFilter): `GroupFilter::default()` lists every group
#[derive(Debug, Clone, Copy)]
pub struct GroupFilter {
    pub config_mask: u64,          // bit c: the configuration of constructor index c
    pub holds: u32,
    pub size_min: u32,
    pub size_max: u32,
    pub health_mask: u32,
    pub rollout_mask: u32,
}

impl Default for GroupFilter {
    fn default() -> Self {
        GroupFilter { config_mask: u64::MAX, holds: GDIR_ANY, size_min: 0, size_max: u32::MAX, health_mask: (1 << GH_N) - 1,
                      rollout_mask: (1 << GR_N) - 1 }
    }
}

/// a group of the group directory: the NodeGroup the route renders, its classes, its claimed task, its counters
#[derive(Debug, Clone)]
pub struct ListedNodeGroup {
    pub group: NodeGroup,
    pub health: u32,               // GH_*, GH_NONE: liveness is off
    pub rollout: u32,              // GR_*, GR_NONE: rollout is off
    pub task_id: Option<String>,   // the claimed task
    pub row: pm_gdir_row,
}

/// one window of the group directory (gpu_match_groupdir.cpp's GroupListing)
#[derive(Default, Debug, Clone)]
pub struct GroupListing {
    pub total: u32,                // the whole filtered list's length, not the window's
    pub totals: pm_gdir_totals,
    pub groups: Vec<ListedNodeGroup>,
}

/// the filter of list_tasks (gpu_match_taskdir.cpp's TaskFilter): `TaskFilter::default()` lists every task
#[derive(Debug, Clone, Copy)]
pub struct TaskFilter {
    pub config_mask: u64,          // u64::MAX: no filter; else bit c: tasks that allow the configuration of constructor index c
    pub serve_mask: u32,
    pub rollout_mask: u32,
    pub workers_min: u32,
    pub workers_max: u32,
}

impl Default for TaskFilter {
    fn default() -> Self {
        TaskFilter { config_mask: u64::MAX, serve_mask: (1 << TKS_N) - 1, rollout_mask: (1 << TKR_N) - 1, workers_min: 0,
                     workers_max: u32::MAX }
    }
}

/// a task of the task directory: the plugin's id and name, its classes, its assigned and reported columns
#[derive(Debug, Clone)]
pub struct ListedTask {
    pub id: String,
    pub name: String,
    pub serve: u32,                // TKS_*
    pub rollout: u32,              // TKR_*, TKR_NONE: rollout is off
    pub row: pm_tdir_row,
}

/// one window of the task directory (gpu_match_taskdir.cpp's TaskListing)
#[derive(Default, Debug, Clone)]
pub struct TaskListing {
    pub total: u32,                // the whole filtered list's length, not the window's
    pub totals: pm_tdir_totals,
    pub tasks: Vec<ListedTask>,
}

#[derive(Default, Debug, Clone)]
pub struct TaskCounts {
    pub totals: pm_tdir_totals,
    pub by_config: std::collections::BTreeMap<String, u32>,   // configuration name -> tasks that allow it, present ones only
}

/// what sync_orchestrator_statistics sets (metrics/sync_service.rs:209-286); the gauges themselves stay the host's
#[derive(Default, Debug, Clone)]
pub struct OrchestratorStatistics {
    pub nodes_by_status: std::collections::BTreeMap<String, u32>,   // lowercase status name -> nodes, present ones only
    pub tasks_count: u32,
    pub nodes_per_task: Vec<NodesPerTask>,                          // the tasks with reporters
    pub groups_count: std::collections::BTreeMap<String, u32>,      // configuration name -> groups, present ones only
}

/// one window of the store's ordered listing (gpu_match_directory.cpp's NodeListing)
#[derive(Default, Debug, Clone)]
pub struct NodeListing {
    pub total: u32,                                  // the whole filtered list's length, not the window's
    pub counts: std::collections::BTreeMap<String, u32>,   // per status name as `{:?}` prints it; present ones only
    pub nodes: Vec<ListedNode>,
}

/// one record_compute_task_gauge call of sync_metrics_from_redis (gpu_match_metrics.cpp's SyncedMetric)
#[derive(Default, Debug, Clone)]
pub struct SyncedMetric {
    pub address: String,
    pub task_id: String,
    pub task_name: String,
    pub label: String,
    pub value: f64,
    pub group_id: Option<String>,
    pub group_config_name: Option<String>,
}

pub struct GpuMatchPlugin {
    engine: *mut c_void,
    templates: Vec<NodeGroupConfiguration>,     // caller order: the engine's configuration index
    config_rows: Vec<pm_config_row>,            // what pm_set_configs was given (pm_host_config_order reads sizes + R_HAS_REQ)
    enabled_mask: AtomicU64,                    // "available_node_group_configs" as last pushed (push_enabled)
    /// NodeGroup.created_at (mod.rs:575: Utc::now() when the group forms): stamped when the creation is reported by the
    /// life-cycle feed, dropped with the group.  A LEAF lock: never held across an engine call or another lock.
    group_created_at: parking_lot::Mutex<HashMap<u64, chrono::DateTime<chrono::Utc>>>,
    dist: parking_lot::Mutex<DistState>,
    dist_rank: AtomicU32,                       // (read by emit_group_webhooks on any thread: rank 0 reports)
    config_names: Vec<String>,
    req_models: Vec<CString>,       // requirement model strings, one per pm_gpu_alt_row.model_row
    nodes: parking_lot::RwLock<NodeTable>,
    tasks: parking_lot::RwLock<Vec<Task>>,   // get_all_tasks order: the engine reports positions in this Vec
    /// the metrics ledger's queue and interner (LOCK ORDER: nodes, metrics, the engine)
    metrics: parking_lot::Mutex<MetricsQueue>,
    /// the rollout ledger's queue and texts (LOCK ORDER: nodes, tasks, rollout, the engine)
    rollout: parking_lot::Mutex<RolloutQueue>,
    /// `upload:<node>:<group>:*` key count (scheduler_impl.rs:130-153): stays with the Redis store
    upload_counter: Box<dyn Fn(&Address, &str) -> usize + Send + Sync>,
    /// as in NodeGroupsPlugin (mod.rs:107, 124): the plugins told about every group created / destroyed
    webhook_plugins: Option<Vec<WebhookPlugin>>,
    /// on_task_created also re-matches the standing groups (pm_tasks_insert_front_ex, republish = 1): a group that
    /// holds no task is served the new one at its next heartbeat, as in the reference (scheduler_impl.rs:33-74),
    /// instead of after the next tick.  Costs one pair sweep + publish (~0.2 ms at 100k x 10k) per created task.
    pub republish_on_insert: bool,
    /// restore_groups' window: after a node and a task snapshot, before the first tick
    nodes_synced: AtomicBool,
    tasks_synced: AtomicBool,
    ticked: AtomicBool,
    /// this plugin is one rank of a pool that runs tick_dist: restore_groups needs an id_state (set before calling it)
    pub multi_gpu: bool,
}

/// what restore_groups left out (gpu_match_restore.cpp's RestoreReport)
#[derive(Default, Debug)]
pub struct RestoreReport {
    pub dropped: Vec<(String, String)>,   // (group id text, reason)
    pub task_cleared: Vec<String>,        // group_task:<id> naming no known task
}

/// explain_node's answer (gpu_match_report.cpp's NodeExplanation)
#[derive(Default, Debug)]
pub struct NodeExplanation {
    pub state: String,                        // "in_group", "unhealthy", "no_p2p", "idle"
    pub configs: Vec<(String, String)>,       // (configuration name, reason name), constructor order
}

/// one row of configuration_report (gpu_match_report.cpp's ConfigurationReport)
#[derive(Default, Debug)]
pub struct ConfigurationReport {
    pub name: String,
    pub enabled: bool,
    pub eligible_meets: u32,
    pub idle_meets: u32,
    pub why: [u32; 10],                       // Healthy nodes with a p2p id by reason code (why[0] == eligible_meets)
    pub groups: u32,
    pub members: u32,
    pub groups_without_task: u32,
    pub tasks_allowing: u32,
}

/// one task of task_report (gpu_match_report.cpp's TaskReport)
#[derive(Default, Debug, Clone, Copy)]
pub struct TaskReport {
    pub groups_running: u32,                  // get_groups_for_task (mod.rs:1350-1386)
    pub workers_running: u32,                 // nodes_per_task (metrics/sync_service.rs:243-267)
    pub groups_allowed: u32,                  // live groups whose configuration the task's topologies allow
}

/// one group of group_spread (gpu_match_spread.cpp's GroupSpread)
#[derive(Default, Debug, Clone)]
pub struct GroupSpread {
    pub located: u32,
    pub ring_hops: u32,
    pub far_a: String,                        // node addresses; empty = none
    pub far_b: String,
    pub hop_from: String,
    pub diameter_km: f64,
    pub ring_km: f64,
    pub longest_hop_km: f64,
}

/// one row of configuration_spread (gpu_match_spread.cpp's ConfigurationSpread)
#[derive(Default, Debug)]
pub struct ConfigurationSpread {
    pub name: String,
    pub groups: u32,
    pub measured: u32,
    pub hist: [u32; 5],                       // measured groups by diameter: < 10, < 100, < 1000, < 5000, >= 5000 km
    pub max_diameter_km: f64,
    pub max_hop_km: f64,
    pub sum_diameter_m: u64,
    pub sum_ring_m: u64,
}

/// force_regroup's answer: the route's dissolved_groups / affected_nodes (api/routes/groups.rs:319-380)
#[derive(Default, Debug, Clone, Copy, PartialEq, Eq)]
pub struct ForceRegroupResult {
    pub dissolved_groups: u32,
    pub affected_nodes: u32,
}

/// changed_nodes' answer (gpu_match_changes.cpp's ChangedNodes)
#[derive(Default, Debug, Clone)]
pub struct ChangedNodes {
    pub nodes: Vec<(String, u32)>,            // (address, OR of CHG_*), in row order
    pub resync: bool,                         // the engine lost track: every node is listed, render them all
}

/// nearest_nodes' answer (gpu_match_near.cpp's NearestNodes)
#[derive(Default, Debug, Clone)]
pub struct NearestNodes {
    pub origin: String,                       // the node the list is measured from; empty: the seed rule found no candidate
    pub candidates: u32,                      // nodes of the pool that meet the configuration, the origin excluded
    pub located: u32,                         // of them with a location
    pub nodes: Vec<(String, f64)>,            // (address, km), nearest first; km = f64::MAX: not measured
}

/// probe_configurations' answer per probe (gpu_match_probe.cpp's ProbeResult)
#[derive(Default, Debug, Clone)]
pub struct ProbeResult {
    pub name: String,
    pub why: [u32; 10],                       // Healthy nodes with a p2p id by reason code (why[0] == eligible_meets)
    pub eligible_meets: u32,
    pub idle_meets: u32,
    pub idle_located: u32,
    pub idle_exclusive: u32,
    pub groups_max: u32,                      // bounds from counts (/ min_group_size), not what a carve would form
    pub groups_exclusive: u32,
    pub overlap: Vec<(String, u32)>,          // (installed configuration name, idle nodes that meet the probe AND it)
}

/// configuration_overlap's answer (gpu_match_probe.cpp's ConfigurationOverlap)
#[derive(Default, Debug, Clone)]
pub struct ConfigurationOverlap {
    pub names: Vec<String>,                   // constructor order
    pub idle: Vec<u32>,                       // [a * names.len() + b]: idle nodes that meet both a and b (symmetric)
}

/// reason names in PM_WHY_* order
const WHY_NAMES: [&str; 10] = ["ok", "no_specs", "cpu", "ram", "storage", "gpu_none", "gpu_count", "gpu_model", "gpu_mem", "gpu_total"];

fn state_name(state: u32) -> &'static str {
    match state { 1 => "in_group", 2 => "unhealthy", 3 => "no_p2p", 0 => "idle", _ => "unknown" }
}

unsafe impl Send for DistState {}
unsafe impl Send for GpuMatchPlugin {}
unsafe impl Sync for GpuMatchPlugin {}

fn task_uid(t: &Task) -> u64 { t.id.as_u64_pair().1 }

impl GpuMatchPlugin {
    /// Same contract as NodeGroupsPlugin::new (node_groups/mod.rs:113-175): duplicate names or max < min panic,
    /// exactly like the reference constructor (the engine answers PM_EINVAL for the latter).
    pub fn new(templates: Vec<NodeGroupConfiguration>, device: i32,
               upload_counter: Box<dyn Fn(&Address, &str) -> usize + Send + Sync>,
               webhook_plugins: Option<Vec<WebhookPlugin>>) -> Self {
        // Hardware queues for the HIP runtime (GPU_MAX_HW_QUEUES, read once at the first HIP call of the process — the
        // pm_engine_create below; the orchestrator uses HIP for nothing else): the runtime maps a process's streams
        // onto 4 of them by default and runs two streams that share one in turn; an engine owns one stream, so a
        // process that serves several pools on one GPU needs >= 1 per pool (include/pm_engine.h,
        // pm_set_carve_workgroups).  `main()` sets it BEFORE the tokio runtime starts: writing the
        // environment from here would race with every getenv of a threaded process (and is `unsafe` in Rust 2024).
        // One pool is indifferent to the value; here it is only looked at.
        match std::env::var("GPU_MAX_HW_QUEUES").ok().and_then(|v| v.parse::<u32>().ok()) {
            Some(q) if q >= 8 => {}
            other => log::warn!("GPU_MAX_HW_QUEUES is {:?}: set it to 16 in main() before the runtime starts if this \
                                 process serves more than one pool on the GPU", other),
        }
        let mut cfg: pm_engine_config = unsafe { std::mem::zeroed() };
        unsafe { pm_engine_config_default(&mut cfg) };
        cfg.device = device;
        let mut engine = std::ptr::null_mut();
        check(unsafe { pm_engine_create(&cfg, &mut engine) }).expect("pm_engine_create");
        let mut seen = std::collections::HashSet::new();
        for t in &templates {
            if !seen.insert(t.name.clone()) { panic!("Configuration names must be unique"); }   // mod.rs:142-144
        }
        let mut this = Self { engine, templates: templates.clone(), config_rows: Vec::new(), enabled_mask: AtomicU64::new(0),
                              group_created_at: Default::default(),
                              dist: parking_lot::Mutex::new(DistState { world: 1, rows: usize::MAX, stream: std::ptr::null_mut() }),
                              dist_rank: AtomicU32::new(0),
                              config_names: templates.iter().map(|t| t.name.clone()).collect(),
                              req_models: Vec::new(), nodes: Default::default(), tasks: Default::default(),
                              metrics: Default::default(), rollout: Default::default(),
                              upload_counter, webhook_plugins, republish_on_insert: false,
                              nodes_synced: AtomicBool::new(false), tasks_synced: AtomicBool::new(false),
                              ticked: AtomicBool::new(false), multi_gpu: false };
        this.set_configs(&templates);
        // an empty worker / task table, so that the delta calls have something to extend
        let empty = RowColumns::default();
        check(unsafe { pm_upload_workers(this.engine, &empty.soa(), 0) }).expect("pm_upload_workers");
        check(unsafe { pm_enable_group_events(this.engine, 1) }).expect("pm_enable_group_events");   // webhook feed
        let t = pm_task_soa { n: 0, topo_mask: std::ptr::null(), created_at: std::ptr::null(), uid: [0u64; 0].as_ptr() };
        check(unsafe { pm_upload_tasks(this.engine, &t) }).expect("pm_upload_tasks");
        this
    }

    /// NodeGroupConfiguration (mod.rs:30-37) + ComputeRequirements / GpuRequirements (shared/models/node.rs:49-70)
    /// -> pm_config_row / pm_gpu_alt_row.  The requirement strings were already parsed by
    /// `ComputeRequirements::from_str` (serde), so this is a field-by-field projection.
    fn pack_templates(templates: &[NodeGroupConfiguration], alts: &mut Vec<pm_gpu_alt_row>,
                      req_models: &mut Vec<CString>) -> Vec<pm_config_row> {
        let mut rows = Vec::with_capacity(templates.len());
        let opt = |v: Option<u32>, bit: u32, flags: &mut u32| -> u32 { if v.is_some() { *flags |= bit; } v.unwrap_or(0) };
        for t in templates {
            let mut row = pm_config_row { min_group_size: t.min_group_size as u32, max_group_size: t.max_group_size as u32,
                                          ..Default::default() };
            if let Some(req) = &t.compute_requirements {
                row.flags |= R_HAS_REQ;
                if let Some(cpu) = &req.cpu {
                    row.flags |= R_CPU;
                    row.cpu_cores = opt(cpu.cores, R_CPU_CORES, &mut row.flags);
                }
                row.ram_mb = opt(req.ram_mb, R_RAM, &mut row.flags);
                row.storage_gb = opt(req.storage_gb, R_STORAGE, &mut row.flags);
                row.alt_begin = alts.len() as u32;
                row.alt_count = req.gpu.len() as u32;
                for g in &req.gpu {
                    let mut a = pm_gpu_alt_row::default();
                    a.count = opt(g.count, G_COUNT, &mut a.flags);
                    a.memory_mb = opt(g.memory_mb, G_MEM, &mut a.flags);
                    a.memory_mb_min = opt(g.memory_mb_min, G_MEM_MIN, &mut a.flags);
                    a.memory_mb_max = opt(g.memory_mb_max, G_MEM_MAX, &mut a.flags);
                    a.total_memory_min = opt(g.total_memory_min, G_TOT_MIN, &mut a.flags);
                    a.total_memory_max = opt(g.total_memory_max, G_TOT_MAX, &mut a.flags);
                    if let Some(m) = &g.model {
                        a.flags |= G_MODEL;
                        a.model_row = req_models.len() as u32;
                        req_models.push(CString::new(m.as_str()).expect("model string"));
                    }
                    alts.push(a);
                }
            }
            rows.push(row);
        }
        rows
    }

    fn set_configs(&mut self, templates: &[NodeGroupConfiguration]) {
        let mut alts: Vec<pm_gpu_alt_row> = Vec::new();
        let rows = Self::pack_templates(templates, &mut alts, &mut self.req_models);
        let rc = unsafe { pm_set_configs(self.engine, rows.as_ptr(), rows.len() as u32, alts.as_ptr(), alts.len() as u32) };
        if rc == PM_EINVAL { panic!("Plugin configuration is invalid"); }                                   // mod.rs:145-147
        check(rc).expect("pm_set_configs");
        self.config_rows = rows;
        self.push_model_table(&NodeTable::default());
    }

    /// The substring rule of GpuSpecs::meets (shared/models/node.rs:463-484), evaluated once per
    /// (requirement model, interned spec model) pair by the library; re-sent whenever a new spec model shows up.
    fn push_model_table(&self, nodes: &NodeTable) {
        let spec: Vec<CString> = nodes.spec_models.iter().map(|s| CString::new(s.as_str()).unwrap()).collect();
        let spec_p: Vec<*const c_char> = spec.iter().map(|s| s.as_ptr()).collect();
        let req_p: Vec<*const c_char> = self.req_models.iter().map(|s| s.as_ptr()).collect();
        let words = (spec.len() + 31) / 32;
        let mut bits = vec![0u32; (self.req_models.len() * words).max(1)];
        check(unsafe { pm_host_build_model_table(req_p.as_ptr(), req_p.len() as u32, spec_p.as_ptr(), spec_p.len() as u32,
                                                 bits.as_mut_ptr()) }).expect("pm_host_build_model_table");
        check(unsafe { pm_set_model_table(self.engine, bits.as_ptr(), req_p.len() as u32, spec_p.len() as u32) })
            .expect("pm_set_model_table");
    }

    /// Projection of one `OrchestratorNode` (orchestrator/src/models/node.rs:11-37) into the SoA row.
    fn project(node: &OrchestratorNode, table: &mut NodeTable, new_model: &mut bool) -> Row {
        let mut r = Row::default();
        if node.status == NodeStatus::Healthy { r.flags |= W_HEALTHY; }
        if node.p2p_id.is_some() { r.flags |= W_HAS_P2P; }
        if let Some(l) = &node.location { r.flags |= W_HAS_LOC; r.lat = l.latitude; r.lon = l.longitude; }
        if let Some(s) = &node.compute_specs {
            let s: &ComputeSpecs = s;
            r.flags |= W_HAS_SPECS;
            if let Some(g) = &s.gpu {
                r.flags |= W_HAS_GPU;
                if let Some(c) = g.count { r.flags |= W_GPU_COUNT; r.gpu_count = c; }
                if let Some(m) = g.memory_mb { r.flags |= W_GPU_MEM; r.gpu_mem = m; }
                if let Some(m) = &g.model {
                    r.flags |= W_GPU_MODEL;
                    r.gpu_class = *table.spec_model_index.entry(m.clone()).or_insert_with(|| {
                        *new_model = true;
                        table.spec_models.push(m.clone());
                        (table.spec_models.len() - 1) as u32
                    });
                }
            }
            if let Some(c) = &s.cpu {
                r.flags |= W_HAS_CPU;
                if let Some(n) = c.cores { r.flags |= W_CPU_CORES; r.cpu_cores = n; }
            }
            if let Some(v) = s.ram_mb { r.flags |= W_RAM; r.ram = v; }
            if let Some(v) = s.storage_gb { r.flags |= W_STORAGE; r.storage = v; }
        }
        r
    }

    /// Called every management interval with `store_context.node_store.get_nodes()` (node_store.rs:163-209).
    /// Sends only what changed: new nodes are appended, changed rows rewritten, departed nodes tombstoned.
    pub fn sync_nodes(&self, snapshot: &[OrchestratorNode]) -> Result<()> {
        let mut t = self.nodes.write();
        let mut new_model = false;
        let mut seen = vec![false; t.rows.len()];
        let mut appended = RowColumns::default();
        let (mut upd_idx, mut updated) = (Vec::<u32>::new(), RowColumns::default());
        for node in snapshot {
            let row = Self::project(node, &mut t, &mut new_model);
            match t.index.get(&node.address).copied() {
                Some(i) => {
                    let i = i as usize;
                    if i < seen.len() { seen[i] = true; }   // (an address twice in one snapshot: the second one finds the row just appended)
                    t.p2p_ids[i] = node.p2p_id.clone().unwrap_or_default();
                    if t.rows[i] != row || !t.present[i] {
                        t.rows[i] = row.clone();
                        t.present[i] = true;
                        if i < seen.len() {
                            upd_idx.push(i as u32);
                            updated.push(&row, 0);      // ranks are replaced wholesale below when they change
                        }
                    }
                }
                None => {
                    let i = t.rows.len() as u32;
                    t.index.insert(node.address, i);
                    t.addresses.push(node.address);
                    t.address_strings.push(node.address.to_string());
                    t.p2p_ids.push(node.p2p_id.clone().unwrap_or_default());
                    t.rows.push(row.clone());
                    t.present.push(true);
                    if t.book_on {  // (no sorted list: the engine ranks the texts it computes; book_sync fetches this row's)
                        let bytes: [u8; 20] = node.address.into_array();  // (an Address IS its bytes: nothing to parse on this side)
                        t.book_bytes.extend_from_slice(&bytes);
                        t.book_by_bytes.insert(bytes, i);
                    } else {
                        let key = &t.address_strings[i as usize];
                        let at = t.by_address.partition_point(|&j| t.address_strings[j as usize] < *key);
                        t.by_address.insert(at, i);
                    }
                    appended.push(&row, i);
                }
            }
        }
        let n_rows = t.rows.len();
        t.beats.resize_with(n_rows, || AtomicU64::new(0));  // (the beat column covers every row a beat can find in the index)
        // The row map above is the plugin's truth from here on; the engine calls below bring the engine's worker table
        // to it.  If one of them fails the two have diverged: the next interval then re-sends the whole table.
        if t.engine_rows_stale {
            // Every row again, in row order — the order the engine has its own in, with the rows it never received
            // behind them: pm_upload_workers(keep_groups = 1) keeps the standing groups, their claims and the id stream
            // (rows never move, so a group's row indices are as valid as before).  Then the deaths the engine may have
            // missed: every row that is not in the store, as dead — a no-op for a row in no group, the reference's
            // dissolution (and its send_group_destroyed) for the others.
            // (book on: the ranks the engine gave last, a new row's own index behind them — all replaced by book_sync right below)
            let mut ranks = if t.book_on { t.book_ranks.clone() } else { Self::address_ranks(&t.by_address, t.rows.len()) };
            for i in ranks.len()..t.rows.len() { ranks.push(i as u32); }
            for i in 0..seen.len() { if !seen[i] { t.present[i] = false; } }
            let mut all = RowColumns::default();
            let (mut gone, mut gone_flags) = (Vec::<u32>::new(), Vec::<u32>::new());
            for i in 0..t.rows.len() {
                if !t.present[i] {
                    t.rows[i].flags &= !W_HEALTHY;
                    gone.push(i as u32);
                    gone_flags.push(t.rows[i].flags);
                }
                let row = t.rows[i].clone();
                all.push(&row, ranks[i]);
            }
            self.push_model_table(&t);
            check(unsafe { pm_upload_workers(self.engine, &all.soa(), 1) })?;
            if t.book_on { self.book_sync(&mut t, 0, true)?; }  // (every row's bytes again: the engine may have missed any of them)
            if !gone.is_empty() {
                let dead = vec![1u32; gone.len()];
                check(unsafe { pm_on_worker_status_many(self.engine, gone.as_ptr(), gone_flags.as_ptr(), dead.as_ptr(), gone.len() as u32) })?;
            }
            t.engine_rows_stale = false;
            self.nodes_synced.store(true, Ordering::Release);
            drop(t);
            return self.emit_group_webhooks();
        }
        t.engine_rows_stale = true;     // (cleared behind the last engine call below: every `?` in between leaves it set)
        if new_model { self.push_model_table(&t); }
        // nodes that left the store: tombstone (their group dissolves, like a death; status_update_impl.rs:17-29)
        let (mut gone, mut gone_flags) = (Vec::<u32>::new(), Vec::<u32>::new());
        for i in 0..seen.len() {
            if !seen[i] && t.present[i] {
                t.present[i] = false;
                t.rows[i].flags &= !W_HEALTHY;
                gone.push(i as u32);
                gone_flags.push(t.rows[i].flags);
            }
        }
        if !gone.is_empty() {
            let dead = vec![1u32; gone.len()];
            check(unsafe { pm_on_worker_status_many(self.engine, gone.as_ptr(), gone_flags.as_ptr(), dead.as_ptr(), gone.len() as u32) })?;
        }
        if !upd_idx.is_empty() {
            // keep the ranks the engine already has for rewritten rows (ranks among the rows it knows: the new
            // ones of this snapshot are sent behind this call)
            // (book on: the ranks pm_addresses_rank gave last are the ones the engine has)
            let ranks = if t.book_on { t.book_ranks.clone() } else { Self::address_ranks(&t.by_address, seen.len()) };
            for (k, &i) in upd_idx.iter().enumerate() { updated.addr_rank[k] = ranks.get(i as usize).copied().unwrap_or(i); }
            check(unsafe { pm_update_workers(self.engine, upd_idx.as_ptr(), &updated.soa()) })?;
        }
        if !appended.flags.is_empty() {
            // (a row appended by this very snapshot may have been rewritten by a later entry of it: send what it is now)
            for k in 0..appended.flags.len() {
                let r = t.rows[seen.len() + k].clone();
                appended.flags[k] = r.flags; appended.gpu_count[k] = r.gpu_count; appended.gpu_mem[k] = r.gpu_mem;
                appended.gpu_class[k] = r.gpu_class; appended.cpu_cores[k] = r.cpu_cores; appended.ram[k] = r.ram;
                appended.storage[k] = r.storage; appended.lat[k] = r.lat; appended.lon[k] = r.lon;
            }
            let mut first = 0u32;
            check(unsafe { pm_append_workers(self.engine, &appended.soa(), &mut first) })?;
            if first as usize != seen.len() {
                return Err(anyhow!("pm_engine error {PM_ESTATE}: the engine's worker table and the plugin's row map disagree"));
            }
            if t.book_on {
                self.book_sync(&mut t, first, false)?;  // the new rows' bytes, pm_addresses_rank, the new rows' texts
            } else {
                // a new address shifts the global ranks of the others: GROUP_INDEX only needs the relative order
                let ranks = Self::address_ranks(&t.by_address, t.rows.len());
                check(unsafe { pm_set_addr_ranks(self.engine, ranks.as_ptr(), ranks.len() as u32) })?;
            }
        }
        t.engine_rows_stale = false;
        self.nodes_synced.store(true, Ordering::Release);
        drop(t);
        self.emit_group_webhooks()      // tombstoned nodes dissolved their groups
    }

    // ---- address book (gpu_match_addresses.cpp, statement for statement; INTEGRATION.md "Address book")

    /// (the node write lock is held.)  The bytes of the rows [first, end) — or of every row — go up, the engine ranks its texts,
    /// and the rows that render no device text yet get theirs: 43 bytes a new row come back, once.  (alloy's Display gives the
    /// same text; taking the device's keeps one source for what is ranked and what is shown, as the C++ twin must.)
    fn book_sync(&self, t: &mut NodeTable, first: u32, all: bool) -> Result<()> {
        let w = t.rows.len() as u32;
        if t.book_bytes.len() != 20 * w as usize {
            return Err(anyhow!("pm_engine error {PM_ESTATE}: the address book and the plugin's row map disagree"));
        }
        let from = if all { 0 } else { first };
        if from < w {
            check(unsafe { pm_addresses_set(self.engine, from, t.book_bytes.as_ptr().add(20 * from as usize), w - from) })?;
        }
        if w == 0 { return Ok(()); }
        t.book_ranks.resize(w as usize, 0);
        check(unsafe { pm_addresses_rank(self.engine, t.book_ranks.as_mut_ptr()) })?;  // (kept: a rewritten row is sent with the rank it has)
        if t.book_texts < w as usize {
            let rows: Vec<u32> = (t.book_texts as u32..w).collect();
            let mut text = vec![0 as c_char; 43 * rows.len()];
            check(unsafe { pm_addresses_text(self.engine, rows.as_ptr(), rows.len() as u32, text.as_mut_ptr()) })?;
            for (k, &row) in rows.iter().enumerate() {
                let bytes: Vec<u8> = text[43 * k..43 * k + 42].iter().map(|&c| c as u8).collect();
                t.address_strings[row as usize] = String::from_utf8_lossy(&bytes).into_owned();
            }
            t.book_texts = w as usize;
        }
        Ok(())
    }

    /// Off by default.  With the book on sync_nodes sends only the new rows' bytes and calls pm_addresses_rank where it kept
    /// `by_address` sorted and replaced the whole rank column; with rows already known: sends them all, ranks, fetches their texts.
    pub fn enable_address_book(&self) -> Result<()> {
        let mut t = self.nodes.write();
        if t.book_on { return Ok(()); }
        let (mut bytes, mut by_bytes) = (Vec::<u8>::new(), HashMap::<[u8; 20], u32>::new());
        for (i, a) in t.addresses.iter().enumerate() {
            let b: [u8; 20] = a.into_array();
            bytes.extend_from_slice(&b);
            by_bytes.insert(b, i as u32);
        }
        check(unsafe { pm_addresses_enable(self.engine, 1) })?;
        t.book_on = true;
        t.book_bytes = bytes;
        t.book_by_bytes = by_bytes;
        t.book_texts = 0;
        t.book_ranks.clear();
        t.by_address.clear();  // (not kept any more: row_of_address_text goes by the bytes)
        if !t.rows.is_empty() && self.nodes_synced.load(Ordering::Acquire) && !t.engine_rows_stale { self.book_sync(&mut t, 0, true)?; }
        Ok(())
    }

    pub fn address_book_enabled(&self) -> bool { self.nodes.read().book_on }

    /// NodeInviter::generate_invite up to the signature (node/invite.rs:86-115), for the nodes uninvited_nodes() lists, in its
    /// order: (address text, nonce, digest, signing hash).  `nonce` is asked once per node (rand::random there), expiration_s
    /// is the caller's clock; wallet.signer.sign_hash(signing hash) is the step that stays with the wallet.
    pub fn invite_digests(&self, domain_id: u32, pool_id: u32, mut nonce: impl FnMut() -> [u8; 32], expiration_s: u64)
                          -> Result<Vec<(String, [u8; 32], [u8; 32], [u8; 32])>> {
        let t = self.nodes.read();
        if !t.book_on { return Err(anyhow!("pm_engine error {PM_ESTATE}: the address book is off (enable_address_book)")); }
        let q = pm_dir_query { status_mask: 1u32 << NS_DISCOVERED, membership: DIR_ANY, order: DIR_BY_ROW, offset: 0, limit: u32::MAX };
        let mut total = 0u32;
        let listed = self.directory_locked(&t, &q, &mut total, None)?;
        let n = listed.len();
        if n == 0 { return Ok(Vec::new()); }
        let rows: Vec<u32> = listed.iter().map(|r| r.worker).collect();
        let nonces: Vec<[u8; 32]> = (0..n).map(|_| nonce()).collect();
        let flat: Vec<u8> = nonces.iter().flatten().copied().collect();
        let expiration = vec![expiration_s; n];
        let (mut digest, mut signing) = (vec![0u8; 32 * n], vec![0u8; 32 * n]);
        check(unsafe { pm_invite_digests(self.engine, domain_id, pool_id, rows.as_ptr(), n as u32, flat.as_ptr(), expiration.as_ptr(),
                                         digest.as_mut_ptr(), signing.as_mut_ptr()) })?;
        Ok((0..n).map(|k| {
            let (mut d, mut s) = ([0u8; 32], [0u8; 32]);
            d.copy_from_slice(&digest[32 * k..32 * k + 32]);
            s.copy_from_slice(&signing[32 * k..32 * k + 32]);
            (t.address_strings[rows[k] as usize].clone(), nonces[k], d, s)
        }).collect())
    }

    /// ValidateSignature (auth_signature_middleware.rs:374-422) and the heartbeat handler's ban check (routes/heartbeat.rs:38-52)
    /// for a batch of requests in ONE engine call: (message = path + payload string as the middleware formats it, the parsed
    /// signature as its 65 bytes r | s | v, the parsed x-address).  alloy has parsed both headers before this is called, so no
    /// flag is set here: INVALID_SIGNATURE_FORMAT and INVALID_ADDRESS_FORMAT of a header that does not parse are the caller's.
    /// The verdict's row is the plugin's row: beat, report_task and beat_metrics can be fed from it.  The rate limit, the
    /// request's age and the nonce (:424-483) stay with the caller.  Needs enable_address_book.
    pub fn verify_requests(&self, requests: &[(&[u8], [u8; 65], Address)]) -> Result<(Vec<pm_rq_verdict>, [u32; RQ_N_CODES])> {
        let t = self.nodes.read();
        if !t.book_on { return Err(anyhow!("pm_engine error {PM_ESTATE}: the address book is off (enable_address_book)")); }
        let n = requests.len();
        let mut counts = [0u32; RQ_N_CODES];
        if n == 0 { return Ok((Vec::new(), counts)); }
        let (mut bytes, mut offsets) = (Vec::<u8>::new(), vec![0u32; n + 1]);
        let (mut sig, mut claimed) = (Vec::<u8>::with_capacity(65 * n), Vec::<u8>::with_capacity(20 * n));
        for (k, (message, signature, address)) in requests.iter().enumerate() {
            bytes.extend_from_slice(message);
            if bytes.len() > 0xFFFF_FF00 { return Err(anyhow!("pm_engine error {PM_ERANGE}: too many message bytes in one call")); }
            offsets[k + 1] = bytes.len() as u32;
            sig.extend_from_slice(signature);
            let a: [u8; 20] = address.into_array();
            claimed.extend_from_slice(&a);
        }
        let mut out = vec![pm_rq_verdict::default(); n];
        check(unsafe { pm_verify_requests(self.engine, bytes.as_ptr(), offsets.as_ptr(), sig.as_ptr(), claimed.as_ptr(), std::ptr::null(),
                                          n as u32, out.as_mut_ptr(), counts.as_mut_ptr()) })?;
        Ok((out, counts))
    }

    /// Turns the engine's admission ledger on (pm_admission_enable): the rate windows, the nonce set and the beat column on the
    /// device.  From then on sweep_statuses sweeps over the later of the device's column and the plugin's own
    /// (pm_liveness_sweep_beats), so beat() keeps working.  Needs enable_address_book.
    pub fn enable_admission(&self) -> Result<()> {
        let mut t = self.nodes.write();       // (LOCK ORDER: nodes, the engine)
        if !t.book_on { return Err(anyhow!("pm_engine error {PM_ESTATE}: the address book is off (enable_address_book)")); }
        check(unsafe { pm_admission_enable(self.engine, 1) })?;
        t.admission_on = true;
        Ok(())
    }

    /// The whole of the middleware behind its signature check (auth_signature_middleware.rs:424-483: rate limit, age, nonce) and
    /// the heartbeat handler's stamp, for a batch in ONE engine call, handled as if one after another in batch order, all at
    /// now_ms: (message, signature, x-address, the timestamp the middleware read or None, the nonce or None, the route is
    /// /heartbeat).  An OK heartbeat stamps its row's beat on the device.  Needs enable_admission.
    #[allow(clippy::type_complexity)]
    pub fn admit_requests(&self, requests: &[(&[u8], [u8; 65], Address, Option<u64>, Option<&str>, bool)], now_ms: u64)
                          -> Result<(Vec<pm_rq_verdict>, [u32; AD_N_CODES])> {
        let t = self.nodes.read();
        if !t.book_on { return Err(anyhow!("pm_engine error {PM_ESTATE}: the address book is off (enable_address_book)")); }
        if !t.admission_on { return Err(anyhow!("pm_engine error {PM_ESTATE}: admission is off (enable_admission)")); }
        let n = requests.len();
        let mut counts = [0u32; AD_N_CODES];
        if n == 0 { return Ok((Vec::new(), counts)); }
        let (mut bytes, mut offsets) = (Vec::<u8>::new(), vec![0u32; n + 1]);
        let (mut nonces, mut nonce_offsets) = (Vec::<u8>::new(), vec![0u32; n + 1]);
        let (mut sig, mut claimed) = (Vec::<u8>::with_capacity(65 * n), Vec::<u8>::with_capacity(20 * n));
        let (mut flags, mut timestamps) = (vec![0u8; n], vec![0u64; n]);
        for (k, (message, signature, address, timestamp, nonce, heartbeat)) in requests.iter().enumerate() {
            bytes.extend_from_slice(message);
            if bytes.len() > 0xFFFF_FF00 { return Err(anyhow!("pm_engine error {PM_ERANGE}: too many message bytes in one call")); }
            offsets[k + 1] = bytes.len() as u32;
            sig.extend_from_slice(signature);
            let a: [u8; 20] = address.into_array();
            claimed.extend_from_slice(&a);
            match timestamp { Some(ts) => timestamps[k] = *ts, None => flags[k] |= RQ_FLAG_NO_TIMESTAMP }
            match nonce { Some(text) => nonces.extend_from_slice(text.as_bytes()), None => flags[k] |= RQ_FLAG_NO_NONCE }
            if nonces.len() > 0xFFFF_FF00 { return Err(anyhow!("pm_engine error {PM_ERANGE}: too many nonce bytes in one call")); }
            nonce_offsets[k + 1] = nonces.len() as u32;
            if *heartbeat { flags[k] |= RQ_FLAG_BEAT; }
        }
        nonces.push(0);  // (never read: a batch without a nonce still has an address)
        let mut out = vec![pm_rq_verdict::default(); n];
        check(unsafe { pm_admit_requests(self.engine, now_ms, bytes.as_ptr(), offsets.as_ptr(), sig.as_ptr(), claimed.as_ptr(),
                                         flags.as_ptr(), timestamps.as_ptr(), nonces.as_ptr(), nonce_offsets.as_ptr(), n as u32,
                                         out.as_mut_ptr(), counts.as_mut_ptr()) })?;
        Ok((out, counts))
    }

    /// rank of address.to_string() in byte order (BTreeSet<String>, mod.rs:424-434) among the first `known` rows:
    /// one pass over the sorted row list (no string is compared here; the list is kept sorted as nodes arrive)
    fn address_ranks(by_address: &[u32], known: usize) -> Vec<u32> {
        let mut rank = vec![0u32; known];
        let mut r = 0u32;
        for &i in by_address {
            if (i as usize) < known { rank[i as usize] = r; r += 1; }
        }
        rank
    }

    /// scheduler_impl.rs:44-59: any None on the way => every configuration allowed (None).  "Unrestricted" is not a
    /// mask value: with 64 configurations a task that names all of them has mask u64::MAX too, and still enables them.
    fn topology_mask(&self, t: &Task) -> Option<u64> {
        let list = t.scheduling_config.as_ref().and_then(|c| c.plugins.as_ref())
            .and_then(|p| p.get("node_groups")).and_then(|n| n.get("allowed_topologies"))?;
        Some(list.iter().filter_map(|name| self.config_names.iter().position(|c| c == name)).fold(0, |m, i| m | (1u64 << i)))
    }

    /// the engine's task mask: an unrestricted task selects every configuration
    fn engine_mask(&self, t: &Task) -> u64 { self.topology_mask(t).unwrap_or(u64::MAX) }

    fn push_enabled(&self, tasks: &[Task]) -> Result<()> {
        // available_node_group_configs: every topology some task names (on_task_created, mod.rs:1224-1243)
        let enabled = tasks.iter().filter_map(|t| self.topology_mask(t)).fold(0u64, |a, m| a | m);
        check(unsafe { pm_set_enabled_mask(self.engine, enabled) })?;
        self.enabled_mask.store(enabled, Ordering::Release);
        Ok(())
    }

    // LOCK ORDER: `nodes`, then `tasks`, then the engine's own mutex (taken inside every pm_* call but the look-up).
    // The engine reports a task as a POSITION in `tasks`, and it re-derives the published positions inside
    // pm_tasks_insert_front / pm_tasks_delete / pm_upload_tasks — so the Vec and the engine's table change under ONE
    // write lock, and filter_tasks holds the read lock from the look-up to the index: a heartbeat never pairs a
    // position of the new table with the old Vec (or the other way round).  (The reference binds group -> task by id,
    // scheduler_impl.rs:62-82, and has no such window; this is what keeps the shim from having one.)

    /// the snapshot upload with `tasks` already locked for writing
    fn sync_tasks_locked(&self, guard: &mut Vec<Task>, tasks: Vec<Task>) -> Result<()> {
        let masks: Vec<u64> = tasks.iter().map(|t| self.engine_mask(t)).collect();
        let created: Vec<i64> = tasks.iter().map(|t| t.created_at).collect();
        let uid: Vec<u64> = tasks.iter().map(task_uid).collect();
        let soa = pm_task_soa { n: tasks.len() as u32, topo_mask: masks.as_ptr(), created_at: created.as_ptr(), uid: uid.as_ptr() };
        check(unsafe { pm_upload_tasks(self.engine, &soa) })?;
        self.push_enabled(&tasks)?;
        *guard = tasks;
        self.tasks_synced.store(true, Ordering::Release);
        Ok(())
    }

    /// Full snapshot: `task_store.get_all_tasks()` (task_store.rs:57-82, already created_at-desc).  Start-up and
    /// the fallback when a delta does not apply.
    pub fn sync_tasks(&self, tasks: Vec<Task>) -> Result<()> {
        let mut guard = self.tasks.write();
        self.sync_tasks_locked(&mut guard, tasks)
    }

    /// TaskStore observer (task_store.rs:46-52 -> on_task_created, mod.rs:1224-1243): the new task is the newest, so
    /// it goes in front; only this row travels to the GPU.  Equal or older timestamps fall back to the snapshot.
    pub fn on_task_created(&self, task: &Task, all_tasks: impl FnOnce() -> Vec<Task>) -> Result<()> {
        let (mask, created, uid) = (self.engine_mask(task), task.created_at, task_uid(task));
        let soa = pm_task_soa { n: 1, topo_mask: &mask, created_at: &created, uid: &uid };
        let mut tasks = self.tasks.write();                 // (before the engine call: see LOCK ORDER)
        let rc = if self.republish_on_insert { unsafe { pm_tasks_insert_front_ex(self.engine, &soa, 1) } }
                 else { unsafe { pm_tasks_insert_front(self.engine, &soa) } };
        if rc != 0 { return self.sync_tasks_locked(&mut tasks, all_tasks()); }
        tasks.insert(0, task.clone());
        self.push_enabled(&tasks)
    }

    /// on_task_deleted (mod.rs:1245-1325): the engine dissolves every group that had claimed the task.
    pub fn on_task_deleted(&self, task: &Task) -> Result<()> {
        let uid = task_uid(task);
        let mut n = 0u32;
        let mut tasks = self.tasks.write();                 // (before the engine call: see LOCK ORDER)
        check(unsafe { pm_tasks_delete(self.engine, &uid, 1, &mut n) })?;
        tasks.retain(|t| t.id != task.id);
        self.push_enabled(&tasks)?;
        drop(tasks);
        self.emit_group_webhooks()      // dissolve_group's send_group_destroyed, mod.rs:1469-1481
    }

    /// One body of run_group_management_loop (mod.rs:180-203) + every worker's filter_tasks, then the webhooks the
    /// reference sends from inside try_form_new_groups / execute_group_merge (mod.rs:612-625, 974-1000).
    pub fn tick(&self) -> Result<pm_stats> {
        self.ticked.store(true, Ordering::Release);
        let mut s = pm_stats::default();
        check(unsafe { pm_tick(self.engine, &mut s) })?;
        self.emit_group_webhooks()?;
        Ok(s)
    }

    /// The management interval of ONE pool matched by several GPUs, one process per GPU: this plugin is rank comm.rank()
    /// of comm.world().  Every rank is fed every store event (sync_nodes, the task observers, status changes — replicated
    /// calls) and calls tick_dist at the same point of its loop; every rank ends with the identical groups and the full
    /// published table (any rank answers any heartbeat).  The five calls of INTEGRATION.md "Multi-GPU" around ONE
    /// all-gather.  From its first tick_dist on a plugin of rank > 0 delivers no webhooks (rank 0 reports them).
    pub fn tick_dist(&self, comm: &dyn AllGather) -> Result<pm_stats> {
        let (rank, world) = (comm.rank(), comm.world());
        if world == 0 || rank >= world { return Err(anyhow!("tick_dist: rank outside the communicator")); }
        self.ticked.store(true, Ordering::Release);
        {
            let t = self.nodes.read();
            let mut d = self.dist.lock();
            if d.stream != comm.stream() {
                // the engine's kernels and the collective on one stream: no host wait between them
                check(unsafe { pm_set_stream(self.engine, comm.stream()) })?;
                d.stream = comm.stream();
            }
            if rank != self.dist_rank.load(Ordering::Acquire) || world != d.world || t.rows.len() != d.rows {
                // ownership is per row and every rank computes the same: a hash of the address, nothing is negotiated
                let shard: Vec<u8> = t.addresses.iter().map(|a| shard_of(a, world) as u8).collect();
                check(unsafe { pm_dist_configure(self.engine, rank, world, if shard.is_empty() { std::ptr::null() } else { shard.as_ptr() }) })?;
                self.dist_rank.store(rank, Ordering::Release);
                d.world = world;
                d.rows = if t.engine_rows_stale { usize::MAX } else { t.rows.len() };  // (the engine is behind the row map: configure again next time)
            }
        }
        let (mut s, mut x) = (pm_stats::default(), pm_dist_xfer::default());
        check(unsafe { pm_dist_tick_begin(self.engine) })?;      // compat sweep; the whole carve is started (replicated)
        check(unsafe { pm_dist_carve_wait(self.engine) })?;      // waits for it; near-ties settled on the host, identically everywhere
        check(unsafe { pm_dist_match_begin(self.engine, &mut x) })?;   // solo merge, pair sweep + claim of the OWNED workers
        if x.bytes_per_rank != 0 {                               // the ONE exchange of a tick: the published rows
            comm.all_gather(x.send_ptr as usize as *const c_void, x.recv_ptr as usize as *mut c_void, x.bytes_per_rank as usize)?;
        }
        check(unsafe { pm_dist_tick_end(self.engine, &mut s) })?;   // scatter into the full table, publish
        self.emit_group_webhooks()?;
        Ok(s)
    }

    /// Drains the engine's group life-cycle feed into send_group_created / send_group_destroyed, in the order the
    /// reference emits them.  Runs after everything that can create or dissolve groups: tick, handle_status_change,
    /// on_task_deleted, sync_nodes (tombstones).  (pm_enable_group_events(1) in `new`.)
    fn emit_group_webhooks(&self) -> Result<()> {
        let (mut ne, mut nm) = (0u32, 0u32);
        let rc = unsafe { pm_drain_group_events(self.engine, std::ptr::null_mut(), 0, std::ptr::null_mut(), 0, &mut ne, &mut nm) };
        if rc == 0 { return Ok(()); }                       // empty log
        // (another thread may log events between the size query and the drain: grow and try again; a drain that
        // still fails is logged and left for the next call — it is not the tick that failed)
        let (mut events, mut members) = (Vec::new(), Vec::new());
        for _ in 0..8 {
            events.resize(ne as usize, pm_group_event::default());
            members.resize(nm as usize, 0u32);
            let (cap_e, cap_m) = (ne, nm);
            let rc = unsafe { pm_drain_group_events(self.engine, events.as_mut_ptr(), cap_e, members.as_mut_ptr(), cap_m, &mut ne, &mut nm) };
            if rc == 0 { break; }
            if rc != PM_ERANGE { log::error!("pm_drain_group_events: {rc}"); return Ok(()); }
        }
        if events.len() < ne as usize { log::error!("group events kept for the next drain"); return Ok(()); }
        {   // NodeGroup.created_at (mod.rs:575): the clock at the report of the creation
            let now = chrono::Utc::now();
            let mut stamps = self.group_created_at.lock();
            for ev in &events[..ne as usize] {
                if ev.kind == 1 { stamps.insert(ev.group_id, now); } else { stamps.remove(&ev.group_id); }
            }
        }
        let Some(plugins) = &self.webhook_plugins else { return Ok(()) };
        if self.dist_rank.load(Ordering::Acquire) != 0 { return Ok(()); }     // a rank > 0 of a multi-GPU pool: rank 0 reports
        let t = self.nodes.read();
        for ev in &events[..ne as usize] {
            let id = format!("{:x}", ev.group_id);                                   // generate_group_id, mod.rs:1489-1493
            let name = self.config_names[ev.config as usize].clone();
            let nodes: Vec<String> = members[ev.member_begin as usize..(ev.member_begin + ev.n_members) as usize]
                .iter().map(|&w| t.address_strings[w as usize].clone()).collect();  // group.nodes order
            for p in plugins {
                let r = if ev.kind == 1 { p.send_group_created(id.clone(), name.clone(), nodes.clone()) }
                        else { p.send_group_destroyed(id.clone(), name.clone(), nodes.clone()) };
                if let Err(e) = r { log::error!("Failed to send group webhook: {e}"); }   // as in the reference: logged, not fatal
            }
        }
        Ok(())
    }

    fn render(f: impl Fn(*mut c_char, usize, *mut usize) -> i32) -> Result<String> {
        let mut need = 0usize;
        check(f(std::ptr::null_mut(), 0, &mut need))?;
        let mut buf = vec![0u8; need];
        check(f(buf.as_mut_ptr() as *mut c_char, need, &mut need))?;
        buf.pop();
        Ok(String::from_utf8(buf)?)
    }

    /// (The positions pm_lookup_task_for_worker reports index `tasks` as it is NOW: the engine re-derives the published
    /// positions inside pm_tasks_insert_front / pm_tasks_delete / pm_upload_tasks, and clears the rows of a group that a
    /// deleted task or a dead node dissolved — no tick needed in between.)
    /// SchedulerPlugin::filter_tasks (plugins/mod.rs:66-78): lock-free lookup + the `${...}` templating the
    /// reference does at scheduler_impl.rs:112-205 (GROUP_INDEX, GROUP_SIZE, NEXT_P2P_ADDRESS, GROUP_ID, upload count).
    /// `_tasks` is ignored — and with the edit of `Scheduler::get_task_for_node` shown in INTEGRATION.md ("The task list
    /// per heartbeat") the scheduler does not even load it: the plugin serves from its own copy, kept current by the
    /// task observers.
    pub(crate) fn filter_tasks(&self, _tasks: &[Task], node_address: &Address) -> Result<Vec<Task>> {
        let nodes = self.nodes.read();
        let Some(&w) = nodes.index.get(node_address) else { return Ok(vec![]) };
        let mut a = pm_assignment::default();
        let tasks = self.tasks.read();                      // held from the look-up to the index (see LOCK ORDER)
        if unsafe { pm_lookup_task_for_worker(self.engine, w, &mut a) } != 0 || a.task == PM_NONE {
            return Ok(vec![]);
        }
        let Some(mut task) = tasks.get(a.task as usize).cloned() else { return Ok(vec![]) };
        drop(tasks);
        let group_id = format!("{:x}", a.group_id);                                   // generate_group_id, mod.rs:1489-1493
        let gid = CString::new(group_id.as_str())?;
        let next = CString::new(nodes.p2p_ids.get(a.next_worker as usize).cloned().unwrap_or_default())?;
        let count = CString::new((self.upload_counter)(node_address, &group_id).to_string())?;
        let vars = pm_group_vars { group_index: a.group_index, group_size: a.group_size,
            next_p2p_address: next.as_ptr(), group_id: gid.as_ptr(), total_upload_count: count.as_ptr() };
        let group_vars = |s: &str| -> Result<String> {
            let cin = CString::new(s)?;
            Self::render(|o, c, n| unsafe { pm_host_group_vars(cin.as_ptr(), &vars, o, c, n) })
        };
        let env = task.env_vars.get_or_insert_with(Default::default);
        env.insert("GROUP_INDEX".to_string(), a.group_index.to_string());             // scheduler_impl.rs:161
        for (_, v) in env.iter_mut() { *v = group_vars(v)?; }
        if let Some(cmd) = task.cmd.as_mut() { for arg in cmd.iter_mut() { *arg = group_vars(arg)?; } }
        if let Some(mounts) = task.volume_mounts.as_mut() {                           // scheduler_impl.rs:185-200
            for m in mounts.iter_mut() {
                for path in [&mut m.host_path, &mut m.container_path] {
                    let cin = CString::new(path.as_str())?;
                    *path = Self::render(|o, c, n| unsafe { pm_host_volume_vars(cin.as_ptr(), gid.as_ptr(), o, c, n) })?;
                }
            }
        }
        Ok(vec![task])
    }

    // ------------------------------------------------------------------------------------------------ the read surface
    // What the API routes call on AppState.node_groups_plugin, with the reference's names and result types
    // (node_groups/mod.rs:324-434, :1002-1065).  `async` only because the reference's are (the routes `.await` them):
    // nothing here waits for anything but the engine's mutex.

    /// one snapshot of the engine's group list: (group_of per row or empty, groups, members)
    fn snapshot_groups(&self, rows: usize, want_group_of: bool) -> Result<(Vec<i32>, Vec<pm_group>, Vec<u32>)> {
        for _ in 0..8 {      // (a tick between the size query and the copy: ask again)
            let (mut ng, mut nm) = (0u32, 0u32);
            check(unsafe { pm_get_groups(self.engine, std::ptr::null_mut(), std::ptr::null_mut(), 0, &mut ng, std::ptr::null_mut(), 0, &mut nm) })?;
            let mut groups = vec![pm_group::default(); ng as usize];
            let mut members = vec![0u32; nm as usize];
            // (group_of_worker gets W entries, W the ENGINE's row count: never more than the plugin's, whose lock the caller holds)
            let mut group_of = if want_group_of { vec![-1i32; rows] } else { Vec::new() };
            let gp = if want_group_of && rows > 0 { group_of.as_mut_ptr() } else { std::ptr::null_mut() };
            let rc = unsafe { pm_get_groups(self.engine, gp, groups.as_mut_ptr(), ng, &mut ng, members.as_mut_ptr(), nm, &mut nm) };
            if rc == 0 {
                groups.truncate(ng as usize);
                members.truncate(nm as usize);
                return Ok((group_of, groups, members));
            }
            if rc != PM_ERANGE { check(rc)?; }
        }
        Err(anyhow!("the group list kept changing under pm_get_groups"))
    }

    fn make_group(&self, t: &NodeTable, g: &pm_group, members: &[u32]) -> NodeGroup {
        let created_at = self.group_created_at.lock().get(&g.id).copied().unwrap_or_else(chrono::Utc::now);
        NodeGroup {
            id: format!("{:x}", g.id),                                                  // generate_group_id, mod.rs:1489-1493
            nodes: members.iter().map(|&w| t.address_strings[w as usize].clone()).collect::<BTreeSet<String>>(),
            created_at,
            configuration_name: self.config_names[g.config as usize].clone(),
        }
    }

    /// the inverse of format!("{:x}", u64): lower-case hex, no sign / prefix / leading zero (but "0"), <= 16 digits.
    /// Anything else is the text of no group id (a Redis key that does not exist in the reference).
    fn parse_group_id(s: &str) -> Option<u64> {
        if s.is_empty() || s.len() > 16 || (s.len() > 1 && s.starts_with('0')) { return None; }
        if !s.bytes().all(|c| c.is_ascii_digit() || (b'a'..=b'f').contains(&c)) { return None; }
        u64::from_str_radix(s, 16).ok()
    }

    /// the reference keys node_to_group by address TEXT: exact string match (binary search in the address-ordered rows)
    fn row_of_address_text(t: &NodeTable, text: &str) -> Option<u32> {
        if t.book_on {  // by the bytes: any spelling of the address finds the row
            let a: Address = text.parse().ok()?;
            return t.book_by_bytes.get(&a.into_array()).copied();
        }
        let at = t.by_address.partition_point(|&j| t.address_strings[j as usize].as_str() < text);
        t.by_address.get(at).copied().filter(|&j| t.address_strings[j as usize] == text)
    }

    fn one_group(&self, t: &NodeTable, call: impl Fn(*mut pm_group, *mut u32, u32, *mut u32) -> i32) -> Result<Option<NodeGroup>> {
        let (mut g, mut slot) = (pm_group::default(), PM_NONE);
        let mut members = vec![0u32; 64];
        let mut rc = call(&mut g, members.as_mut_ptr(), members.len() as u32, &mut slot);
        if rc == PM_ERANGE && slot != PM_NONE {          // a group of more than 64 nodes: its size is in the record
            members.resize(g.n_members as usize, 0);
            rc = call(&mut g, members.as_mut_ptr(), members.len() as u32, &mut slot);
        }
        if rc == PM_ERANGE && slot == PM_NONE { return Ok(None); }   // (a row the engine has not been sent yet: in no group)
        check(rc)?;
        if slot == PM_NONE { return Ok(None); }
        Ok(Some(self.make_group(t, &g, &members[..g.n_members as usize])))
    }

    /// get_all_groups (mod.rs:1006-1044): every group, sorted by id text (:1040)
    pub(crate) async fn get_all_groups(&self) -> Result<Vec<NodeGroup>, Error> {
        let t = self.nodes.read();
        let (_, groups, members) = self.snapshot_groups(t.rows.len(), false)?;
        let mut out: Vec<NodeGroup> = groups.iter()
            .map(|g| self.make_group(&t, g, &members[g.member_begin as usize..(g.member_begin + g.n_members) as usize])).collect();
        out.sort_by(|a, b| a.id.cmp(&b.id));
        Ok(out)
    }

    /// get_group_by_id (mod.rs:1046-1055)
    pub(crate) async fn get_group_by_id(&self, group_id: &str) -> Result<Option<NodeGroup>, Error> {
        let Some(id) = Self::parse_group_id(group_id) else { return Ok(None) };
        let t = self.nodes.read();
        self.one_group(&t, |g, m, cap, slot| unsafe { pm_get_group_by_id(self.engine, id, g, m, cap, slot) })
    }

    /// get_all_node_group_mappings (mod.rs:1057-1065): node address text -> group id text
    pub(crate) async fn get_all_node_group_mappings(&self) -> Result<HashMap<String, String>, Error> {
        let t = self.nodes.read();
        let (_, groups, members) = self.snapshot_groups(t.rows.len(), false)?;
        let mut out = HashMap::new();
        for g in &groups {
            let id = format!("{:x}", g.id);
            for &w in &members[g.member_begin as usize..(g.member_begin + g.n_members) as usize] {
                out.insert(t.address_strings[w as usize].clone(), id.clone());
            }
        }
        Ok(out)
    }

    /// get_node_group (mod.rs:324-337)
    pub async fn get_node_group(&self, node_addr: &str) -> Result<Option<NodeGroup>, Error> {
        let t = self.nodes.read();
        let Some(row) = Self::row_of_address_text(&t, node_addr) else { return Ok(None) };
        self.one_group(&t, |g, m, cap, slot| unsafe { pm_get_group_of_worker(self.engine, row, g, m, cap, slot) })
    }

    /// get_node_groups_batch (mod.rs:339-397): every asked address is a key of the result; one snapshot of the list
    pub async fn get_node_groups_batch(&self, node_addresses: &[String]) -> Result<HashMap<String, Option<NodeGroup>>, Error> {
        let mut result = HashMap::new();
        if node_addresses.is_empty() { return Ok(result); }                             // mod.rs:346-348
        let t = self.nodes.read();
        let (group_of, groups, members) = self.snapshot_groups(t.rows.len(), true)?;
        let mut made: HashMap<i32, NodeGroup> = HashMap::new();      // every group is built once (the reference MGETs the unique ids)
        for a in node_addresses {
            let gi = Self::row_of_address_text(&t, a).and_then(|r| group_of.get(r as usize).copied()).filter(|&g| g >= 0);
            let group = gi.map(|gi| made.entry(gi).or_insert_with(|| {
                let g = &groups[gi as usize];
                self.make_group(&t, g, &members[g.member_begin as usize..(g.member_begin + g.n_members) as usize])
            }).clone());
            result.insert(a.clone(), group);
        }
        Ok(result)
    }

    /// get_idx_in_group (mod.rs:424-434)
    pub fn get_idx_in_group(&self, node_group: &NodeGroup, node_addr: &str) -> Result<usize, Error> {
        if let Some(at) = node_group.nodes.iter().position(|n| n == node_addr) { return Ok(at); }
        // (book on: the group lists the device's texts; another spelling of a member's address is that member)
        let t = self.nodes.read();
        let shown = if t.book_on { Self::row_of_address_text(&t, node_addr).map(|row| t.address_strings[row as usize].clone()) } else { None };
        shown.and_then(|text| node_group.nodes.iter().position(|n| *n == text)).ok_or_else(|| anyhow!("Node {} not found in group", node_addr))
    }

    fn ordered_templates(&self, enabled: u64) -> Vec<NodeGroupConfiguration> {
        let mut order = vec![0u32; self.config_rows.len() + 1];
        let mut n = 0u32;
        let rc = unsafe { pm_host_config_order(self.config_rows.as_ptr(), self.config_rows.len() as u32, enabled, order.as_mut_ptr(), &mut n) };
        if rc != 0 { return vec![]; }                                                   // (the reference answers vec![] on a store error, mod.rs:400-402)
        order[..n as usize].iter().map(|&c| self.templates[c as usize].clone()).collect()
    }

    /// get_available_configurations (mod.rs:399-418): the templates some task names, min_group_size descending (stable)
    pub async fn get_available_configurations(&self) -> Vec<NodeGroupConfiguration> {
        self.ordered_templates(self.enabled_mask.load(Ordering::Acquire))
    }

    /// get_all_configuration_templates (mod.rs:420-422): in the constructor's order (mod.rs:150-164) = the carve order
    /// with nothing disabled
    pub fn get_all_configuration_templates(&self) -> Vec<NodeGroupConfiguration> {
        let c = self.config_rows.len();
        self.ordered_templates(if c >= 64 { u64::MAX } else { (1u64 << c) - 1 })
    }

    /// dissolve_group (mod.rs:1002-1004 -> :1423-1487): by id text; an id that names no group is Ok(()) ("No group found")
    pub(crate) async fn dissolve_group(&self, group_id: &str) -> Result<(), Error> {
        let Some(id) = Self::parse_group_id(group_id) else { return Ok(()) };
        let mut dissolved = 0u32;
        check(unsafe { pm_dissolve_group_by_id(self.engine, id, &mut dissolved) })?;
        if dissolved != 0 { self.emit_group_webhooks()?; }                              // send_group_destroyed, mod.rs:1469-1481
        Ok(())
    }

    /// Restart and switch-over: the groups the store holds (orchestrator:groups_index / node_group:<id> in
    /// get_all_groups order, group_task:<id>) into the engine — after sync_nodes and sync_tasks, before the first tick
    /// (PM_ESTATE at any other time).  A group that cannot be taken over is dropped and reported, not an error: an id that is
    /// not "{:x}" text, an unknown configuration name, an address outside the node table, a node of an earlier group, no
    /// nodes, more than max_group_size nodes, the id of an earlier group.  A group_task naming an unknown task leaves the
    /// group without one (get_current_group_task, mod.rs:436-469): task_cleared.  created_at is kept.  id_state None draws
    /// one from the OS (the reference's ids are random, mod.rs:1489-1493) — an error on a multi-GPU pool, whose ranks must
    /// draw the same ids.  Ends with one pm_match: heartbeats are served from the adopted groups at once.
    pub fn restore_groups(&self, groups: &[NodeGroup], group_tasks: &HashMap<String, String>, id_state: Option<u64>)
                          -> Result<RestoreReport> {
        if self.ticked.load(Ordering::Acquire) || !self.nodes_synced.load(Ordering::Acquire) || !self.tasks_synced.load(Ordering::Acquire) {
            return Err(anyhow!("pm_engine error {PM_ESTATE}: restore_groups: after sync_nodes and sync_tasks, before the first tick"));
        }
        if id_state.is_none() && (self.multi_gpu || self.dist.lock().world > 1) {
            return Err(anyhow!("restore_groups: the ranks of a multi-GPU pool must draw the same ids: pass id_state"));
        }
        let mut report = RestoreReport::default();
        let t = self.nodes.read();          // (LOCK ORDER: nodes, tasks, the engine)
        let tasks = self.tasks.read();
        let task_position: HashMap<String, u32> =
            tasks.iter().enumerate().rev().map(|(i, task)| (task.id.to_string(), i as u32)).collect();   // (first occurrence wins)
        let (mut records, mut members, mut created) = (Vec::<pm_group>::new(), Vec::<u32>::new(), Vec::new());
        let mut ids = std::collections::HashSet::new();
        let mut taken = vec![false; t.rows.len()];
        'groups: for g in groups {
            let Some(id) = Self::parse_group_id(&g.id) else {
                report.dropped.push((g.id.clone(), "the id is not the {:x} text of a u64".into()));
                continue;
            };
            let Some(cfg) = self.config_names.iter().position(|n| *n == g.configuration_name) else {
                report.dropped.push((g.id.clone(), format!("unknown configuration {}", g.configuration_name)));
                continue;
            };
            let mut rows = Vec::<u32>::new();
            for a in &g.nodes {
                let Some(row) = Self::row_of_address_text(&t, a) else {
                    report.dropped.push((g.id.clone(), format!("node {a} is not in the node table")));
                    continue 'groups;
                };
                if taken[row as usize] || rows.contains(&row) {
                    report.dropped.push((g.id.clone(), format!("node {a} is already in an earlier group")));
                    continue 'groups;
                }
                rows.push(row);
            }
            let max_size = self.templates[cfg].max_group_size;
            if rows.is_empty() || rows.len() > max_size {
                let why = if rows.is_empty() { "the group has no nodes".to_string() }
                          else { format!("{} nodes, more than max_group_size {}", rows.len(), max_size) };
                report.dropped.push((g.id.clone(), why));
                continue;
            }
            if !ids.insert(id) {
                report.dropped.push((g.id.clone(), "the id of an earlier group".into()));
                continue;
            }
            let mut task = PM_NONE;
            if let Some(task_id) = group_tasks.get(&g.id) {                              // get_current_group_task (mod.rs:436-469)
                match task_position.get(task_id) {
                    Some(&at) => task = at,
                    None => report.task_cleared.push(g.id.clone()),
                }
            }
            for &r in &rows { taken[r as usize] = true; }
            records.push(pm_group { id, config: cfg as u32, n_members: rows.len() as u32, member_begin: members.len() as u32, task });
            members.extend_from_slice(&rows);
            created.push((id, g.created_at));
        }
        let state = match id_state {
            Some(s) => s,
            None => rand::random::<u64>(),   // (generate_group_id draws from rand::rng(), mod.rs:1489-1493)
        };
        check(unsafe { pm_adopt_groups(self.engine, if records.is_empty() { std::ptr::null() } else { records.as_ptr() }, records.len() as u32,
                                       if members.is_empty() { std::ptr::null() } else { members.as_ptr() }, members.len() as u32, state) })?;
        {
            let mut stamps = self.group_created_at.lock();
            for (id, at) in created { stamps.insert(id, at); }
        }
        check(unsafe { pm_match(self.engine, std::ptr::null_mut(), std::ptr::null_mut()) })?;   // heartbeats served from here on
        Ok(report)
    }

    /// group id text -> task id of every group that holds a task (what group_task:<id> holds): the store's write-through
    pub fn group_tasks(&self) -> Result<HashMap<String, String>> {
        let t = self.nodes.read();
        let tasks = self.tasks.read();      // (task positions are positions in this Vec)
        let (_, groups, _) = self.snapshot_groups(t.rows.len(), false)?;
        Ok(groups.iter().filter(|g| g.task != PM_NONE && (g.task as usize) < tasks.len())
                 .map(|g| (format!("{:x}", g.id), tasks[g.task as usize].id.to_string())).collect())
    }

    /// the state of the group id stream, for a successor's restore_groups (persisted under a key of the plugin's own)
    pub fn group_id_state(&self) -> Result<u64> {
        let mut state = 0u64;
        check(unsafe { pm_group_id_state(self.engine, &mut state) })?;
        Ok(state)
    }

    // ---- diagnostics (INTEGRATION.md "Diagnostics"): the engine's three read-only reports by name

    /// why a node sits idle: None when the node table does not hold the address
    pub fn explain_node(&self, address: &str) -> Result<Option<NodeExplanation>> {
        let t = self.nodes.read();           // (LOCK ORDER: nodes, the engine)
        let Some(row) = Self::row_of_address_text(&t, address) else { return Ok(None) };
        let mut why = vec![0u8; self.config_names.len()];
        let mut state = 0u32;
        check(unsafe { pm_explain_workers(self.engine, &row, 1, if why.is_empty() { std::ptr::null_mut() } else { why.as_mut_ptr() },
                                          &mut state) })?;
        Ok(Some(NodeExplanation {
            state: state_name(state).to_string(),
            configs: why.iter().enumerate()
                        .map(|(c, &k)| (self.config_names[c].clone(), WHY_NAMES.get(k as usize).unwrap_or(&"unknown").to_string()))
                        .collect(),
        }))
    }

    /// how much room each configuration has left, constructor order
    pub fn configuration_report(&self) -> Result<Vec<ConfigurationReport>> {
        let mut rows = vec![pm_config_report_row::default(); self.config_names.len()];
        let mut n = 0u32;
        check(unsafe { pm_config_report(self.engine, if rows.is_empty() { std::ptr::null_mut() } else { rows.as_mut_ptr() },
                                        rows.len() as u32, &mut n) })?;
        Ok(rows.iter().take(n as usize).enumerate().map(|(c, r)| ConfigurationReport {
            name: self.config_names[c].clone(),
            enabled: r.enabled != 0,
            eligible_meets: r.eligible_meets,
            idle_meets: r.idle_meets,
            why: r.why,
            groups: r.groups,
            members: r.members,
            groups_without_task: r.groups_without_task,
            tasks_allowing: r.tasks_allowing,
        }).collect())
    }

    /// by task id, every task of the last sync_tasks / on_task_created / on_task_deleted
    pub fn task_report(&self) -> Result<HashMap<String, TaskReport>> {
        let tasks = self.tasks.read();      // (the engine's positions index this Vec)
        let n = tasks.len();
        let (mut running, mut workers, mut allowed) = (vec![0u32; n], vec![0u32; n], vec![0u32; n]);
        let ptr = |v: &mut Vec<u32>| if v.is_empty() { std::ptr::null_mut() } else { v.as_mut_ptr() };
        check(unsafe { pm_task_report(self.engine, ptr(&mut running), ptr(&mut workers), ptr(&mut allowed)) })?;
        Ok(tasks.iter().enumerate().map(|(i, t)| (t.id.to_string(), TaskReport {
            groups_running: running[i], workers_running: workers[i], groups_allowed: allowed[i],
        })).collect())
    }

    // ---- group geography (INTEGRATION.md "Diagnostics"): pm_group_spread / pm_config_spread by name, and the force-regroup route

    /// every live group by id text ("{:x}")
    pub fn group_spread(&self) -> Result<HashMap<String, GroupSpread>> {
        let t = self.nodes.read();           // (LOCK ORDER: nodes, the engine)
        // the ids in slot order, then the rows in the same order; another thread's call in between changes the count: ask again
        for _attempt in 0..8 {
            let (_, groups, _) = self.snapshot_groups(t.rows.len(), false)?;
            let mut rows = vec![pm_group_spread_row::default(); groups.len()];
            let mut n = 0u32;
            let rc = unsafe { pm_group_spread(self.engine, if rows.is_empty() { std::ptr::null_mut() } else { rows.as_mut_ptr() },
                                              rows.len() as u32, &mut n) };
            if rc == PM_ERANGE && n as usize != rows.len() { continue; }
            check(rc)?;
            if n as usize != rows.len() { continue; }
            let addr = |w: u32| if w == PM_NONE { String::new() } else { t.address_strings[w as usize].clone() };
            return Ok(groups.iter().zip(rows.iter()).map(|(g, r)| (format!("{:x}", g.id), GroupSpread {
                located: r.located,
                ring_hops: r.ring_hops,
                far_a: addr(r.far_a),
                far_b: addr(r.far_b),
                hop_from: addr(r.hop_from),
                diameter_km: r.diameter_km,
                ring_km: r.ring_km,
                longest_hop_km: r.longest_hop_km,
            })).collect());
        }
        Err(anyhow!("pm_engine error {PM_ESTATE}: group_spread: the group list kept changing under the report"))
    }

    /// constructor order
    pub fn configuration_spread(&self) -> Result<Vec<ConfigurationSpread>> {
        let mut rows = vec![pm_config_spread_row::default(); self.config_names.len()];
        let mut n = 0u32;
        check(unsafe { pm_config_spread(self.engine, if rows.is_empty() { std::ptr::null_mut() } else { rows.as_mut_ptr() },
                                        rows.len() as u32, &mut n) })?;
        Ok(rows.iter().take(n as usize).enumerate().map(|(c, r)| ConfigurationSpread {
            name: self.config_names[c].clone(),
            groups: r.groups,
            measured: r.measured,
            hist: r.hist,
            max_diameter_km: r.max_diameter_km,
            max_hop_km: r.max_hop_km,
            sum_diameter_m: r.sum_diameter_m,
            sum_ring_m: r.sum_ring_m,
        }).collect())
    }

    /// POST /groups/force-regroup (api/routes/groups.rs:319-380) with a selection: metric REGROUP_ALL is the route as the
    /// reference has it, REGROUP_DIAMETER / REGROUP_LONGEST_HOP dissolve the groups at or above threshold_km.  None: no
    /// configuration has this name (the route's 404).  Sends the destroyed webhooks, in get_all_groups order.
    pub fn force_regroup(&self, configuration_name: &str, metric: u32, threshold_km: f64) -> Result<Option<ForceRegroupResult>> {
        let Some(config) = self.config_names.iter().position(|n| n == configuration_name) else { return Ok(None) };
        let mut out = ForceRegroupResult::default();
        check(unsafe { pm_force_regroup(self.engine, config as u32, metric, threshold_km, &mut out.dissolved_groups,
                                        &mut out.affected_nodes) })?;
        if out.dissolved_groups != 0 { self.emit_group_webhooks()?; }                    // send_group_destroyed, mod.rs:1469-1481
        Ok(Some(out))
    }

    // ---- nearest candidates (INTEGRATION.md "Diagnostics: nearest candidates"): pm_nearest_workers by address and name

    /// address None: from the seed try_form_new_groups would take for the configuration now (NEAR_SEED).  pool: NEAR_IDLE
    /// (the next carve's candidates) or NEAR_ELIGIBLE; k in [1, NEAR_MAX_K].  Ok(None): the node table does not hold the
    /// address.  Err: no configuration has this name.
    pub fn nearest_nodes(&self, address: Option<&str>, configuration_name: &str, pool: u32, k: u32) -> Result<Option<NearestNodes>> {
        let Some(config) = self.config_names.iter().position(|n| n == configuration_name) else {
            return Err(anyhow!("nearest_nodes: no configuration is named '{configuration_name}'"));
        };
        let t = self.nodes.read();           // (LOCK ORDER: nodes, the engine)
        let mut q = pm_near_query { origin: NEAR_SEED, config: config as u32 };
        if let Some(a) = address {
            let Some(row) = Self::row_of_address_text(&t, a) else { return Ok(None) };
            q.origin = row;
        }
        let mut r = pm_near_row::default();
        let mut workers = vec![0u32; k.max(1) as usize];     // (k == 0 is the engine's to refuse)
        let mut km = vec![0f64; workers.len()];
        check(unsafe { pm_nearest_workers(self.engine, &q, 1, pool, k, &mut r, workers.as_mut_ptr(), km.as_mut_ptr()) })?;
        Ok(Some(NearestNodes {
            origin: if r.origin == PM_NONE { String::new() } else { t.address_strings[r.origin as usize].clone() },
            candidates: r.candidates,
            located: r.located,
            nodes: workers.iter().zip(km.iter()).take(r.n as usize).map(|(&w, &d)| (t.address_strings[w as usize].clone(), d)).collect(),
        }))
    }

    // ---- probing configurations (INTEGRATION.md "Diagnostics: probing configurations"): pm_probe_configs / pm_config_overlap

    /// name, sizes and requirements of every probe, packed exactly as the constructor packs the installed ones, the model rule
    /// against the node table's interned spec models.  One result per probe, in the given order.
    pub fn probe_configurations(&self, probes: &[NodeGroupConfiguration]) -> Result<Vec<ProbeResult>> {
        let mut alts: Vec<pm_gpu_alt_row> = Vec::new();
        let mut req_models: Vec<CString> = Vec::new();
        let rows = Self::pack_templates(probes, &mut alts, &mut req_models);
        let t = self.nodes.read();           // (LOCK ORDER: nodes, the engine)
        // the probes' model rule against the interned spec models: the list the installed table was last built against
        let spec: Vec<CString> = t.spec_models.iter().map(|s| CString::new(s.as_str()).unwrap()).collect();
        let spec_p: Vec<*const c_char> = spec.iter().map(|s| s.as_ptr()).collect();
        let req_p: Vec<*const c_char> = req_models.iter().map(|s| s.as_ptr()).collect();
        let words = (spec.len() + 31) / 32;
        let mut bits = vec![0u32; (req_models.len() * words).max(1)];
        check(unsafe { pm_host_build_model_table(req_p.as_ptr(), req_p.len() as u32, spec_p.as_ptr(), spec_p.len() as u32,
                                                 bits.as_mut_ptr()) })?;
        let c = self.config_names.len();
        let mut out = vec![pm_probe_row::default(); rows.len().max(1)];
        let mut overlap = vec![0u32; (rows.len() * c).max(1)];
        check(unsafe { pm_probe_configs(self.engine, rows.as_ptr(), rows.len() as u32, alts.as_ptr(), alts.len() as u32,
                                        bits.as_ptr(), req_p.len() as u32, spec_p.len() as u32, out.as_mut_ptr(),
                                        overlap.as_mut_ptr(), std::ptr::null_mut()) })?;
        Ok(probes.iter().enumerate().map(|(p, probe)| {
            let k = &out[p];
            ProbeResult {
                name: probe.name.clone(),
                why: k.why,
                eligible_meets: k.eligible_meets,
                idle_meets: k.idle_meets,
                idle_located: k.idle_located,
                idle_exclusive: k.idle_exclusive,
                groups_max: k.groups_max,
                groups_exclusive: k.groups_exclusive,
                overlap: self.config_names.iter().enumerate().map(|(i, n)| (n.clone(), overlap[p * c + i])).collect(),
            }
        }).collect())
    }

    pub fn configuration_overlap(&self) -> Result<ConfigurationOverlap> {
        let c = self.config_names.len();
        let mut idle = vec![0u32; (c * c).max(1)];
        let mut n = 0u32;
        check(unsafe { pm_config_overlap(self.engine, idle.as_mut_ptr(), (c * c) as u32, &mut n) })?;
        idle.truncate(c * c);
        Ok(ConfigurationOverlap { names: self.config_names.clone(), idle })
    }

    // ---- change feed (INTEGRATION.md "Change feed"): pm_enable_assignment_changes / pm_drain_assignment_changes by address

    /// off also clears; on = resync
    pub fn enable_change_feed(&self, on: bool) -> Result<()> {
        check(unsafe { pm_enable_assignment_changes(self.engine, on as u32) })
    }

    /// drains the feed.  Err: the engine lists a row the node table does not hold.
    pub fn changed_nodes(&self) -> Result<ChangedNodes> {
        let t = self.nodes.read();           // (LOCK ORDER: nodes, the engine)
        let mut rows: Vec<pm_change_row> = Vec::new();
        let (mut n, mut flags) = (0u32, 0u32);
        let mut rc = unsafe { pm_drain_assignment_changes(self.engine, std::ptr::null_mut(), 0, &mut n, &mut flags) };  // the size query
        while rc == PM_ERANGE {              // (a publish between two calls lengthens the list: ask again, never read short)
            rows.resize(n.max(1) as usize, pm_change_row::default());
            rc = unsafe { pm_drain_assignment_changes(self.engine, rows.as_mut_ptr(), rows.len() as u32, &mut n, &mut flags) };
        }
        check(rc)?;
        if n as usize > rows.len() { return Err(anyhow!("changed_nodes: the engine reports more rows than it was given room for")); }
        for r in &rows[..n as usize] {
            if r.worker as usize >= t.address_strings.len() {
                return Err(anyhow!("changed_nodes: the engine lists a row the node table does not hold"));
            }
        }
        Ok(ChangedNodes {
            resync: flags & CHANGES_RESYNC != 0,
            nodes: rows[..n as usize].iter().map(|r| (t.address_strings[r.worker as usize].clone(), r.what)).collect(),
        })
    }

    // ---- liveness (INTEGRATION.md "Liveness"): NodeStatusUpdater::process_nodes (status_update/mod.rs:144-372) as
    // pm_liveness_sweep over the plugin's rows; the heartbeat route's heartbeat_store.beat (routes/heartbeat.rs:54-93) as a
    // store into a column of atomics indexed by the node's row

    /// pm_liveness_enable(on = 1): the ledger starts from the rows' Healthy bit; from here on handle_status_change also
    /// writes the ledger
    pub fn enable_liveness(&self, missing_heartbeat_threshold: u32) -> Result<()> {
        let mut t = self.nodes.write();       // (LOCK ORDER: nodes, the engine)
        check(unsafe { pm_liveness_enable(self.engine, 1, missing_heartbeat_threshold) })?;
        t.liveness_on = true;
        Ok(())
    }

    /// handle_status_change's write to the ledger (the write lock is held): the discovery monitor's and the ban route's
    /// statuses leave the unhealthy counter alone, the invite's WaitingForHeartbeat clears it (node/invite.rs:168-176)
    fn liveness_note(&self, row: u32, status: &NodeStatus) -> Result<()> {
        let s = node_status_code(status);
        let mut counter = 0u32;
        if *status != NodeStatus::WaitingForHeartbeat {
            check(unsafe { pm_liveness_get(self.engine, &row, 1, std::ptr::null_mut(), &mut counter) })?;
        }
        check(unsafe { pm_liveness_set(self.engine, &row, &s, &counter, 1) })
    }

    /// no engine call: under the read lock.  An address the node table does not hold is ignored.
    pub fn beat(&self, address: &Address, now_ms: u64) {
        let t = self.nodes.read();
        if let Some(&w) = t.index.get(address) {
            if let Some(b) = t.beats.get(w as usize) { b.store(now_ms, Ordering::Relaxed); }
        }
    }

    /// one process_nodes pass: the engine sweeps with apply = 1, the rows' Healthy bits follow, and the transitions come
    /// back in row order for the host's metric clean-up and chain sync (mod.rs:314-350, :118-142).  out_of_pool: the nodes
    /// is_node_in_pool (mod.rs:380-390) is false for; empty = the cfg(test) stub.
    pub fn sweep_statuses(&self, now_ms: u64, out_of_pool: &[Address]) -> Result<Vec<(String, NodeStatus, NodeStatus)>> {
        let mut t = self.nodes.write();       // (LOCK ORDER: nodes, the engine; the rows' flags are written below)
        let w_rows = t.rows.len();
        let beats: Vec<u64> = (0..w_rows).map(|w| t.beats.get(w).map_or(0, |b| b.load(Ordering::Relaxed))).collect();
        let mut pool: Vec<u64> = Vec::new();
        if !out_of_pool.is_empty() {
            pool = vec![!0u64; (w_rows + 63) / 64];
            for a in out_of_pool {
                if let Some(&w) = t.index.get(a) { pool[(w >> 6) as usize] &= !(1u64 << (w & 63)); }
            }
        }
        let mut n = 0u32;
        // (admission on: the later of the device's beat column and this one, so beat() and admitted heartbeats both count)
        let beats_ptr = if w_rows != 0 { beats.as_ptr() } else { std::ptr::null() };
        let pool_ptr = if pool.is_empty() { std::ptr::null() } else { pool.as_ptr() };
        check(unsafe {
            if t.admission_on { pm_liveness_sweep_beats(self.engine, now_ms, beats_ptr, pool_ptr, 1, &mut n, std::ptr::null_mut()) }
            else { pm_liveness_sweep(self.engine, now_ms, beats_ptr, pool_ptr, 1, &mut n, std::ptr::null_mut()) }
        })?;
        let mut rows = vec![pm_live_row::default(); n.max(1) as usize];
        let mut got = 0u32;
        check(unsafe { pm_liveness_transitions(self.engine, rows.as_mut_ptr(), rows.len() as u32, &mut got) })?;
        if got != n { return Err(anyhow!("sweep_statuses: the list is not the sweep's")); }
        for r in &rows[..n as usize] {
            if r.worker as usize >= w_rows || r.old_status >= NS_N || r.new_status >= NS_N {
                return Err(anyhow!("sweep_statuses: the engine lists a row the node table does not hold"));
            }
        }
        let mut out = Vec::with_capacity(n as usize);
        let mut any_dead = false;
        for r in &rows[..n as usize] {
            let mut flags = t.rows[r.worker as usize].flags & !W_HEALTHY;   // (what the engine's apply gave the row)
            if r.new_status == NS_HEALTHY { flags |= W_HEALTHY; }
            t.rows[r.worker as usize].flags = flags;
            note_stamp(&mut t, r.worker, now_ms);
            any_dead = any_dead || r.new_status == NS_DEAD;
            out.push((t.address_strings[r.worker as usize].clone(), node_status_of(r.old_status), node_status_of(r.new_status)));
        }
        drop(t);
        if any_dead { self.emit_group_webhooks()?; }       // whole groups were dissolved (status_update_impl.rs:17-29)
        Ok(out)
    }

    // ---- discovery sync (INTEGRATION.md "Discovery sync"): DiscoveryMonitor::get_nodes -> sync_single_node_with_discovery
    // (discovery/monitor.rs:218-435) as pm_discovery_sync over the plugin's rows.  Needs enable_liveness.

    /// the store's ip and port of a node (start-up, add_node by another writer); unknown addresses are remembered until
    /// sync_nodes brings their row
    pub fn set_endpoint(&self, address: &Address, ip_address: &str, port: u16) {
        let mut t = self.nodes.write();
        t.ep_pending.insert(address.clone(), (ip_address.to_string(), port));
        fit_endpoints(&mut t);
    }

    pub fn endpoint_of(&self, address: &Address) -> Option<(String, u16)> {
        let t = self.nodes.read();
        let w = *t.index.get(address)? as usize;
        if w >= t.ep_ip.len() || t.ep_ip[w].is_empty() { return None; }
        Some((t.ep_ip[w].clone(), t.ep_port[w]))
    }

    pub fn last_status_change_ms(&self, address: &Address) -> u64 {
        let t = self.nodes.read();
        t.index.get(address).and_then(|&w| t.stamps.get(w as usize).copied()).unwrap_or(0)
    }

    /// one get_nodes pass, applied.  A sighting whose address has no present row is the reference's Ok(None): admitted or
    /// skipped.  ADMITTED NODES ARE RETURNED, NOT APPENDED: the caller adds them to its store and the next sync_nodes brings
    /// their rows (their endpoint is remembered from the sighting).  The store writes of location and specs are the caller's.
    pub fn sync_discovery(&self, now_ms: u64, sightings: &[DiscoverySighting], max_same_endpoint: u32) -> Result<Vec<DiscoveryOutcome>> {
        let mut guard = self.nodes.write();   // (LOCK ORDER: nodes, the engine; flags, stamps and endpoints are written below)
        let t = &mut *guard;
        let (w_rows, d_rows) = (t.rows.len(), sightings.len());
        fit_endpoints(t);
        let mut rows = vec![pm_disc_row::default(); d_rows];
        let mut pass = 0;
        loop {
            for (j, s) in sightings.iter().enumerate() {
                let r = &mut rows[j];
                *r = pm_disc_row::default();
                r.endpoint = intern_endpoint(t, &s.ip_address, s.port);
                r.flags = (if s.is_validated { DF_VALIDATED } else { 0 }) | (if s.is_provider_whitelisted { DF_WHITELISTED } else { 0 })
                    | (if s.is_active { DF_ACTIVE } else { 0 }) | (if s.balance_zero { DF_BALANCE_ZERO } else { 0 });
                r.last_updated_ms = s.last_updated_ms;
                let w = match t.index.get(&s.address) {   // get_node is Ok(None) (a tombstoned row left the store)
                    Some(&w) if t.present[w as usize] => w,
                    _ => { r.row = DISC_NEW; continue; }
                };
                r.row = w;
                // "discovery ip : STORED port" (a row whose endpoint nobody told has no stored port: the sighting's)
                let stored_port = if t.ep_ip[w as usize].is_empty() { s.port } else { t.ep_port[w as usize] };
                r.endpoint_after = intern_endpoint(t, &s.ip_address, stored_port);
                r.flags |= (if s.location_new { DF_LOCATION_NEW } else { 0 }) | (if s.specs_differ { DF_SPECS_DIFFER } else { 0 });
                r.last_change_ms = t.stamps[w as usize];
            }
            if t.ep_intern.len() <= w_rows + 2 * d_rows || pass != 0 { break; }
            // ids of endpoints nobody holds any more have piled up past what the engine accepts: intern the column afresh
            pass += 1;
            t.ep_intern.clear();
            for w in 0..w_rows {
                let (ip, port) = (t.ep_ip[w].clone(), t.ep_port[w]);
                t.ep_id[w] = if ip.is_empty() { EP_NONE } else { intern_endpoint(t, &ip, port) };
            }
        }
        // (a node that left the store is no "other node")
        let column: Vec<u32> = (0..w_rows).map(|w| if t.present[w] { t.ep_id[w] } else { EP_NONE }).collect();
        let mut res = vec![pm_disc_result::default(); d_rows.max(1)];
        check(unsafe { pm_discovery_sync(self.engine, now_ms, if w_rows != 0 { column.as_ptr() } else { std::ptr::null() },
                                         t.ep_intern.len() as u32, max_same_endpoint,
                                         if d_rows != 0 { rows.as_ptr() } else { std::ptr::null() }, d_rows as u32, 1,
                                         res.as_mut_ptr(), std::ptr::null_mut()) })?;
        for j in 0..d_rows {
            if rows[j].row != DISC_NEW && (res[j].old_status >= NS_N || res[j].final_status >= NS_N || res[j].n_updates > 3) {
                return Err(anyhow!("sync_discovery: a result that is no node status"));
            }
        }
        let mut out = Vec::with_capacity(d_rows);
        let mut any_dead = false;
        for (j, s) in sightings.iter().enumerate() {
            let r = res[j];
            let ops = r.ops as u32;
            let mut o = DiscoveryOutcome {
                kind: DiscoveryKind::Synced, address: s.address.to_string(), healthy_same_endpoint: r.healthy_same_endpoint,
                old_status: NodeStatus::Discovered, final_status: NodeStatus::Discovered, updates: Vec::new(),
                ip_rewritten: false, location_new: false, specs_rewritten: false, stamped_now: false,
            };
            if rows[j].row == DISC_NEW {
                o.kind = if ops & DO_ADMIT != 0 { DiscoveryKind::Admitted } else { DiscoveryKind::Skipped };
                if ops & DO_ADMIT != 0 { t.ep_pending.insert(s.address.clone(), (s.ip_address.clone(), s.port)); }
                out.push(o);
                continue;
            }
            let w = rows[j].row as usize;
            o.old_status = node_status_of(r.old_status);
            o.final_status = node_status_of(r.final_status);
            for u in 0..r.n_updates as usize {
                o.updates.push((node_status_of(r.upd_old[u]), node_status_of(r.upd_new[u])));
                any_dead = any_dead || r.upd_new[u] == NS_DEAD || r.upd_new[u] == NS_LOWBALANCE;
            }
            o.ip_rewritten = ops & DO_IP_REWRITE != 0;
            o.location_new = ops & DO_LOCATION != 0;
            o.specs_rewritten = ops & DO_SPECS_REWRITE != 0;
            o.stamped_now = ops & DO_STAMP_NOW != 0;
            if o.ip_rewritten && !o.specs_rewritten {   // (the specs put-back restores the old ip)
                if t.ep_ip[w].is_empty() { t.ep_port[w] = s.port; }
                t.ep_ip[w] = s.ip_address.clone();
                t.ep_id[w] = rows[j].endpoint_after;
            }
            if r.n_updates != 0 {   // (what the engine's apply gave the row)
                let mut flags = t.rows[w].flags & !W_HEALTHY;
                if r.final_status == NS_HEALTHY { flags |= W_HEALTHY; }
                t.rows[w].flags = flags;
            }
            if o.stamped_now { t.stamps[w] = now_ms; }
            out.push(o);
        }
        drop(guard);
        if any_dead { self.emit_group_webhooks()?; }       // whole groups were dissolved (status_update_impl.rs:16-29)
        Ok(out)
    }

    // ---- metrics (INTEGRATION.md "Metrics"): MetricsStore (store/domains/metrics_store.rs), the heartbeat route's metric block
    // (api/routes/heartbeat.rs:94-151) and the sync service's list (metrics/sync_service.rs:127-200) over the engine's metrics
    // ledger.  The writes queue; flush_metrics sends the queue in one pm_metrics_ingest, every read flushes first.  Address::ZERO
    // is the manual row; an address the node table does not hold is ignored.

    /// pm_metrics_enable(on = 1): an empty ledger; the queue and the interner start over
    pub fn enable_metrics(&self) -> Result<()> {
        let _t = self.nodes.read();           // (LOCK ORDER: nodes, metrics, the engine)
        let mut q = self.metrics.lock();
        check(unsafe { pm_metrics_enable(self.engine, 1) })?;
        *q = MetricsQueue::default();
        Ok(())
    }

    fn metric_row(t: &NodeTable, address: &Address) -> Option<u32> {
        if *address == Address::ZERO { return Some(MX_MANUAL); }
        t.index.get(address).copied()
    }

    /// the series of "{task_id or "manual"}:{label without ':'}" (metrics_store.rs:43-49); a new field gets the next number
    fn metric_series(q: &mut MetricsQueue, task_id: &str, label: &str) -> u32 {
        let task = if task_id.is_empty() { "manual" } else { task_id };
        let cleaned = label.replace(':', "");
        let next = q.keys.len() as u32;
        let s = *q.series.entry(format!("{task}:{cleaned}")).or_insert(next);
        if s == next { q.keys.push((task.to_string(), cleaned)); }
        s
    }

    fn queue_metrics(&self, address: &Address, kind: u32, entries: &[(String, String, f64)]) {
        let t = self.nodes.read();
        let Some(row) = Self::metric_row(&t, address) else { return };
        let mut q = self.metrics.lock();
        let first = q.entries.len() as u32;
        q.beats.push(pm_mx_beat { row, kind, first, n: entries.len() as u32 });
        for (task_id, label, value) in entries {
            // the rule is the ORIGINAL label's (metrics_store.rs:52)
            let flags = if label.contains("dashboard-progress") { MXF_MAX } else { 0 };
            let series = Self::metric_series(&mut q, task_id, label);
            q.entries.push(pm_mx_entry { series, flags, value: *value });
        }
    }

    /// heartbeat.rs:94-151 with Some(metrics): an empty list empties the row
    pub fn beat_metrics(&self, address: &Address, entries: &[(String, String, f64)]) {
        self.queue_metrics(address, MXB_REPLACE, entries)
    }

    /// metrics_store.rs:25-75
    pub fn store_metrics(&self, address: &Address, entries: &[(String, String, f64)]) {
        if entries.is_empty() { return; }     // :34-36
        self.queue_metrics(address, MXB_MERGE, entries)
    }

    /// :77-89
    pub fn store_manual_metric(&self, label: &str, value: f64) {
        self.store_metrics(&Address::ZERO, &[(String::new(), label.to_string(), value)])
    }

    /// :91-109 (the key is "{task_id}:{cleaned}" as given: no "manual" for an empty task id); a field nobody stored is in no row
    pub fn delete_metric(&self, task_id: &str, label: &str, address: &Address) {
        let t = self.nodes.read();
        let Some(row) = Self::metric_row(&t, address) else { return };
        let mut q = self.metrics.lock();
        let Some(&series) = q.series.get(&format!("{task_id}:{}", label.replace(':', ""))) else { return };
        let first = q.entries.len() as u32;
        q.beats.push(pm_mx_beat { row, kind: MXB_DELETE, first, n: 1 });
        q.entries.push(pm_mx_entry { series, flags: 0, value: 0.0 });
    }

    /// the clean-up of an Ejected / Banned node (status_update/mod.rs:314-343); the sweep empties Dead rows itself
    pub fn clear_metrics(&self, address: &Address) {
        self.queue_metrics(address, MXB_REPLACE, &[])
    }

    fn flush_metrics_locked(&self, q: &mut MetricsQueue) -> Result<()> {
        if q.beats.is_empty() { return Ok(()); }
        let n_series = (q.keys.len() as u32).max(1);
        let rc = unsafe { pm_metrics_ingest(self.engine, q.beats.as_ptr(), q.beats.len() as u32,
                                            if q.entries.is_empty() { std::ptr::null() } else { q.entries.as_ptr() },
                                            q.entries.len() as u32, n_series) };
        q.beats.clear();                      // (a refused batch is dropped, not sent again and again)
        q.entries.clear();
        check(rc)
    }

    pub fn flush_metrics(&self) -> Result<()> {
        let _t = self.nodes.read();
        let mut q = self.metrics.lock();
        self.flush_metrics_locked(&mut q)
    }

    fn metric_totals(&self) -> Result<(Vec<f64>, Vec<u32>)> {
        let mut n = 0u32;
        let rc = unsafe { pm_metrics_totals(self.engine, std::ptr::null_mut(), std::ptr::null_mut(), 0, &mut n) };
        if rc != PM_ERANGE { check(rc)?; }
        let mut sum = vec![0f64; n.max(1) as usize];
        let mut count = vec![0u32; n.max(1) as usize];
        check(unsafe { pm_metrics_totals(self.engine, sum.as_mut_ptr(), count.as_mut_ptr(), sum.len() as u32, &mut n) })?;
        sum.truncate(n as usize);
        count.truncate(n as usize);
        Ok((sum, count))
    }

    fn metric_rows(&self, t: &NodeTable, q: &MetricsQueue, rows: Option<&[u32]>) -> Result<Vec<pm_mx_row>> {
        let (ptr, n) = rows.map_or((std::ptr::null(), 0u32), |r| (r.as_ptr(), r.len() as u32));
        let mut have = 0u32;
        let rc = unsafe { pm_metrics_rows(self.engine, ptr, n, std::ptr::null_mut(), 0, &mut have) };
        if rc != PM_ERANGE { check(rc)?; }
        let mut out = vec![pm_mx_row::default(); have.max(1) as usize];
        let mut got = 0u32;
        check(unsafe { pm_metrics_rows(self.engine, ptr, n, out.as_mut_ptr(), out.len() as u32, &mut got) })?;
        if got as usize > out.len() { return Err(anyhow!("metrics: the listing grew between two calls")); }
        out.truncate(got as usize);
        for r in &out {
            if r.series as usize >= q.keys.len() || (r.row != MX_MANUAL && r.row as usize >= t.rows.len()) {
                return Err(anyhow!("metrics: the engine lists an entry the plugin does not know"));
            }
        }
        Ok(out)
    }

    /// get_aggregate_metrics_for_all_tasks (:176-202): the series' totals rolled up to label names, ascending series order
    pub fn aggregate_metrics_for_all_tasks(&self) -> Result<HashMap<String, f64>> {
        let _t = self.nodes.read();
        let mut q = self.metrics.lock();
        self.flush_metrics_locked(&mut q)?;
        let (sum, count) = self.metric_totals()?;
        let mut out: HashMap<String, f64> = HashMap::new();
        for s in 0..sum.len().min(q.keys.len()) {
            if count[s] != 0 { *out.entry(q.keys[s].1.clone()).or_insert(0.0) += sum[s]; }    // :196
        }
        Ok(out)
    }

    /// get_aggregate_metrics_for_task (:143-174)
    pub fn aggregate_metrics_for_task(&self, task_id: &str) -> Result<HashMap<String, f64>> {
        let _t = self.nodes.read();
        let mut q = self.metrics.lock();
        self.flush_metrics_locked(&mut q)?;
        let (sum, count) = self.metric_totals()?;
        let mut out: HashMap<String, f64> = HashMap::new();
        for s in 0..sum.len().min(q.keys.len()) {
            if count[s] != 0 && q.keys[s].0 == task_id { *out.entry(q.keys[s].1.clone()).or_insert(0.0) += sum[s]; }   // :166-167
        }
        Ok(out)
    }

    /// get_metrics_for_node (:111-131): task -> name -> value
    pub fn metrics_for_node(&self, address: &Address) -> Result<HashMap<String, HashMap<String, f64>>> {
        let t = self.nodes.read();
        let mut q = self.metrics.lock();
        self.flush_metrics_locked(&mut q)?;
        let mut out: HashMap<String, HashMap<String, f64>> = HashMap::new();
        let Some(row) = Self::metric_row(&t, address) else { return Ok(out) };
        for r in self.metric_rows(&t, &q, Some(&[row]))? {
            let (task, name) = &q.keys[r.series as usize];
            out.entry(task.clone()).or_default().insert(name.clone(), r.value);
        }
        Ok(out)
    }

    /// get_all_metrics (:204-240): task -> name -> address -> value
    pub fn all_metrics(&self) -> Result<HashMap<String, HashMap<String, HashMap<String, f64>>>> {
        let t = self.nodes.read();
        let mut q = self.metrics.lock();
        self.flush_metrics_locked(&mut q)?;
        let mut out: HashMap<String, HashMap<String, HashMap<String, f64>>> = HashMap::new();
        for r in self.metric_rows(&t, &q, None)? {
            let address = if r.row == MX_MANUAL { Address::ZERO.to_string() } else { t.address_strings[r.row as usize].clone() };
            let (task, name) = &q.keys[r.series as usize];
            out.entry(task.clone()).or_default().entry(name.clone()).or_default().insert(address, r.value);
        }
        Ok(out)
    }

    /// sync_metrics_from_redis' list (sync_service.rs:127-200): every entry with its task's name ("unknown" where the map has
    /// none) and its node's group id and configuration name, joined by the engine
    pub fn synced_metrics(&self, task_names: &HashMap<String, String>) -> Result<Vec<SyncedMetric>> {
        let t = self.nodes.read();
        let mut q = self.metrics.lock();
        self.flush_metrics_locked(&mut q)?;
        let mut out = Vec::new();
        for r in self.metric_rows(&t, &q, None)? {
            let (task, name) = &q.keys[r.series as usize];
            let mut m = SyncedMetric {
                address: if r.row == MX_MANUAL { Address::ZERO.to_string() } else { t.address_strings[r.row as usize].clone() },
                task_id: task.clone(),
                task_name: task_names.get(task).cloned().unwrap_or_else(|| "unknown".to_string()),   // :172-175
                label: name.clone(),
                value: r.value,
                group_id: None,
                group_config_name: None,
            };
            if r.group_id != PM_NONE as u64 {                                                        // :179-182
                let Some(cfg) = self.config_names.get(r.config as usize) else {
                    return Err(anyhow!("metrics: the engine names a configuration the plugin has not"));
                };
                m.group_id = Some(format!("{:x}", r.group_id));
                m.group_config_name = Some(cfg.clone());
            }
            out.push(m);
        }
        Ok(out)
    }

    // ---- rollout (INTEGRATION.md "Rollout"): the task fields the heartbeat route stores per node (api/routes/heartbeat.rs:54-73 ->
    // NodeStore::update_node_task, node_store.rs:339-377) over the engine's rollout ledger, and the reads that join them with the
    // standing groups.  The writes queue; flush_rollout sends the queue in one pm_rollout_ingest, every read flushes first.

    /// the 64-bit id of a reported task_id text: task_uid of a UUID (hyphenated or the 32 digits alone), else FNV-1a of the bytes.
    /// A DEVIATION: two texts whose ids collide are one id to the ledger (the reference keys by the text).
    pub fn reported_task_uid(task_id: &str) -> u64 {
        if task_id.len() == 32 || task_id.len() == 36 {
            if let Ok(u) = uuid::Uuid::parse_str(task_id) { return u.as_u64_pair().1; }
        }
        task_id.bytes().fold(0xCBF2_9CE4_8422_2325u64, |h, c| (h ^ c as u64).wrapping_mul(0x0000_0100_0000_01B3))
    }

    /// pm_rollout_enable(on = 1): empty columns; the queue and the texts start over
    pub fn enable_rollout(&self) -> Result<()> {
        let _t = self.nodes.read();           // (LOCK ORDER: nodes, tasks, rollout, the engine)
        let mut q = self.rollout.lock();
        check(unsafe { pm_rollout_enable(self.engine, 1) })?;
        *q = RolloutQueue::default();
        Ok(())
    }

    /// update_node_task's match (node_store.rs:356-373): both present set the report, anything else clears it
    pub fn report_task(&self, address: &Address, task_id: Option<&str>, task_state: Option<&str>) {
        let t = self.nodes.read();
        let Some(&row) = t.index.get(address) else { return };
        let mut q = self.rollout.lock();
        match (task_id, task_state) {
            (Some(task), Some(state)) => {
                let uid = Self::reported_task_uid(task);
                q.texts.entry(uid).or_insert_with(|| task.to_string());   // (the first text of an id stays)
                let state = CString::new(state).map(|s| unsafe { pm_host_task_state(s.as_ptr()) }).unwrap_or(TS_UNKNOWN);
                q.reports.push(pm_ro_report { worker: row, state, uid });
            }
            _ => q.reports.push(pm_ro_report { worker: row, state: TS_NONE, uid: 0 }),
        }
    }

    fn flush_rollout_locked(&self, q: &mut RolloutQueue) -> Result<()> {
        if q.reports.is_empty() { return Ok(()); }
        let rc = unsafe { pm_rollout_ingest(self.engine, q.reports.as_ptr(), q.reports.len() as u32) };
        q.reports.clear();                    // (a refused batch is dropped, not sent again and again)
        check(rc)
    }

    pub fn flush_rollout(&self) -> Result<()> {
        let _t = self.nodes.read();
        let mut q = self.rollout.lock();
        self.flush_rollout_locked(&mut q)
    }

    /// the task report; the texts of ids it no longer lists go (a listed id keeps its text also while the task list carries it: a
    /// task deleted under its reporters renders with the text they sent)
    fn rollout_task_rows(&self, tasks: &[Task], q: &mut RolloutQueue) -> Result<Vec<pm_ro_task_row>> {
        let mut have = 0u32;
        let rc = unsafe { pm_rollout_tasks(self.engine, std::ptr::null_mut(), 0, &mut have) };
        if rc != PM_ERANGE { check(rc)?; }
        let mut out = vec![pm_ro_task_row::default(); have.max(1) as usize];
        let mut got = 0u32;
        check(unsafe { pm_rollout_tasks(self.engine, out.as_mut_ptr(), out.len() as u32, &mut got) })?;
        if got as usize > out.len() { return Err(anyhow!("rollout: the task report grew between two calls")); }
        out.truncate(got as usize);
        let mut kept = HashMap::new();
        for r in &out {
            if r.task != PM_NONE && r.task as usize >= tasks.len() {
                return Err(anyhow!("rollout: the engine names a task the plugin has not"));
            }
            if let Some(text) = q.texts.remove(&r.uid) { kept.insert(r.uid, text); }
        }
        q.texts = kept;
        Ok(out)
    }

    fn rollout_text(tasks: &[Task], q: &RolloutQueue, uid: u64, task: u32) -> String {
        if let Some(t) = tasks.get(task as usize).filter(|_| task != PM_NONE) { return t.id.to_string(); }
        q.texts.get(&uid).cloned().unwrap_or_else(|| format!("{:x}", uid))
    }

    pub fn task_rollout(&self) -> Result<Vec<TaskRollout>> {
        let _t = self.nodes.read();
        let tasks = self.tasks.read();
        let mut q = self.rollout.lock();
        self.flush_rollout_locked(&mut q)?;
        let rows = self.rollout_task_rows(&tasks, &mut q)?;
        Ok(rows.into_iter().map(|r| TaskRollout {
            task_id: Self::rollout_text(&tasks, &q, r.uid, r.task),
            task_name: if r.task != PM_NONE { tasks[r.task as usize].name.clone() } else { "unknown".to_string() },
            row: r,
        }).collect())
    }

    /// nodes_per_task as the sync service sets it (sync_service.rs:243-267): only tasks with nodes, ascending by the 64-bit id
    pub fn nodes_per_task(&self) -> Result<Vec<NodesPerTask>> {
        Ok(self.task_rollout()?.into_iter().filter_map(|t| {
            let count: u32 = t.row.reporters.iter().sum();
            (count != 0).then(|| NodesPerTask { task_id: t.task_id, task_name: t.task_name, count })
        }).collect())
    }

    pub fn rollout_summary(&self) -> Result<pm_ro_summary> {
        let _t = self.nodes.read();
        let mut q = self.rollout.lock();
        self.flush_rollout_locked(&mut q)?;
        let mut out = pm_ro_summary::default();
        check(unsafe { pm_rollout_summary(self.engine, &mut out) })?;
        Ok(out)
    }

    pub fn group_rollout(&self) -> Result<Vec<GroupRollout>> {
        let _t = self.nodes.read();
        let tasks = self.tasks.read();
        let mut q = self.rollout.lock();
        self.flush_rollout_locked(&mut q)?;
        let mut have = 0u32;
        let rc = unsafe { pm_rollout_groups(self.engine, std::ptr::null_mut(), 0, &mut have) };
        if rc != PM_ERANGE { check(rc)?; }
        let mut rows = vec![pm_ro_group_row::default(); have.max(1) as usize];
        let mut got = 0u32;
        check(unsafe { pm_rollout_groups(self.engine, rows.as_mut_ptr(), rows.len() as u32, &mut got) })?;
        if got as usize > rows.len() { return Err(anyhow!("rollout: the group report grew between two calls")); }
        rows.truncate(got as usize);
        let mut out = Vec::new();
        for r in rows {
            let (Some(cfg), Some(task)) = (self.config_names.get(r.config as usize), tasks.get(r.task as usize)) else {
                return Err(anyhow!("rollout: the engine names a configuration or a task the plugin has not"));
            };
            out.push(GroupRollout { group_id: format!("{:x}", r.group_id), configuration_name: cfg.clone(),
                                    task_id: task.id.to_string(), row: r });
        }
        Ok(out)
    }

    pub fn rollout_nodes(&self, class_mask: u32) -> Result<Vec<NodeRollout>> {
        let t = self.nodes.read();
        let tasks = self.tasks.read();
        let mut q = self.rollout.lock();
        self.flush_rollout_locked(&mut q)?;
        let mut have = 0u32;
        let rc = unsafe { pm_rollout_workers(self.engine, class_mask, std::ptr::null_mut(), 0, &mut have) };
        if rc != PM_ERANGE { check(rc)?; }
        let mut rows = vec![pm_ro_worker_row::default(); have.max(1) as usize];
        let mut got = 0u32;
        check(unsafe { pm_rollout_workers(self.engine, class_mask, rows.as_mut_ptr(), rows.len() as u32, &mut got) })?;
        if got as usize > rows.len() { return Err(anyhow!("rollout: the node list grew between two calls")); }
        rows.truncate(got as usize);
        // the texts of the reported ids: the task list's where it carries the id (the first row that does), else the remembered one
        let mut first: HashMap<u64, u32> = HashMap::new();
        for (k, task) in tasks.iter().enumerate().rev() { first.insert(task_uid(task), k as u32); }
        let mut out = Vec::new();
        for r in rows {
            if r.worker as usize >= t.rows.len() { return Err(anyhow!("rollout: the engine lists a row the plugin does not know")); }
            let task_id = (r.state as u32 != TS_NONE).then(|| {
                let task = if r.uid == u64::MAX { PM_NONE } else { first.get(&r.uid).copied().unwrap_or(PM_NONE) };
                Self::rollout_text(&tasks, &q, r.uid, task)
            });
            out.push(NodeRollout { address: t.address_strings[r.worker as usize].clone(), cls: r.cls as u32, state: r.state as u32,
                                   task_id });
        }
        Ok(out)
    }

    // ---- node directory (gpu_match_directory.cpp, statement for statement): NodeStore::get_nodes' ordered listing over
    // pm_directory, for GET /nodes, the sync service's gauge, the inviter and sync_chain_with_nodes.  LOCK ORDER: nodes, the engine.

    /// one window through the size query, checked against the node table (the node lock is held)
    fn directory_locked(&self, t: &NodeTable, q: &pm_dir_query, total: &mut u32, counts: Option<&mut [u32; NS_N as usize]>)
                        -> Result<Vec<pm_dir_row>> {
        let counts = counts.map_or(std::ptr::null_mut(), |c| c.as_mut_ptr());
        let mut have = 0u32;
        let rc = unsafe { pm_directory(self.engine, q, total, counts, std::ptr::null_mut(), 0, &mut have) };
        if rc != PM_ERANGE { check(rc)?; }      // (PM_ERANGE unless the window is empty)
        if have == 0 { return Ok(Vec::new()); }
        let mut rows = vec![pm_dir_row::default(); have as usize];
        let mut got = 0u32;
        check(unsafe { pm_directory(self.engine, q, total, counts, rows.as_mut_ptr(), rows.len() as u32, &mut got) })?;
        if got as usize > rows.len() { return Err(anyhow!("directory: the window grew between two calls")); }
        rows.truncate(got as usize);
        if rows.iter().any(|r| r.worker as usize >= t.rows.len() || r.status >= NS_N) {
            return Err(anyhow!("directory: the engine lists a row the plugin does not know"));
        }
        Ok(rows)
    }

    /// GET /nodes (api/routes/nodes.rs:29-105): the window [offset, offset + limit) of the listing, without Dead unless asked
    pub fn list_nodes(&self, include_dead: bool, order: u32, offset: u32, limit: u32) -> Result<NodeListing> {
        let t = self.nodes.read();
        let all = (1u32 << NS_N) - 1;
        let q = pm_dir_query { status_mask: if include_dead { all } else { all & !(1u32 << NS_DEAD) }, membership: DIR_ANY, order,
                               offset, limit };
        let mut counts = [0u32; NS_N as usize];
        let mut out = NodeListing::default();
        let rows = self.directory_locked(&t, &q, &mut out.total, Some(&mut counts))?;
        for (s, &c) in counts.iter().enumerate() {
            if c != 0 { out.counts.insert(format!("{:?}", node_status_of(s as u8)), c); }   // (the statuses it met: nodes.rs:47-59)
        }
        for r in rows {
            let group = if r.group_slot != PM_NONE {
                let Some(cfg) = self.config_names.get(r.config as usize) else {
                    return Err(anyhow!("directory: the engine names a configuration the plugin has not"));
                };
                let created_at = self.group_created_at.lock().get(&r.group_id).copied().unwrap_or_else(chrono::Utc::now);
                Some(ListedGroup { id: format!("{:x}", r.group_id), size: r.group_size, created_at, topology_config: cfg.clone() })
            } else {
                None
            };
            out.nodes.push(ListedNode { address: t.address_strings[r.worker as usize].clone(), status: node_status_of(r.status),
                                        unhealthy_counter: r.counter, task_state: r.state as u32, group });
        }
        Ok(out)
    }

    /// the sync service's gauge (metrics/sync_service.rs:209-225): every node, lowercase names, present statuses only
    pub fn status_counts(&self) -> Result<std::collections::BTreeMap<String, u32>> {
        let t = self.nodes.read();
        let q = pm_dir_query { status_mask: (1u32 << NS_N) - 1, membership: DIR_ANY, order: DIR_BY_ROW, offset: 0, limit: 0 };
        let (mut total, mut counts) = (0u32, [0u32; NS_N as usize]);
        self.directory_locked(&t, &q, &mut total, Some(&mut counts))?;   // the counters alone
        Ok(counts.iter().enumerate().filter(|(_, &c)| c != 0)
               .map(|(s, &c)| (format!("{:?}", node_status_of(s as u8)).to_lowercase(), c)).collect())
    }

    fn nodes_of_status(&self, status: u8) -> Result<Vec<String>> {
        let t = self.nodes.read();
        let q = pm_dir_query { status_mask: 1u32 << status, membership: DIR_ANY, order: DIR_BY_ROW, offset: 0, limit: u32::MAX };
        let mut total = 0u32;
        Ok(self.directory_locked(&t, &q, &mut total, None)?.iter().map(|r| t.address_strings[r.worker as usize].clone()).collect())
    }

    /// get_uninvited_nodes (node_store.rs:247-282): the Discovered nodes, in row order
    pub fn uninvited_nodes(&self) -> Result<Vec<String>> { self.nodes_of_status(NS_DISCOVERED) }

    /// what sync_chain_with_nodes walks (status_update/mod.rs:118-142): the Dead nodes; the pool test stays the host's
    pub fn dead_nodes(&self) -> Result<Vec<String>> { self.nodes_of_status(NS_DEAD) }

    // ---- group directory (gpu_match_groupdir.cpp, statement for statement): GET /groups joined, filtered and paged over
    // pm_group_directory, the groups_count gauge, the groups that stand on a member that is not Healthy.  LOCK ORDER: nodes,
    // tasks, the engine.  get_all_groups stays as it is.

    /// one window, checked against the plugin's tables (the node and task locks are held).  The COUNTERS-ONLY query first
    /// (limit 0: one synchronisation, no sort, no row): its totals size the buffers, and ONE call behind it makes the order and
    /// the window; the engine's own size query (a null row buffer) would make the order twice.
    fn group_directory_locked(&self, t: &NodeTable, tasks: &[Task], q: &pm_gdir_query, by_config: Option<&mut [u32; 64]>)
                              -> Result<(pm_gdir_totals, Vec<pm_gdir_row>, Vec<u32>)> {
        let (by_config, cap_cfgs) = by_config.map_or((std::ptr::null_mut(), 0u32), |c| (c.as_mut_ptr(), 64u32));
        let mut totals = pm_gdir_totals::default();
        let counters = pm_gdir_query { limit: 0, ..*q };
        let (mut have, mut have_members) = (0u32, 0u32);
        check(unsafe { pm_group_directory(self.engine, &counters, &mut totals, by_config, cap_cfgs, std::ptr::null_mut(), 0, &mut have,
                                          std::ptr::null_mut(), 0, &mut have_members) })?;
        have = if q.offset >= totals.total { 0 } else { q.limit.min(totals.total - q.offset) };
        if have == 0 { return Ok((totals, Vec::new(), Vec::new())); }
        let mut rows = vec![pm_gdir_row::default(); have as usize];
        let mut members = vec![0u32; totals.members_total.max(1) as usize];
        let (mut got, mut got_members) = (0u32, 0u32);
        check(unsafe { pm_group_directory(self.engine, q, &mut totals, by_config, cap_cfgs, rows.as_mut_ptr(), rows.len() as u32,
                                          &mut got, members.as_mut_ptr(), members.len() as u32, &mut got_members) })?;
        if got as usize > rows.len() || got_members as usize > members.len() {
            return Err(anyhow!("group directory: the window grew between two calls"));
        }
        rows.truncate(got as usize);
        members.truncate(got_members as usize);
        for r in &rows {
            if r.config as usize >= self.config_names.len() {
                return Err(anyhow!("group directory: the engine names a configuration the plugin has not"));
            }
            if r.task != PM_NONE && r.task as usize >= tasks.len() {
                return Err(anyhow!("group directory: the engine names a task the plugin has not"));
            }
            if r.member_begin as u64 + r.size as u64 > members.len() as u64 {
                return Err(anyhow!("group directory: a row's members lie outside the window's"));
            }
        }
        if members.iter().any(|&m| m as usize >= t.address_strings.len()) {
            return Err(anyhow!("group directory: the engine lists a member the plugin has no address of"));
        }
        Ok((totals, rows, members))
    }

    fn listed_groups_locked(&self, t: &NodeTable, tasks: &[Task], rows: &[pm_gdir_row], members: &[u32]) -> Vec<ListedNodeGroup> {
        rows.iter().map(|r| {
            let mem = &members[r.member_begin as usize..(r.member_begin + r.size) as usize];
            // (formed, creation not reported yet: now, as make_group and list_nodes answer; the C++ twin asks its `clock`, which
            // is the same clock unless a test has set it)
            let created_at = self.group_created_at.lock().get(&r.group_id).copied().unwrap_or_else(chrono::Utc::now);
            let group = NodeGroup {
                id: format!("{:x}", r.group_id),
                nodes: mem.iter().map(|&w| t.address_strings[w as usize].clone()).collect::<BTreeSet<String>>(),
                created_at,
                configuration_name: self.config_names[r.config as usize].clone(),
            };
            let task_id = if r.task != PM_NONE { Some(tasks[r.task as usize].id.to_string()) } else { None };
            ListedNodeGroup { group, health: r.health as u32, rollout: r.rollout as u32, task_id, row: *r }
        }).collect()
    }

    /// GET /groups (api/routes/groups.rs:32-66): the window [offset, offset + limit) of the filtered groups in the chosen order
    /// (GDIR_BY_ID_TEXT is the reference's, mod.rs:1040)
    pub fn list_groups(&self, filter: &GroupFilter, order: u32, offset: u32, limit: u32) -> Result<GroupListing> {
        let t = self.nodes.read();
        let tasks = self.tasks.read();
        let q = pm_gdir_query { config_mask: filter.config_mask, holds: filter.holds, size_min: filter.size_min,
                                size_max: filter.size_max, health_mask: filter.health_mask, rollout_mask: filter.rollout_mask, order,
                                offset, limit };
        let (totals, rows, members) = self.group_directory_locked(&t, &tasks, &q, None)?;
        Ok(GroupListing { total: totals.total, totals, groups: self.listed_groups_locked(&t, &tasks, &rows, &members) })
    }

    /// the groups_count gauge (metrics/sync_service.rs:272-286): configuration name -> groups, present ones only; one
    /// counters-only query
    pub fn group_counts(&self) -> Result<std::collections::BTreeMap<String, u32>> {
        let t = self.nodes.read();
        let tasks = self.tasks.read();
        let q = pm_gdir_query { config_mask: u64::MAX, holds: GDIR_ANY, size_min: 0, size_max: u32::MAX, health_mask: (1 << GH_N) - 1,
                                rollout_mask: (1 << GR_N) - 1, order: GDIR_BY_SLOT, offset: 0, limit: 0 };
        let mut by_config = [0u32; 64];
        let (totals, _, _) = self.group_directory_locked(&t, &tasks, &q, Some(&mut by_config))?;
        if totals.n_cfgs as usize > self.config_names.len() {
            return Err(anyhow!("group directory: the engine counts a configuration the plugin has not"));
        }
        let mut out = std::collections::BTreeMap::new();
        for c in 0..totals.n_cfgs as usize {
            if by_config[c] != 0 { *out.entry(self.config_names[c].clone()).or_insert(0) += by_config[c]; }
        }
        Ok(out)
    }

    /// the groups that stand on a member that is not Healthy (health LOST or DEGRADED), in id-text order
    pub fn degraded_groups(&self) -> Result<Vec<ListedNodeGroup>> {
        let t = self.nodes.read();
        let tasks = self.tasks.read();
        let q = pm_gdir_query { config_mask: u64::MAX, holds: GDIR_ANY, size_min: 0, size_max: u32::MAX,
                                health_mask: (1 << GH_LOST) | (1 << GH_DEGRADED), rollout_mask: (1 << GR_N) - 1,
                                order: GDIR_BY_ID_TEXT, offset: 0, limit: u32::MAX };
        let (_, rows, members) = self.group_directory_locked(&t, &tasks, &q, None)?;
        Ok(self.listed_groups_locked(&t, &tasks, &rows, &members))
    }

    // ---- task directory (gpu_match_taskdir.cpp, statement for statement): GET /tasks joined, filtered and paged over
    // pm_task_directory, the counters, the tasks no standing group can run, the sync service's statistics.  LOCK ORDER: nodes,
    // tasks, the engine.

    /// one window, checked against the plugin's task list (the node and task locks are held).  The COUNTERS-ONLY query first
    /// (limit 0: no sort, no row): its total sizes the buffer, and ONE call behind it makes the order and the window.
    fn task_directory_locked(&self, tasks: &[Task], q: &pm_tdir_query, by_config: Option<&mut [u32; 64]>)
                             -> Result<(pm_tdir_totals, Vec<pm_tdir_row>)> {
        let (by_config, cap_cfgs) = by_config.map_or((std::ptr::null_mut(), 0u32), |c| (c.as_mut_ptr(), 64u32));
        let mut totals = pm_tdir_totals::default();
        let counters = pm_tdir_query { limit: 0, ..*q };
        let mut have = 0u32;
        check(unsafe { pm_task_directory(self.engine, &counters, &mut totals, by_config, cap_cfgs, std::ptr::null_mut(), 0, &mut have) })?;
        have = if q.offset >= totals.total { 0 } else { q.limit.min(totals.total - q.offset) };
        if have == 0 { return Ok((totals, Vec::new())); }
        let mut rows = vec![pm_tdir_row::default(); have as usize];
        let mut got = 0u32;
        check(unsafe { pm_task_directory(self.engine, q, &mut totals, by_config, cap_cfgs, rows.as_mut_ptr(), rows.len() as u32, &mut got) })?;
        if got as usize > rows.len() { return Err(anyhow!("task directory: the window grew between two calls")); }
        rows.truncate(got as usize);
        if rows.iter().any(|r| r.task as usize >= tasks.len()) {
            return Err(anyhow!("task directory: the engine names a task the plugin has not"));
        }
        Ok((totals, rows))
    }

    fn listed_tasks_locked(&self, tasks: &[Task], rows: &[pm_tdir_row]) -> Vec<ListedTask> {
        rows.iter().map(|r| {
            let t = &tasks[r.task as usize];
            ListedTask { id: t.id.to_string(), name: t.name.clone(), serve: r.serve as u32, rollout: r.rollout as u32, row: *r }
        }).collect()
    }

    /// GET /tasks (api/routes/task.rs:20-39): the window [offset, offset + limit) of the filtered tasks in the chosen order
    /// (TDIR_BY_LIST is the reference's, task_store.rs:57-82)
    pub fn list_tasks(&self, filter: &TaskFilter, order: u32, offset: u32, limit: u32) -> Result<TaskListing> {
        let _t = self.nodes.read();
        let tasks = self.tasks.read();
        let q = pm_tdir_query { config_mask: filter.config_mask, serve_mask: filter.serve_mask, rollout_mask: filter.rollout_mask,
                                workers_min: filter.workers_min, workers_max: filter.workers_max, order, offset, limit, _pad: 0 };
        let (totals, rows) = self.task_directory_locked(&tasks, &q, None)?;
        Ok(TaskListing { total: totals.total, totals, tasks: self.listed_tasks_locked(&tasks, &rows) })
    }

    /// the task table's counters: one counters-only query
    pub fn task_counts(&self) -> Result<TaskCounts> {
        let _t = self.nodes.read();
        let tasks = self.tasks.read();
        let q = pm_tdir_query { config_mask: u64::MAX, serve_mask: (1 << TKS_N) - 1, rollout_mask: (1 << TKR_N) - 1, workers_min: 0,
                                workers_max: u32::MAX, order: TDIR_BY_LIST, offset: 0, limit: 0, _pad: 0 };
        let mut by_config = [0u32; 64];
        let (totals, _) = self.task_directory_locked(&tasks, &q, Some(&mut by_config))?;
        if totals.n_cfgs as usize > self.config_names.len() {
            return Err(anyhow!("task directory: the engine counts a configuration the plugin has not"));
        }
        let mut out = TaskCounts { totals, ..Default::default() };
        for c in 0..totals.n_cfgs as usize {
            if by_config[c] != 0 { *out.by_config.entry(self.config_names[c].clone()).or_insert(0) += by_config[c]; }
        }
        Ok(out)
    }

    /// the tasks no standing group can run (serving class STARVED), in list order
    pub fn starved_tasks(&self) -> Result<Vec<ListedTask>> {
        let _t = self.nodes.read();
        let tasks = self.tasks.read();
        let q = pm_tdir_query { config_mask: u64::MAX, serve_mask: 1 << TKS_STARVED, rollout_mask: (1 << TKR_N) - 1, workers_min: 0,
                                workers_max: u32::MAX, order: TDIR_BY_LIST, offset: 0, limit: u32::MAX, _pad: 0 };
        let (_, rows) = self.task_directory_locked(&tasks, &q, None)?;
        Ok(self.listed_tasks_locked(&tasks, &rows))
    }

    /// what sync_orchestrator_statistics sets: counters-only queries of the three directories and the rollout task table, one
    /// after the other (each under the locks it needs: not one snapshot); needs enable_liveness and enable_rollout
    pub fn orchestrator_statistics(&self) -> Result<OrchestratorStatistics> {
        Ok(OrchestratorStatistics {
            nodes_by_status: self.status_counts()?,
            tasks_count: self.task_counts()?.totals.tasks,
            nodes_per_task: self.nodes_per_task()?,
            groups_count: self.group_counts()?,
        })
    }

    /// the ledger's rows as stored (what the tests look at)
    pub fn reported_tasks(&self, rows: &[u32]) -> Result<(Vec<u64>, Vec<u8>)> {
        let mut uid = vec![0u64; rows.len()];
        let mut state = vec![0u8; rows.len()];
        check(unsafe { pm_rollout_get(self.engine, rows.as_ptr(), rows.len() as u32, uid.as_mut_ptr(), state.as_mut_ptr()) })?;
        Ok((uid, state))
    }

    /// StatusUpdatePlugin::handle_status_change (status_update_impl.rs:8-39).
    pub(crate) fn handle_status_change(&self, node: &OrchestratorNode) -> Result<()> {
        let mut t = self.nodes.write();
        let Some(&w) = t.index.get(&node.address) else { return Ok(()) };
        let mut flags = t.rows[w as usize].flags & !W_HEALTHY;
        if node.status == NodeStatus::Healthy { flags |= W_HEALTHY; }
        t.rows[w as usize].flags = flags;
        let dead = matches!(node.status, NodeStatus::Dead | NodeStatus::LowBalance) as u32;
        check(unsafe { pm_on_worker_status(self.engine, w, flags, dead) })?;
        if t.liveness_on { self.liveness_note(w, &node.status)?; }   // (the ledger learns what the host has set)
        note_stamp(&mut t, w, chrono::Utc::now().timestamp_millis() as u64);   // (update_node_status stamps: node_store.rs:284-305)
        drop(t);
        if dead != 0 { self.emit_group_webhooks()?; }      // the whole group was dissolved (status_update_impl.rs:17-29)
        Ok(())
    }
}

/// last_status_change of a row (write lock): what sync_discovery hands the engine as the snapshot's stamp
fn note_stamp(t: &mut NodeTable, row: u32, ms: u64) {
    if t.stamps.len() <= row as usize { t.stamps.resize(t.rows.len().max(row as usize + 1), 0); }
    t.stamps[row as usize] = ms;
}

fn intern_endpoint(t: &mut NodeTable, ip: &str, port: u16) -> u32 {
    let next = t.ep_intern.len() as u32;
    *t.ep_intern.entry(format!("{ip}:{port}")).or_insert(next)
}

/// the column covers every row; the endpoints remembered for addresses that have a row by now move into it
fn fit_endpoints(t: &mut NodeTable) {
    let w_rows = t.rows.len();
    if t.ep_ip.len() < w_rows {
        t.ep_ip.resize(w_rows, String::new());
        t.ep_port.resize(w_rows, 0);
        t.ep_id.resize(w_rows, EP_NONE);
    }
    if t.stamps.len() < w_rows { t.stamps.resize(w_rows, 0); }
    let arrived: Vec<Address> = t.ep_pending.keys().filter(|a| t.index.contains_key(*a)).cloned().collect();
    for a in arrived {
        let (ip, port) = t.ep_pending.remove(&a).unwrap();
        let w = t.index[&a] as usize;
        t.ep_id[w] = intern_endpoint(t, &ip, port);
        t.ep_ip[w] = ip;
        t.ep_port[w] = port;
    }
}

impl Drop for GpuMatchPlugin {
    fn drop(&mut self) { unsafe { pm_engine_destroy(self.engine) } }
}
