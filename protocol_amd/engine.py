"""ctypes binding of include/pm_engine.h (libpm_engine.so).

This is plumbing for tests and bench.py: every call goes straight through the C ABI.  Loading fails
loudly if the library has not been built, and Engine() fails with PM_ENODEV when no MI355X is
visible — there is no CPU fallback in the product path.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import build as _build

PM_NONE = 0xFFFFFFFF
PM_MAX_CONFIGS = 64
PM_OK, PM_EINVAL, PM_ENODEV, PM_ENOMEM, PM_ESTATE, PM_ERANGE, PM_EPARSE, PM_EPANIC = 0, -1, -2, -3, -4, -5, -6, -7
CHOOSE_FIRST, CHOOSE_SEEDED = 0, 1

# worker flag bits
(W_HAS_SPECS, W_HAS_GPU, W_GPU_COUNT, W_GPU_MEM, W_GPU_MODEL, W_HAS_CPU, W_CPU_CORES, W_RAM, W_STORAGE,
 W_HEALTHY, W_HAS_P2P, W_HAS_LOC) = (1 << i for i in range(12))
R_HAS_REQ, R_CPU, R_CPU_CORES, R_RAM, R_STORAGE = (1 << i for i in range(5))
G_COUNT, G_MODEL, G_MEM, G_MEM_MIN, G_MEM_MAX, G_TOT_MIN, G_TOT_MAX = (1 << i for i in range(7))

config_row_dt = np.dtype([("flags", "<u4"), ("cpu_cores", "<u4"), ("ram_mb", "<u4"), ("storage_gb", "<u4"),
                          ("alt_begin", "<u4"), ("alt_count", "<u4"), ("min_group_size", "<u4"),
                          ("max_group_size", "<u4")], align=True)
alt_row_dt = np.dtype([("flags", "<u4"), ("count", "<u4"), ("memory_mb", "<u4"), ("memory_mb_min", "<u4"),
                       ("memory_mb_max", "<u4"), ("total_memory_min", "<u4"), ("total_memory_max", "<u4"),
                       ("model_row", "<u4")], align=True)
group_dt = np.dtype([("id", "<u8"), ("config", "<u4"), ("n_members", "<u4"), ("member_begin", "<u4"),
                     ("task", "<u4")], align=True)
GROUP_EVENT = np.dtype([("group_id", "<u8"), ("kind", "<u4"), ("config", "<u4"), ("member_begin", "<u4"),
                        ("n_members", "<u4")])   # pm_group_event
GROUP_CREATED, GROUP_DESTROYED = 1, 2
# pm_config_report_row (include/pm_engine.h)
config_report_dt = np.dtype([("enabled", "<u4"), ("eligible_meets", "<u4"), ("idle_meets", "<u4"), ("why", "<u4", (10,)),
                             ("groups", "<u4"), ("members", "<u4"), ("groups_without_task", "<u4"), ("tasks_allowing", "<u4")])
# reason codes (PM_WHY_*, first failing clause of ComputeSpecs::meets) and worker states (PM_WS_*)
WHY_NAMES = ["ok", "no_specs", "cpu", "ram", "storage", "gpu_none", "gpu_count", "gpu_model", "gpu_mem", "gpu_total"]
WS_IDLE, WS_IN_GROUP, WS_UNHEALTHY, WS_NO_P2P = 0, 1, 2, 3
# pm_group_spread_row / pm_config_spread_row (include/pm_engine.h): group geography
group_spread_dt = np.dtype([("located", "<u4"), ("ring_hops", "<u4"), ("far_a", "<u4"), ("far_b", "<u4"), ("hop_from", "<u4"),
                            ("_pad", "<u4"), ("diameter_km", "<f8"), ("ring_km", "<f8"), ("longest_hop_km", "<f8")])
SPREAD_BUCKETS = 5
SPREAD_EDGES_KM = (10.0, 100.0, 1000.0, 5000.0)  # PM_SPREAD_EDGES_KM
config_spread_dt = np.dtype([("groups", "<u4"), ("measured", "<u4"), ("hist", "<u4", (SPREAD_BUCKETS,)), ("_pad", "<u4"),
                             ("max_diameter_km", "<f8"), ("max_hop_km", "<f8"), ("sum_diameter_m", "<u8"),
                             ("sum_ring_m", "<u8")])
assert group_spread_dt.itemsize == 48 and config_spread_dt.itemsize == 64
REGROUP_ALL, REGROUP_DIAMETER, REGROUP_LONGEST_HOP = 0, 1, 2
# pm_near_query / pm_near_row (include/pm_engine.h): nearest candidates
near_query_dt = np.dtype([("origin", "<u4"), ("config", "<u4")])
near_row_dt = np.dtype([("origin", "<u4"), ("n", "<u4"), ("candidates", "<u4"), ("located", "<u4")])
NEAR_IDLE, NEAR_ELIGIBLE = 0, 1
NEAR_SEED = 0xFFFFFFFE
NEAR_MAX_K, NEAR_MAX_QUERIES = 256, 65535
# pm_probe_row (include/pm_engine.h): probes against the live swarm
probe_row_dt = np.dtype([("why", "<u4", (10,)), ("eligible_meets", "<u4"), ("idle_meets", "<u4"), ("idle_located", "<u4"),
                         ("idle_exclusive", "<u4"), ("groups_max", "<u4"), ("groups_exclusive", "<u4")])
assert probe_row_dt.itemsize == 64
# pm_change_row (include/pm_engine.h): assignment change feed
change_row_dt = np.dtype([("worker", "<u4"), ("what", "<u4")])
CHG_GROUP, CHG_RING, CHG_TASK = 1, 2, 4
CHANGES_RESYNC = 1
# pm_live_row, PM_NS_* (include/pm_engine.h): liveness
live_row_dt = np.dtype([("worker", "<u4"), ("old_status", "u1"), ("new_status", "u1"), ("_pad", "<u2"), ("counter", "<u4")])
assert live_row_dt.itemsize == 12
NS_DISCOVERED, NS_WAITING, NS_HEALTHY, NS_UNHEALTHY, NS_DEAD, NS_EJECTED, NS_BANNED, NS_LOWBALANCE, NS_N = range(9)
LIVE_TTL_MS, LIVE_GIVE_UP = 90000, 360
# pm_disc_row, pm_disc_result, PM_DF_*, PM_DO_* (include/pm_engine.h): discovery sync
disc_row_dt = np.dtype([("row", "<u4"), ("endpoint", "<u4"), ("endpoint_after", "<u4"), ("flags", "<u4"),
                        ("last_change_ms", "<u8"), ("last_updated_ms", "<u8")])
disc_result_dt = np.dtype([("healthy_same_endpoint", "<u4"), ("old_status", "u1"), ("final_status", "u1"), ("n_updates", "u1"),
                           ("ops", "u1"), ("upd_old", "u1", (3,)), ("upd_new", "u1", (3,)), ("_pad", "<u2")])
assert disc_row_dt.itemsize == 32 and disc_result_dt.itemsize == 16
DISC_NEW, EP_NONE, DISC_GRACE_MS = 0xFFFFFFFF, 0xFFFFFFFF, 300000
DF_VALIDATED, DF_WHITELISTED, DF_ACTIVE, DF_LOCATION_NEW, DF_SPECS_DIFFER, DF_BALANCE_ZERO = 1, 2, 4, 8, 16, 32
DO_ADMIT, DO_SKIP, DO_IP_REWRITE, DO_LOCATION, DO_SPECS_REWRITE, DO_STAMP_NOW = 1, 2, 4, 8, 16, 32
# pm_mx_beat, pm_mx_entry, pm_mx_row, PM_MX* (include/pm_engine.h): metrics ledger
mx_beat_dt = np.dtype([("row", "<u4"), ("kind", "<u4"), ("first", "<u4"), ("n", "<u4")])
mx_entry_dt = np.dtype([("series", "<u4"), ("flags", "<u4"), ("value", "<f8")])
mx_row_dt = np.dtype([("row", "<u4"), ("series", "<u4"), ("value", "<f8"), ("group_id", "<u8"), ("config", "<u4"), ("_pad", "<u4")])
assert mx_beat_dt.itemsize == 16 and mx_entry_dt.itemsize == 16 and mx_row_dt.itemsize == 32
MX_MANUAL, MX_ROW_MAX = 0xFFFFFFFF, 1024
# pm_ro_* and PM_TS_* / PM_RO_* (include/pm_engine.h): rollout ledger
ro_report_dt = np.dtype([("worker", "<u4"), ("state", "<u4"), ("uid", "<u8")])
ro_summary_dt = np.dtype([("by_class", "<u4", (6,)), ("by_state", "<u4", (9,)), ("groups_with_task", "<u4"),
                          ("groups_converged", "<u4"), ("distinct_uids", "<u4")])
ro_task_row_dt = np.dtype([("uid", "<u8"), ("task", "<u4"), ("groups", "<u4"), ("groups_converged", "<u4"), ("assigned", "<u4"),
                           ("converged", "<u4"), ("reporters", "<u4", (8,)), ("_pad", "<u4")])
ro_group_row_dt = np.dtype([("group_id", "<u8"), ("slot", "<u4"), ("config", "<u4"), ("task", "<u4"), ("size", "<u4"),
                            ("same", "<u4", (8,)), ("other", "<u4"), ("silent", "<u4")])
ro_worker_row_dt = np.dtype([("worker", "<u4"), ("group_slot", "<u4"), ("uid", "<u8"), ("cls", "u1"), ("state", "u1"),
                             ("_pad", "<u2"), ("_pad2", "<u4")])
assert (ro_report_dt.itemsize, ro_summary_dt.itemsize, ro_task_row_dt.itemsize, ro_group_row_dt.itemsize,
        ro_worker_row_dt.itemsize) == (16, 72, 64, 64, 24)
# pm_dir_query, pm_dir_row, PM_DIR_*, PM_DC_* (include/pm_engine.h): node directory
dir_query_dt = np.dtype([("status_mask", "<u4"), ("membership", "<u4"), ("order", "<u4"), ("offset", "<u4"), ("limit", "<u4")])
dir_row_dt = np.dtype([("worker", "<u4"), ("status", "u1"), ("cls", "u1"), ("state", "u1"), ("_pad", "u1"), ("counter", "<u4"),
                       ("group_slot", "<u4"), ("group_id", "<u8"), ("group_size", "<u4"), ("config", "<u4"), ("task", "<u4"),
                       ("_pad2", "<u4"), ("uid", "<u8")])
assert dir_query_dt.itemsize == 20 and dir_row_dt.itemsize == 48
DIR_ANY, DIR_GROUPED, DIR_UNGROUPED = 0, 1, 2
DIR_BY_ROW, DIR_BY_ADDRESS = 0, 1
DC_HEALTHY, DC_DISCOVERED, DC_OTHER, DC_DEAD, DC_N = 0, 1, 2, 3, 4
# pm_gdir_query, pm_gdir_totals, pm_gdir_row, PM_GDIR_*, PM_GH_*, PM_GR_* (include/pm_engine.h): group directory
gdir_query_dt = np.dtype([("config_mask", "<u8"), ("holds", "<u4"), ("size_min", "<u4"), ("size_max", "<u4"), ("health_mask", "<u4"),
                          ("rollout_mask", "<u4"), ("order", "<u4"), ("offset", "<u4"), ("limit", "<u4")])
gdir_totals_dt = np.dtype([("total", "<u4"), ("members_total", "<u4"), ("by_health", "<u4", (3,)), ("by_rollout", "<u4", (3,)),
                           ("n_cfgs", "<u4")])
gdir_row_dt = np.dtype([("group_id", "<u8"), ("slot", "<u4"), ("config", "<u4"), ("size", "<u4"), ("task", "<u4"),
                        ("member_begin", "<u4"), ("health", "u1"), ("rollout", "u1"), ("_pad", "<u2"), ("by_status", "<u4", (8,)),
                        ("converged", "<u4"), ("behind", "<u4"), ("other", "<u4"), ("silent", "<u4")])
assert (gdir_query_dt.itemsize, gdir_totals_dt.itemsize, gdir_row_dt.itemsize) == (40, 36, 80)
GDIR_ANY, GDIR_WITH_TASK, GDIR_WITHOUT_TASK = 0, 1, 2
GDIR_BY_SLOT, GDIR_BY_ID_TEXT, GDIR_BY_SIZE_DESC = 0, 1, 2
GH_LOST, GH_DEGRADED, GH_SOUND, GH_N, GH_NONE = 0, 1, 2, 3, 255
GR_NO_TASK, GR_CONVERGED, GR_ROLLING, GR_N, GR_NONE = 0, 1, 2, 3, 255
# pm_tdir_query, pm_tdir_totals, pm_tdir_row, PM_TDIR_*, PM_TKS_*, PM_TKR_* (include/pm_engine.h): task directory
tdir_query_dt = np.dtype([("config_mask", "<u8"), ("serve_mask", "<u4"), ("rollout_mask", "<u4"), ("workers_min", "<u4"),
                          ("workers_max", "<u4"), ("order", "<u4"), ("offset", "<u4"), ("limit", "<u4"), ("_pad", "<u4")])
tdir_totals_dt = np.dtype([("tasks", "<u4"), ("total", "<u4"), ("by_serve", "<u4", (3,)), ("by_rollout", "<u4", (3,)),
                           ("unrestricted", "<u4"), ("workers_running", "<u4"), ("reporters", "<u4"), ("orphan_uids", "<u4"),
                           ("orphan_reporters", "<u4"), ("n_cfgs", "<u4")])
tdir_row_dt = np.dtype([("uid", "<u8"), ("created_at", "<i8"), ("topo_mask", "<u8"), ("task", "<u4"), ("groups_allowed", "<u4"),
                        ("groups_running", "<u4"), ("workers_running", "<u4"), ("groups_converged", "<u4"), ("converged", "<u4"),
                        ("reporters", "<u4", (8,)), ("serve", "u1"), ("rollout", "u1"), ("_pad", "<u2"), ("_pad2", "<u4")])
assert (tdir_query_dt.itemsize, tdir_totals_dt.itemsize, tdir_row_dt.itemsize) == (40, 56, 88)
TDIR_BY_LIST, TDIR_BY_OLDEST, TDIR_BY_WORKERS_DESC, TDIR_BY_REPORTERS_DESC = 0, 1, 2, 3
TKS_RUNNING, TKS_WAITING, TKS_STARVED, TKS_N = 0, 1, 2, 3
TKR_UNHELD, TKR_CONVERGED, TKR_ROLLING, TKR_N, TKR_NONE = 0, 1, 2, 3, 255
TS_NAMES = ("PENDING", "PULLING", "RUNNING", "COMPLETED", "FAILED", "PAUSED", "RESTARTING", "UNKNOWN")
TS_RUNNING, TS_UNKNOWN, TS_N, TS_NONE = 2, 7, 8, 255
RO_IDLE, RO_STRAY, RO_SILENT, RO_OTHER, RO_BEHIND, RO_CONVERGED, RO_N = 0, 1, 2, 3, 4, 5, 6
RO_CHUNK = 1024    # PM_RO_CHUNK (csrc/pm_device.h): the keys of one radix chunk of the rollout ledger's id sort
MX_CHUNK = 1024    # PM_MX_CHUNK (csrc/pm_device.h): the entries of one radix chunk of pm_metrics_totals
# neighbour rows (csrc/pm_device.h, csrc/pm_propose.inc; tests/test_host_helpers.py holds each to the source): the flags word of
# near_row_finish, the two geometries rows run at (slot bits, certificate band, window), the regimes of near_row_bulk4_body
ROW_SAFE, ROW_TAIL_CLEAR, ROW_CLEAN, ROW_TAIL_OK, ROW_COMPLETE = 1 << 27, 1 << 28, 1 << 29, 1 << 30, 1 << 31
PROP_KMAX = 63
A_MAX_SAFE = 1.0 - 1.0 / 1048576.0
ROW_SLOT_BITS, ROW_SLOT_BITS_BIG = 13, 18
TIE_BAND, TIE_BAND_BIG = 2.0 ** -36, 2.0 ** -31
WINDOW_ULPS, WINDOW_ULPS_BIG = 1 << 20, 1 << 25
NET_SERIAL_MAX, NET_PACK_KEYS = 16, 128
# the first batch's snapshot (include/pm_engine_debug.h, PM_FB_*): the words of its head ("" = unused), its parts in order
PROP_ROW, PROP_SLOTS = 96, 64      # PM_PROP_ROW, PM_PROP_SLOTS: a row's u64 words, the word its 32-bit half begins at
FB_HEAD = ("planned", "ci0", "total_available", "valid", "none", "ci", "n_list", "prop_k", "prop_limit", "n_seeds", "cell_g",
           "n_eligible", "index_g", "n_indexed", "prune_fallbacks", "pruned_batches", "n_props", "prop_keys_lo", "prop_keys_hi",
           "scan_ticket", "prune_mode", "", "", "")
FB_PARTS = (("head", "<u4"), ("order", "<u4"), ("c_site", "<u4"), ("c_ux", "<f8"), ("c_uy", "<f8"), ("c_uz", "<f8"), ("c_lat", "<f8"),
            ("c_lon", "<f8"), ("c_cos", "<f8"), ("c_compat", "<u8"), ("loc_g", "<u8"), ("alive_snap", "<u8"), ("slot_wid", "<u4"),
            ("slot_pos", "<u4"), ("cc_site", "<u4"), ("slot_alive", "<u8"), ("slot_loc", "<u8"), ("seed_map", "<u8"),
            ("seed_prefix", "<u4"), ("seed_slots", "<u4"), ("prop", "<u8"), ("cell_start", "<u4"), ("cell_cnt", "<u4"),
            ("pos_cell", "<u4"), ("cs_of_pos", "<u4"), ("cs_slot", "<u4"), ("cs_site", "<u4"), ("cs_ux", "<f8"), ("cs_uy", "<f8"),
            ("cs_uz", "<f8"))
MXB_REPLACE, MXB_MERGE, MXB_DELETE = 0, 1, 2
MXF_MAX = 1
assignment_dt = np.dtype([("task", "<u4"), ("group_slot", "<u4"), ("group_index", "<u4"), ("group_size", "<u4"),
                          ("next_worker", "<u4"), ("group_id", "<u8")], align=True)
assert config_row_dt.itemsize == 32 and alt_row_dt.itemsize == 32 and assignment_dt.itemsize == 32


class WorkerSoa(C.Structure):
    _fields_ = [("n", C.c_uint32)] + [(k, C.c_void_p) for k in
                                      ("flags", "gpu_count", "gpu_mem_mb", "gpu_model_class", "cpu_cores", "ram_mb",
                                       "storage_gb", "price", "addr_rank", "lat", "lon")]


class TaskSoa(C.Structure):
    _fields_ = [("n", C.c_uint32), ("topo_mask", C.c_void_p), ("created_at", C.c_void_p), ("uid", C.c_void_p)]


class EngineConfig(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("proximity_enabled", C.c_uint32),
                ("switching_enabled", C.c_uint32), ("prefer_larger_groups", C.c_uint32), ("chooser", C.c_uint32),
                ("chooser_seed", C.c_uint64), ("group_id_seed", C.c_uint64), ("debug_uncertain_every", C.c_uint32),
                ("sweep_variant", C.c_uint32), ("carve_variant", C.c_uint32), ("time_proposer", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [("ms_compat", C.c_float), ("ms_carve", C.c_float), ("ms_merge", C.c_float), ("ms_sweep", C.c_float),
                ("ms_publish", C.c_float), ("ms_total", C.c_float), ("ms_compat_kernel", C.c_float),
                ("ms_carve_kernel", C.c_float), ("ms_sweep_kernel", C.c_float), ("n_groups", C.c_uint32),
                ("n_formed", C.c_uint32), ("n_merged", C.c_uint32), ("carve_steps", C.c_uint32),
                ("carve_fast_steps", C.c_uint32),
                ("host_resolved_steps", C.c_uint32), ("carve_launches", C.c_uint32), ("pair_evals", C.c_uint64),
                ("carve_cand_sum", C.c_uint64), ("ms_propose_kernel", C.c_float), ("proposals", C.c_uint32),
                ("propose_keys", C.c_uint64)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class GroupVars(C.Structure):
    _fields_ = [("group_index", C.c_uint32), ("group_size", C.c_uint32), ("next_p2p_address", C.c_char_p),
                ("group_id", C.c_char_p), ("total_upload_count", C.c_char_p)]


class DistXfer(C.Structure):
    """pm_dist_xfer: device pointers + size of one all-gather (recv = [world][bytes_per_rank])."""
    _fields_ = [("send_ptr", C.c_uint64), ("recv_ptr", C.c_uint64), ("bytes_per_rank", C.c_uint64)]


class Assignment(C.Structure):
    _fields_ = [("task", C.c_uint32), ("group_slot", C.c_uint32), ("group_index", C.c_uint32),
                ("group_size", C.c_uint32), ("next_worker", C.c_uint32), ("group_id", C.c_uint64)]


# every symbol include/pm_engine.h declares (tests check the library exports all of them)
EXPORTS = [
    "pm_engine_config_default", "pm_engine_create", "pm_engine_destroy", "pm_last_error", "pm_set_configs",
    "pm_set_model_table", "pm_set_enabled_mask", "pm_upload_workers", "pm_update_workers", "pm_upload_tasks",
    "pm_on_worker_status", "pm_on_worker_status_many", "pm_enable_group_events", "pm_drain_group_events",
    "pm_dissolve_group", "pm_reset_groups", "pm_compat_masks", "pm_form_groups",
    "pm_merge_solo_groups", "pm_get_groups", "pm_match", "pm_match_per_task", "pm_newest_task", "pm_tick",
    "pm_last_stats", "pm_lookup_task_for_worker", "pm_device_task_column", "pm_host_parse_requirements", "pm_host_model_matches",
    "pm_host_build_model_table", "pm_host_config_order", "pm_host_group_vars", "pm_host_volume_vars",
    "pm_host_upload_name_vars", "pm_host_last_file_idx", "pm_abi_version",
    "pm_append_workers", "pm_set_addr_ranks", "pm_tasks_insert_front", "pm_tasks_insert_front_ex", "pm_tasks_delete", "pm_set_stream", "pm_set_carve_workgroups", "pm_tick_many", "pm_dist_configure", "pm_dist_tick_begin", "pm_dist_carve_wait",
    "pm_dist_match_begin", "pm_dist_tick_end", "pm_match_per_task_device",
    "pm_dissolve_group_by_id", "pm_get_group_by_id", "pm_get_group_of_worker", "pm_host_to_lowercase",
    "pm_adopt_groups", "pm_group_id_state",
    "pm_explain_workers", "pm_config_report", "pm_task_report",
    "pm_group_spread", "pm_config_spread", "pm_force_regroup",
    "pm_nearest_workers",
    "pm_probe_configs", "pm_config_overlap",
    "pm_enable_assignment_changes", "pm_drain_assignment_changes",
    "pm_liveness_enable", "pm_liveness_set", "pm_liveness_get", "pm_liveness_sweep", "pm_liveness_transitions",
    "pm_discovery_sync",
    "pm_metrics_enable", "pm_metrics_ingest", "pm_metrics_totals", "pm_metrics_rows",
    "pm_rollout_enable", "pm_rollout_ingest", "pm_rollout_get", "pm_rollout_summary", "pm_rollout_tasks", "pm_rollout_groups",
    "pm_rollout_workers", "pm_host_task_state",
    "pm_directory",
    "pm_group_directory",
    "pm_task_directory",
    "pm_addresses_enable", "pm_addresses_set", "pm_addresses_rank", "pm_addresses_text", "pm_invite_digests",
    "pm_ecrecover_many", "pm_verify_requests", "pm_host_ecrecover",
    "pm_admission_enable", "pm_admit_requests", "pm_admission_rate_get", "pm_admission_rate_set", "pm_admission_nonces",
    "pm_beats_get", "pm_beats_set", "pm_liveness_sweep_beats",
]
# ... and the declared names that carry a digit, which the header check's name pattern (letters and '_') does not take in
EXPORTS_NUMBERED = ["pm_keccak256_many", "pm_host_keccak256", "pm_host_eip55"]

_lib = None


class EngineError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"pm_engine error {code}: {msg}")
        self.code = code


def lib() -> C.CDLL:
    """Load libpm_engine.so (building it in-tree first if the sources are newer)."""
    global _lib
    if _lib is None:
        path = _build.LIB_PATH
        if _build.needs_build():
            path = _build.build()
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: run `python -m protocol_amd.build` (needs hipcc)")
        L = C.CDLL(path)
        vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int32
        L.pm_last_error.restype = C.c_char_p
        L.pm_abi_version.restype = u32
        L.pm_engine_config_default.argtypes = [C.POINTER(EngineConfig)]
        L.pm_engine_create.argtypes = [C.POINTER(EngineConfig), C.POINTER(vp)]
        L.pm_engine_destroy.argtypes = [vp]
        L.pm_engine_destroy.restype = None
        L.pm_set_configs.argtypes = [vp, vp, u32, vp, u32]
        L.pm_set_model_table.argtypes = [vp, vp, u32, u32]
        L.pm_set_enabled_mask.argtypes = [vp, u64]
        L.pm_upload_workers.argtypes = [vp, C.POINTER(WorkerSoa), u32]
        L.pm_update_workers.argtypes = [vp, vp, C.POINTER(WorkerSoa)]
        L.pm_upload_tasks.argtypes = [vp, C.POINTER(TaskSoa)]
        L.pm_on_worker_status.argtypes = [vp, u32, u32, u32]
        L.pm_on_worker_status_many.argtypes = [vp, vp, vp, vp, u32]
        L.pm_enable_group_events.argtypes = [vp, u32]
        L.pm_drain_group_events.argtypes = [vp, vp, u32, vp, u32, C.POINTER(u32), C.POINTER(u32)]
        L.pm_dissolve_group.argtypes = [vp, u32]
        L.pm_reset_groups.argtypes = [vp]
        L.pm_compat_masks.argtypes = [vp, vp]
        L.pm_form_groups.argtypes = [vp, C.POINTER(u32)]
        L.pm_merge_solo_groups.argtypes = [vp, C.POINTER(u32)]
        L.pm_get_groups.argtypes = [vp, vp, vp, u32, C.POINTER(u32), vp, u32, C.POINTER(u32)]
        L.pm_match.argtypes = [vp, vp, vp]
        L.pm_match_per_task.argtypes = [vp, vp, vp]
        L.pm_newest_task.argtypes = [vp, C.POINTER(u32)]
        L.pm_tick.argtypes = [vp, C.POINTER(Stats)]
        L.pm_last_stats.argtypes = [vp, C.POINTER(Stats)]
        L.pm_tick_many.argtypes = [C.POINTER(vp), u32, C.POINTER(Stats), u32]
        L.pm_lookup_task_for_worker.argtypes = [vp, u32, C.POINTER(Assignment)]
        L.pm_device_task_column.argtypes = [vp, C.POINTER(u64), C.POINTER(u32)]
        L.pm_append_workers.argtypes = [vp, C.POINTER(WorkerSoa), C.POINTER(u32)]
        L.pm_set_addr_ranks.argtypes = [vp, vp, u32]
        L.pm_tasks_insert_front.argtypes = [vp, C.POINTER(TaskSoa)]
        L.pm_tasks_delete.argtypes = [vp, vp, u32, C.POINTER(u32)]
        L.pm_set_stream.argtypes = [vp, vp]
        L.pm_dist_configure.argtypes = [vp, u32, u32, vp]
        L.pm_dist_tick_begin.argtypes = [vp]
        L.pm_dist_carve_wait.argtypes = [vp]
        L.pm_dissolve_group_by_id.argtypes = [vp, u64, C.POINTER(u32)]
        L.pm_get_group_by_id.argtypes = [vp, u64, vp, vp, u32, C.POINTER(u32)]
        L.pm_get_group_of_worker.argtypes = [vp, u32, vp, vp, u32, C.POINTER(u32)]
        L.pm_adopt_groups.argtypes = [vp, vp, u32, vp, u32, u64]
        L.pm_group_id_state.argtypes = [vp, C.POINTER(u64)]
        L.pm_explain_workers.argtypes = [vp, vp, u32, vp, vp]
        L.pm_config_report.argtypes = [vp, vp, u32, C.POINTER(u32)]
        L.pm_task_report.argtypes = [vp, vp, vp, vp]
        L.pm_group_spread.argtypes = [vp, vp, u32, C.POINTER(u32)]
        L.pm_config_spread.argtypes = [vp, vp, u32, C.POINTER(u32)]
        L.pm_force_regroup.argtypes = [vp, u32, u32, C.c_double, C.POINTER(u32), C.POINTER(u32)]
        L.pm_nearest_workers.argtypes = [vp, vp, u32, u32, u32, vp, vp, vp]
        L.pm_probe_configs.argtypes = [vp, vp, u32, vp, u32, vp, u32, u32, vp, vp, vp]
        L.pm_config_overlap.argtypes = [vp, vp, u32, C.POINTER(u32)]
        L.pm_enable_assignment_changes.argtypes = [vp, u32]
        L.pm_drain_assignment_changes.argtypes = [vp, vp, u32, C.POINTER(u32), C.POINTER(u32)]
        L.pm_liveness_enable.argtypes = [vp, u32, u32]
        L.pm_liveness_set.argtypes = [vp, vp, vp, vp, u32]
        L.pm_liveness_get.argtypes = [vp, vp, u32, vp, vp]
        L.pm_liveness_sweep.argtypes = [vp, u64, vp, vp, u32, C.POINTER(u32), vp]
        L.pm_liveness_transitions.argtypes = [vp, vp, u32, C.POINTER(u32)]
        L.pm_discovery_sync.argtypes = [vp, u64, vp, u32, u32, vp, u32, u32, vp, C.POINTER(u32)]
        L.pm_metrics_enable.argtypes = [vp, u32]
        L.pm_metrics_ingest.argtypes = [vp, vp, u32, vp, u32, u32]
        L.pm_metrics_totals.argtypes = [vp, vp, vp, u32, C.POINTER(u32)]
        L.pm_metrics_rows.argtypes = [vp, vp, u32, vp, u32, C.POINTER(u32)]
        L.pm_rollout_enable.argtypes = [vp, u32]
        L.pm_rollout_ingest.argtypes = [vp, vp, u32]
        L.pm_rollout_get.argtypes = [vp, vp, u32, vp, vp]
        L.pm_rollout_summary.argtypes = [vp, vp]
        L.pm_rollout_tasks.argtypes = [vp, vp, u32, C.POINTER(u32)]
        L.pm_rollout_groups.argtypes = [vp, vp, u32, C.POINTER(u32)]
        L.pm_rollout_workers.argtypes = [vp, u32, vp, u32, C.POINTER(u32)]
        L.pm_directory.argtypes = [vp, vp, C.POINTER(u32), vp, vp, u32, C.POINTER(u32)]
        L.pm_group_directory.argtypes = [vp, vp, vp, vp, u32, vp, u32, C.POINTER(u32), vp, u32, C.POINTER(u32)]
        L.pm_task_directory.argtypes = [vp, vp, vp, vp, u32, vp, u32, C.POINTER(u32)]
        L.pm_dist_match_begin.argtypes = [vp, C.POINTER(DistXfer)]
        L.pm_dist_tick_end.argtypes = [vp, C.POINTER(Stats)]
        L.pm_match_per_task_device.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u32)]
        L.pm_host_parse_requirements.argtypes = [C.c_char_p, vp, vp, u32, C.c_char_p, C.c_size_t]
        L.pm_host_model_matches.argtypes = [C.c_char_p, C.c_char_p]
        L.pm_host_build_model_table.argtypes = [C.POINTER(C.c_char_p), u32, C.POINTER(C.c_char_p), u32, vp]
        L.pm_host_config_order.argtypes = [vp, u32, u64, vp, C.POINTER(u32)]
        sz = C.c_size_t
        L.pm_host_group_vars.argtypes = [C.c_char_p, C.POINTER(GroupVars), C.c_char_p, sz, C.POINTER(sz)]
        L.pm_host_volume_vars.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, sz, C.POINTER(sz)]
        L.pm_host_upload_name_vars.argtypes = [C.c_char_p, C.c_char_p, u32, u32, u64, C.c_char_p, sz, C.POINTER(sz)]
        L.pm_host_to_lowercase.argtypes = [C.c_char_p, C.c_char_p, sz, C.POINTER(sz)]
        L.pm_host_last_file_idx.argtypes = [C.c_char_p]
        L.pm_host_last_file_idx.restype = u32
        L.pm_host_task_state.argtypes = [C.c_char_p]
        L.pm_host_task_state.restype = u32
        L.pm_addresses_enable.argtypes = [vp, u32]
        L.pm_addresses_set.argtypes = [vp, u32, vp, u32]
        L.pm_addresses_rank.argtypes = [vp, vp]
        L.pm_addresses_text.argtypes = [vp, vp, u32, vp]
        L.pm_invite_digests.argtypes = [vp, u32, u32, vp, u32, vp, vp, vp, vp]
        L.pm_ecrecover_many.argtypes = [vp, vp, vp, u32, vp, vp, vp]
        L.pm_verify_requests.argtypes = [vp, vp, vp, vp, vp, vp, u32, vp, vp]
        L.pm_host_ecrecover.argtypes = [vp, vp, vp]
        L.pm_admission_enable.argtypes = [vp, u32]
        L.pm_admit_requests.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, vp, vp, u32, vp, vp]
        L.pm_admission_rate_get.argtypes = [vp, vp, u32, vp, vp]
        L.pm_admission_rate_set.argtypes = [vp, vp, vp, vp, u32]
        L.pm_admission_nonces.argtypes = [vp, u64, C.POINTER(u32), C.POINTER(u32)]
        L.pm_beats_get.argtypes = [vp, vp, u32, vp]
        L.pm_beats_set.argtypes = [vp, vp, vp, u32]
        L.pm_liveness_sweep_beats.argtypes = [vp, u64, vp, vp, u32, C.POINTER(u32), vp]
        # (bound where the library has them: a test library that stubs EXPORTS alone lacks them, and a call then fails by name)
        numbered = {"pm_keccak256_many": [vp, vp, vp, u32, vp], "pm_host_keccak256": [vp, sz, vp], "pm_host_eip55": [vp, vp]}
        for name in EXPORTS_NUMBERED:
            if hasattr(L, name):
                getattr(L, name).argtypes = numbered[name]
        for name in EXPORTS + [n for n in EXPORTS_NUMBERED if hasattr(L, n)]:
            fn = getattr(L, name)
            if name not in ("pm_last_error", "pm_abi_version", "pm_engine_destroy", "pm_engine_config_default",
                            "pm_host_last_file_idx", "pm_host_task_state"):
                fn.restype = i32
        _lib = L
    return _lib


def check(rc: int) -> int:
    if rc < 0:
        raise EngineError(rc, lib().pm_last_error().decode(errors="replace"))
    return rc


def _arr(a, dtype) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=dtype)


def _addr_bytes(addr20) -> np.ndarray:
    """addresses as uint8 [n, 20]: an array of that shape, or a sequence of 20-byte strings"""
    if isinstance(addr20, np.ndarray):
        a = _arr(addr20, np.uint8)
    else:
        a = np.frombuffer(b"".join(bytes(x) for x in addr20), dtype=np.uint8)
    return a.reshape(-1, 20)


def host_keccak256(data: bytes) -> bytes:
    """pm_host_keccak256"""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    out = np.zeros(32, dtype=np.uint8)
    check(lib().pm_host_keccak256(buf.ctypes.data if len(buf) else None, len(buf), out.ctypes.data))
    return out.tobytes()


def host_eip55(addr20: bytes) -> str:
    """pm_host_eip55: the EIP-55 text of 20 bytes"""
    buf = np.frombuffer(bytes(addr20), dtype=np.uint8)
    assert len(buf) == 20
    out = np.zeros(43, dtype=np.uint8)
    check(lib().pm_host_eip55(buf.ctypes.data, out.ctypes.data))
    return out[:42].tobytes().decode("ascii")


def host_ecrecover(hash32: bytes, sig65: bytes):
    """pm_host_ecrecover: the signer's 20 bytes, or None where nothing is recovered"""
    h, g = np.frombuffer(bytes(hash32), dtype=np.uint8), np.frombuffer(bytes(sig65), dtype=np.uint8)
    assert len(h) == 32 and len(g) == 65
    out = np.zeros(20, dtype=np.uint8)
    rc = lib().pm_host_ecrecover(h.ctypes.data, g.ctypes.data, out.ctypes.data)
    if rc == PM_EPARSE:
        return None
    check(rc)
    return out.tobytes()


# pm_rq_verdict, and the codes in the middleware's order
RQ_VERDICT = np.dtype([("code", np.uint32), ("row", np.uint32), ("status", np.uint8), ("_pad", np.uint8, (3,)), ("address", np.uint8, (20,))])
assert RQ_VERDICT.itemsize == 32
RQ_BAD_SIGNATURE, RQ_NO_KEY, RQ_BAD_ADDRESS, RQ_MISMATCH, RQ_UNKNOWN, RQ_EJECTED, RQ_BANNED, RQ_OK, RQ_N_CODES = range(9)
RQ_FLAG_BAD_ADDRESS = 1
# ... and what admission appends (include/pm_engine.h "request gate: admission")
RQ_RATE_LIMITED, RQ_EXPIRED, RQ_BAD_NONCE, RQ_REPLAY, RQ_NO_NONCE, AD_N_CODES = range(8, 14)
RQ_FLAG_NO_TIMESTAMP, RQ_FLAG_NO_NONCE, RQ_FLAG_BEAT = 2, 4, 8
RQ_NONCE_TTL_MS = 60000


def ad_debug_prefix_bits(k: int) -> int:
    """PM_AD_DEBUG_PREFIX_BITS(k) of include/pm_engine_debug.h: `on` for enable_admission with the nonce set's key narrowed to k bits"""
    return 1 | (int(k) << 8)


TICK_MANY_THREADS = 1


def tick_many(engines, threads: bool = False) -> list:
    """pm_tick_many: one match per engine (pool), all of them in one call — the carves started before the first is
    waited for, from one host thread (threads=True: one host thread per engine inside the library, for comparison).
    Returns the engines' stats in order."""
    n = len(engines)
    hs = (C.c_void_p * n)(*[e._h for e in engines])
    st = (Stats * n)()
    check(lib().pm_tick_many(hs, n, st, TICK_MANY_THREADS if threads else 0))
    return [s.as_dict() for s in st]


class Engine:
    """Owns a pm_engine*.  Keeps nothing but the handle: all state lives behind the C ABI."""

    def __init__(self, *, device: int = 0, proximity=True, switching=True, prefer_larger=True,
                 chooser=CHOOSE_FIRST, chooser_seed=0, group_id_seed=1, debug_uncertain_every=0, sweep_variant=0,
                 carve_variant=0, time_proposer=False):
        L = lib()
        cfg = EngineConfig()
        L.pm_engine_config_default(C.byref(cfg))
        cfg.device = device
        cfg.proximity_enabled = int(proximity)
        cfg.switching_enabled = int(switching)
        cfg.prefer_larger_groups = int(prefer_larger)
        cfg.chooser = chooser
        cfg.chooser_seed = chooser_seed
        cfg.group_id_seed = group_id_seed
        cfg.debug_uncertain_every = debug_uncertain_every
        cfg.sweep_variant = sweep_variant
        cfg.carve_variant = carve_variant
        cfg.time_proposer = int(time_proposer)
        self._h = C.c_void_p()
        check(L.pm_engine_create(C.byref(cfg), C.byref(self._h)))
        self.W = 0
        self.C = 0
        self.T = 0

    def close(self):
        if getattr(self, "_h", None):
            lib().pm_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- tables
    def set_configs(self, cfg_rows: np.ndarray, alt_rows: np.ndarray):
        cfg_rows = _arr(cfg_rows, config_row_dt)
        alt_rows = _arr(alt_rows, alt_row_dt)
        check(lib().pm_set_configs(self._h, cfg_rows.ctypes.data, len(cfg_rows),
                                   alt_rows.ctypes.data if len(alt_rows) else None, len(alt_rows)))
        self.C = len(cfg_rows)

    def set_model_table(self, bits: np.ndarray, n_rows: int, n_classes: int):
        bits = _arr(bits, np.uint32)
        check(lib().pm_set_model_table(self._h, bits.ctypes.data if bits.size else None, n_rows, n_classes))

    def set_enabled_mask(self, mask: int):
        check(lib().pm_set_enabled_mask(self._h, mask & 0xFFFFFFFFFFFFFFFF))

    @staticmethod
    def _worker_soa(cols: dict):
        keep = {}
        soa = WorkerSoa()
        n = len(cols["flags"])
        soa.n = n
        for k, dt in (("flags", np.uint32), ("gpu_count", np.uint32), ("gpu_mem_mb", np.uint32),
                      ("gpu_model_class", np.uint32), ("cpu_cores", np.uint32), ("ram_mb", np.uint32),
                      ("storage_gb", np.uint32), ("price", np.uint32), ("addr_rank", np.uint32),
                      ("lat", np.float64), ("lon", np.float64)):
            v = cols.get(k)
            if v is None:
                setattr(soa, k, None)
            else:
                keep[k] = _arr(v, dt)
                assert len(keep[k]) == n, k
                setattr(soa, k, keep[k].ctypes.data)
        return soa, keep

    def upload_workers(self, cols: dict, keep_groups: bool = False):
        soa, keep = self._worker_soa(cols)
        check(lib().pm_upload_workers(self._h, C.byref(soa), int(keep_groups)))
        self.W = soa.n

    def update_workers(self, idx, cols: dict):
        idx = _arr(idx, np.uint32)
        soa, keep = self._worker_soa(cols)
        assert soa.n == len(idx)
        check(lib().pm_update_workers(self._h, idx.ctypes.data, C.byref(soa)))

    def append_workers(self, cols: dict) -> int:
        """-> index of the first appended row"""
        soa, keep = self._worker_soa(cols)
        first = C.c_uint32(0)
        check(lib().pm_append_workers(self._h, C.byref(soa), C.byref(first)))
        self.W += soa.n
        return first.value

    def set_addr_ranks(self, ranks):
        r = _arr(ranks, np.uint32)
        check(lib().pm_set_addr_ranks(self._h, r.ctypes.data if len(r) else None, len(r)))

    @staticmethod
    def _task_soa(topo_mask, created_at, uid):
        tm, ca = _arr(topo_mask, np.uint64), _arr(created_at, np.int64)
        soa = TaskSoa()
        soa.n = len(tm)
        soa.topo_mask = tm.ctypes.data if len(tm) else None
        soa.created_at = ca.ctypes.data if len(ca) else None
        u = None
        if uid is not None:
            u = _arr(uid, np.uint64)
            soa.uid = u.ctypes.data if len(u) else None
        return soa, (tm, ca, u)

    def upload_tasks(self, topo_mask, created_at, uid=None):
        soa, keep = self._task_soa(topo_mask, created_at, uid)
        check(lib().pm_upload_tasks(self._h, C.byref(soa)))
        self.T = soa.n

    def tasks_insert_front(self, topo_mask, created_at, uid=None, republish=False):
        """new tasks, newest first; they sort in front of the table (on_task_created).  republish: also run pm_match's
        pair sweep + claim + publish on the standing groups (pm_tasks_insert_front_ex), so that a group holding no task
        is served the new one before the next tick"""
        soa, keep = self._task_soa(topo_mask, created_at, uid)
        if republish:
            check(lib().pm_tasks_insert_front_ex(self._h, C.byref(soa), 1))
        else:
            check(lib().pm_tasks_insert_front(self._h, C.byref(soa)))
        self.T += soa.n

    def set_carve_workgroups(self, n: int):
        """row-making workgroups of the carve's launch (0 = by the size of the swarm): the share of the GPU this engine
        takes when several pools match on it at the same time"""
        check(lib().pm_set_carve_workgroups(self._h, int(n)))

    def tasks_delete(self, uids) -> int:
        u = _arr(uids, np.uint64)
        n = C.c_uint32(0)
        check(lib().pm_tasks_delete(self._h, u.ctypes.data if len(u) else None, len(u), C.byref(n)))
        self.T -= n.value
        return n.value

    # ---- events
    def on_worker_status(self, worker: int, flags_new: int, dead: bool):
        check(lib().pm_on_worker_status(self._h, worker, flags_new, int(dead)))

    def on_worker_status_many(self, workers, flags_new, dead=None):
        """pm_on_worker_status for a batch, in array order; `dead`: per-entry flags (None = nobody)."""
        w, f = _arr(workers, np.uint32), _arr(flags_new, np.uint32)
        assert len(w) == len(f)
        d = _arr(dead, np.uint32) if dead is not None else None
        assert d is None or len(d) == len(w)
        check(lib().pm_on_worker_status_many(self._h, w.ctypes.data if len(w) else None, f.ctypes.data if len(f) else None,
                                             d.ctypes.data if d is not None and len(d) else None, len(w)))

    def enable_group_events(self, on: bool = True):
        check(lib().pm_enable_group_events(self._h, int(on)))

    def drain_group_events(self):
        """[(kind, group id, config, members in BTreeSet order)] since the last drain (kind 1 = created, 2 = destroyed):
        the webhook feed, in the order the reference emits it"""
        ne, nm = C.c_uint32(0), C.c_uint32(0)
        rc = lib().pm_drain_group_events(self._h, None, 0, None, 0, C.byref(ne), C.byref(nm))
        if rc == 0:
            return []                                          # the log is empty
        ev = np.zeros(max(ne.value, 1), dtype=GROUP_EVENT)
        mem = np.zeros(max(nm.value, 1), dtype=np.uint32)
        check(lib().pm_drain_group_events(self._h, ev.ctypes.data, len(ev), mem.ctypes.data, len(mem), C.byref(ne),
                                          C.byref(nm)))
        return [(int(e["kind"]), int(e["group_id"]), int(e["config"]),
                 mem[int(e["member_begin"]):int(e["member_begin"]) + int(e["n_members"])].tolist()) for e in ev[:ne.value]]

    def dissolve_group(self, slot: int):
        check(lib().pm_dissolve_group(self._h, slot))

    def dissolve_group_by_id(self, group_id: int) -> bool:
        """dissolve_group(&group_id) (mod.rs:1002-1004): False = no group has this id (not an error)"""
        n = C.c_uint32(0)
        check(lib().pm_dissolve_group_by_id(self._h, int(group_id), C.byref(n)))
        return bool(n.value)

    def _one_group(self, call):
        g = np.zeros(1, dtype=group_dt)
        slot = C.c_uint32(0)
        members = np.zeros(64, dtype=np.uint32)
        rc = call(g.ctypes.data, members.ctypes.data, len(members), C.byref(slot))
        if rc == PM_ERANGE and slot.value != PM_NONE:            # a group of more than 64: its size is in the record
            members = np.zeros(int(g[0]["n_members"]), dtype=np.uint32)
            rc = call(g.ctypes.data, members.ctypes.data, len(members), C.byref(slot))
        check(rc)
        if slot.value == PM_NONE:
            return None
        n = int(g[0]["n_members"])
        return {"slot": slot.value, "id": int(g[0]["id"]), "config": int(g[0]["config"]), "task": int(g[0]["task"]),
                "members": members[:n].tolist()}

    def get_group_by_id(self, group_id: int):
        """get_group_by_id (mod.rs:1046-1055) -> None or {slot, id, config, task, members (BTreeSet order)}"""
        return self._one_group(lambda g, m, cap, s: lib().pm_get_group_by_id(self._h, int(group_id), g, m, cap, s))

    def get_group_of_worker(self, worker: int):
        """get_node_group (mod.rs:324-337) by row index -> None or the same record"""
        return self._one_group(lambda g, m, cap, s: lib().pm_get_group_of_worker(self._h, int(worker), g, m, cap, s))

    def reset_groups(self):
        check(lib().pm_reset_groups(self._h))

    def adopt_groups(self, groups, members, id_state: int):
        """pm_adopt_groups: install a group list into an engine that holds none -- `groups` (group_dt records) and `members`
        exactly as get_groups() returns them, `id_state` as group_id_state() returned it"""
        g = np.ascontiguousarray(groups, dtype=group_dt)
        m = _arr(members, np.uint32)
        check(lib().pm_adopt_groups(self._h, g.ctypes.data if len(g) else None, len(g), m.ctypes.data if len(m) else None,
                                    len(m), int(id_state) & 0xFFFFFFFFFFFFFFFF))

    def group_id_state(self) -> int:
        """the state of the group id stream (splitmix64), for a successor's adopt_groups"""
        s = C.c_uint64(0)
        check(lib().pm_group_id_state(self._h, C.byref(s)))
        return s.value

    # ---- diagnostics (read-only reports; they change nothing the next tick does)
    def explain_workers(self, workers=None):
        """pm_explain_workers -> (why: uint8 [n, C], the PM_WHY_* code of every (worker, configuration) pair; state: uint32 [n],
        PM_WS_*).  workers=None: every row."""
        w = np.arange(self.W, dtype=np.uint32) if workers is None else _arr(workers, np.uint32)
        why = np.zeros((len(w), self.C), dtype=np.uint8)
        state = np.zeros(len(w), dtype=np.uint32)
        check(lib().pm_explain_workers(self._h, w.ctypes.data if len(w) else None, len(w),
                                       why.ctypes.data if why.size else None, state.ctypes.data if len(w) else None))
        return why, state

    def config_report(self) -> np.ndarray:
        """pm_config_report -> one config_report_dt record per configuration (pm_set_configs row order)"""
        out = np.zeros(self.C, dtype=config_report_dt)
        n = C.c_uint32(0)
        check(lib().pm_config_report(self._h, out.ctypes.data if self.C else None, self.C, C.byref(n)))
        return out[:n.value]

    def task_report(self):
        """pm_task_report -> (groups_running, workers_running, groups_allowed), uint32 [T] each, by task position"""
        outs = [np.zeros(self.T, dtype=np.uint32) for _ in range(3)]
        check(lib().pm_task_report(self._h, *[o.ctypes.data if self.T else None for o in outs]))
        return tuple(outs)

    # ---- group geography (read-only reports) and the force-regroup route
    def group_spread(self) -> np.ndarray:
        """pm_group_spread -> one group_spread_dt record per live group, in the slot order get_groups would give now"""
        n = C.c_uint32(0)
        rc = lib().pm_group_spread(self._h, None, 0, C.byref(n))
        if rc != -5:  # PM_ERANGE: the size query
            check(rc)
        out = np.zeros(n.value, dtype=group_spread_dt)
        if n.value:
            check(lib().pm_group_spread(self._h, out.ctypes.data, n.value, C.byref(n)))
        return out[:n.value]

    def config_spread(self) -> np.ndarray:
        """pm_config_spread -> one config_spread_dt record per configuration (pm_set_configs row order)"""
        out = np.zeros(self.C, dtype=config_spread_dt)
        n = C.c_uint32(0)
        check(lib().pm_config_spread(self._h, out.ctypes.data if self.C else None, self.C, C.byref(n)))
        return out[:n.value]

    def force_regroup(self, config, metric=0, threshold_km=0.0):
        """pm_force_regroup -> (dissolved_groups, affected_workers)"""
        g, w = C.c_uint32(0), C.c_uint32(0)
        check(lib().pm_force_regroup(self._h, int(config), int(metric), float(threshold_km), C.byref(g), C.byref(w)))
        return g.value, w.value

    # ---- nearest candidates (read-only)
    def nearest_workers(self, queries, pool=NEAR_IDLE, k=16, want_km=True):
        """pm_nearest_workers -> (rows: near_row_dt [n_q], workers: uint32 [n_q, k], km: float64 [n_q, k] or None).
        `queries`: (origin, config) pairs (or near_query_dt records); origin a worker index or NEAR_SEED.  Entries behind
        rows[i]["n"] read PM_NONE / DBL_MAX."""
        if isinstance(queries, np.ndarray) and queries.dtype == near_query_dt:
            q = np.ascontiguousarray(queries)
        else:
            q = np.zeros(len(queries), dtype=near_query_dt)
            for i, (o, c) in enumerate(queries):
                q[i] = (int(o), int(c))
        n, kk = len(q), max(int(k), 0)
        rows = np.zeros(n, dtype=near_row_dt)
        workers = np.full((n, kk), PM_NONE, dtype=np.uint32)
        km = np.full((n, kk), np.finfo(np.float64).max, dtype=np.float64) if want_km else None
        check(lib().pm_nearest_workers(self._h, q.ctypes.data if n else None, n, int(pool), int(k),
                                       rows.ctypes.data if n else None, workers.ctypes.data if n else None,
                                       km.ctypes.data if (want_km and n) else None))
        return rows, workers, km

    # ---- probes and configuration overlap (read-only)
    def probe_configs(self, cfg_rows, alt_rows, bits, n_model_rows, n_classes, want_overlap=True, want_mask=True):
        """pm_probe_configs -> (rows: probe_row_dt [P], overlap: uint32 [P, C] or None, mask: uint64 [W] or None).
        `cfg_rows` / `alt_rows` / `bits`: configuration rows that are NOT installed, with their own alternative and model
        bit tables (host.pack_probes builds them); n_classes must be the installed table's class count."""
        cfg_rows = _arr(cfg_rows, config_row_dt)
        alt_rows = _arr(alt_rows, alt_row_dt)
        bits = _arr(bits, np.uint32)
        n = len(cfg_rows)
        rows = np.zeros(n, dtype=probe_row_dt)
        overlap = np.zeros((n, self.C), dtype=np.uint32) if want_overlap else None
        mask = np.zeros(self.W, dtype=np.uint64) if want_mask else None
        check(lib().pm_probe_configs(self._h, cfg_rows.ctypes.data if n else None, n,
                                     alt_rows.ctypes.data if len(alt_rows) else None, len(alt_rows),
                                     bits.ctypes.data if bits.size else None, int(n_model_rows), int(n_classes),
                                     rows.ctypes.data if n else None,
                                     overlap.ctypes.data if (want_overlap and overlap.size) else None,
                                     mask.ctypes.data if (want_mask and self.W) else None))
        return rows, overlap, mask

    def config_overlap(self) -> np.ndarray:
        """pm_config_overlap -> uint32 [C, C]: the idle workers that meet both configurations (pm_set_configs row order)"""
        out = np.zeros((self.C, self.C), dtype=np.uint32)
        n = C.c_uint32(0)
        check(lib().pm_config_overlap(self._h, out.ctypes.data if self.C else None, out.size, C.byref(n)))
        return out

    # ---- assignment change feed
    def enable_assignment_changes(self, on: bool = True):
        """pm_enable_assignment_changes: on = resync (the next publish lists every row); off also clears"""
        check(lib().pm_enable_assignment_changes(self._h, int(on)))

    def drain_assignment_changes(self):
        """pm_drain_assignment_changes -> (workers: uint32 [n] ascending, what: uint32 [n] OR of CHG_*, resync: bool).
        The size query, then the drain (again if a publish lengthened the list in between)."""
        n, flags = C.c_uint32(0), C.c_uint32(0)
        rc = lib().pm_drain_assignment_changes(self._h, None, 0, C.byref(n), C.byref(flags))
        while True:
            if rc != -5:                                       # (PM_ERANGE is the size query's answer)
                check(rc)
            rows = np.zeros(max(n.value, 1), dtype=change_row_dt)
            rc = lib().pm_drain_assignment_changes(self._h, rows.ctypes.data, len(rows), C.byref(n), C.byref(flags))
            if rc == 0:
                break
        rows = rows[:n.value]
        return rows["worker"].copy(), rows["what"].copy(), bool(flags.value & CHANGES_RESYNC)

    # ---- liveness
    def liveness_enable(self, on: bool = True, missing_heartbeat_threshold: int = 3):
        """pm_liveness_enable: on = (re-)initialise the ledger from the host's flags; off releases it"""
        check(lib().pm_liveness_enable(self._h, int(on), int(missing_heartbeat_threshold)))

    def liveness_set(self, idx, status, counter=None):
        """pm_liveness_set: ledger rows idx <- (status, counter or 0); a repeated index takes its last entry"""
        i, s = _arr(idx, np.uint32), _arr(status, np.uint8)
        c = _arr(counter, np.uint32) if counter is not None else None
        assert len(i) == len(s) and (c is None or len(c) == len(i))
        n = len(i)
        check(lib().pm_liveness_set(self._h, i.ctypes.data if n else None, s.ctypes.data if n else None,
                                    c.ctypes.data if c is not None and n else None, n))

    def liveness_get(self, idx=None):
        """pm_liveness_get -> (status uint8 [n], counter uint32 [n]) of the rows idx (None = every row)"""
        i = _arr(idx, np.uint32) if idx is not None else np.arange(self.W, dtype=np.uint32)
        n = len(i)
        s, c = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint32)
        check(lib().pm_liveness_get(self._h, i.ctypes.data if n else None, n, s.ctypes.data if n else None,
                                    c.ctypes.data if n else None))
        return s, c

    def liveness_sweep(self, now_ms: int, last_beat_ms, in_pool_bits=None, apply: bool = False):
        """pm_liveness_sweep -> (n_transitions, census uint32 [NS_N]).  last_beat_ms: uint64 [W]; in_pool_bits: uint64
        [(W + 63) // 64] or None (all in pool)"""
        b = _arr(last_beat_ms, np.uint64) if last_beat_ms is not None else None
        assert b is None or len(b) == self.W
        p = _arr(in_pool_bits, np.uint64) if in_pool_bits is not None else None
        assert p is None or len(p) == (self.W + 63) // 64
        n, census = C.c_uint32(0), np.zeros(NS_N, dtype=np.uint32)
        check(lib().pm_liveness_sweep(self._h, int(now_ms), b.ctypes.data if b is not None and len(b) else None,
                                      p.ctypes.data if p is not None and len(p) else None, int(apply), C.byref(n),
                                      census.ctypes.data))
        return n.value, census

    def liveness_transitions(self) -> np.ndarray:
        """pm_liveness_transitions -> live_row_dt [n], ascending by worker: the last sweep's list (reading consumes nothing)"""
        n = C.c_uint32(0)
        rc = lib().pm_liveness_transitions(self._h, None, 0, C.byref(n))
        if rc != -5:                                           # (PM_ERANGE is the size query's answer)
            check(rc)
        rows = np.zeros(max(n.value, 1), dtype=live_row_dt)
        check(lib().pm_liveness_transitions(self._h, rows.ctypes.data, len(rows), C.byref(n)))
        return rows[:n.value]

    # ---- discovery sync
    def discovery_sync(self, now_ms: int, row_endpoint, n_endpoints: int, max_healthy_same_endpoint: int, rows,
                       apply: bool = False):
        """pm_discovery_sync -> (disc_result_dt [n_rows] in input order, n_updates_total).  row_endpoint: uint32 [W] (EP_NONE =
        matches nothing); rows: disc_row_dt [n_rows], the de-duplicated discovery list in order"""
        ep = _arr(row_endpoint, np.uint32) if row_endpoint is not None else None
        assert ep is None or len(ep) == self.W
        r = np.ascontiguousarray(rows, dtype=disc_row_dt)
        n, total = len(r), C.c_uint32(0)
        out = np.zeros(n, dtype=disc_result_dt)
        check(lib().pm_discovery_sync(self._h, int(now_ms), ep.ctypes.data if ep is not None and len(ep) else None,
                                      int(n_endpoints), int(max_healthy_same_endpoint), r.ctypes.data if n else None, n,
                                      int(apply), out.ctypes.data if n else None, C.byref(total)))
        return out, total.value

    # ---- metrics ledger
    def metrics_enable(self, on: bool = True):
        """pm_metrics_enable: on = an empty ledger (again: empties it); off releases it"""
        check(lib().pm_metrics_enable(self._h, int(on)))

    def metrics_ingest(self, beats, entries, n_series: int):
        """pm_metrics_ingest: beats (mx_beat_dt) applied in order over entries (mx_entry_dt); every series < n_series"""
        b = np.ascontiguousarray(beats, dtype=mx_beat_dt)
        en = np.ascontiguousarray(entries, dtype=mx_entry_dt)
        check(lib().pm_metrics_ingest(self._h, b.ctypes.data if len(b) else None, len(b), en.ctypes.data if len(en) else None,
                                      len(en), int(n_series)))

    def metrics_totals(self):
        """pm_metrics_totals -> (sum float64 [n_series], count uint32 [n_series]): per series over all rows, ascending row"""
        n = C.c_uint32(0)
        rc = lib().pm_metrics_totals(self._h, None, None, 0, C.byref(n))
        if rc != -5:                                           # (PM_ERANGE is the size query's answer)
            check(rc)
        s, c = np.zeros(max(n.value, 1), dtype=np.float64), np.zeros(max(n.value, 1), dtype=np.uint32)
        check(lib().pm_metrics_totals(self._h, s.ctypes.data, c.ctypes.data, len(s), C.byref(n)))
        return s[:n.value], c[:n.value]

    def metrics_rows(self, rows=None) -> np.ndarray:
        """pm_metrics_rows -> mx_row_dt [n]: every entry (rows=None: the manual row's, then ascending (worker, series)) or the
        entries of the named rows in the order named, each with its worker's group id and configuration"""
        r = _arr(rows, np.uint32) if rows is not None else None
        if r is not None and not len(r):
            return np.zeros(0, dtype=mx_row_dt)
        rp, rn = (r.ctypes.data, len(r)) if r is not None else (None, 0)
        n = C.c_uint32(0)
        rc = lib().pm_metrics_rows(self._h, rp, rn, None, 0, C.byref(n))
        if rc != -5:
            check(rc)
        out = np.zeros(max(n.value, 1), dtype=mx_row_dt)
        check(lib().pm_metrics_rows(self._h, rp, rn, out.ctypes.data, len(out), C.byref(n)))
        return out[:n.value]

    # ---- phases
    # ---- rollout ledger
    def rollout_enable(self, on: bool = True):
        """pm_rollout_enable: on = empty columns for the rows [0, W) (again: empties them); off releases them"""
        check(lib().pm_rollout_enable(self._h, int(on)))

    def rollout_ingest(self, reports):
        """pm_rollout_ingest: reports (ro_report_dt) applied in order; state TS_NONE clears the row; the last entry of a worker wins"""
        r = np.ascontiguousarray(reports, dtype=ro_report_dt)
        check(lib().pm_rollout_ingest(self._h, r.ctypes.data if len(r) else None, len(r)))

    def rollout_get(self, idx=None):
        """pm_rollout_get -> (uid uint64 [n], state uint8 [n]) of the rows idx (None: every row)"""
        idx = np.arange(self.W, dtype=np.uint32) if idx is None else _arr(idx, np.uint32)
        uid = np.zeros(len(idx), dtype=np.uint64)
        st = np.zeros(len(idx), dtype=np.uint8)
        check(lib().pm_rollout_get(self._h, idx.ctypes.data if len(idx) else None, len(idx), uid.ctypes.data, st.ctypes.data))
        return uid, st

    def rollout_summary(self) -> np.ndarray:
        """pm_rollout_summary -> one ro_summary_dt record"""
        out = np.zeros(1, dtype=ro_summary_dt)
        check(lib().pm_rollout_summary(self._h, out.ctypes.data))
        return out[0]

    def _rollout_list(self, call, dt) -> np.ndarray:
        n = C.c_uint32(0)
        rc = call(None, 0, C.byref(n))
        if rc < 0 and rc != -5:  # (PM_ERANGE with *n set: the size query)
            check(rc)
        out = np.zeros(max(n.value, 1), dtype=dt)
        check(call(out.ctypes.data, len(out), C.byref(n)))
        return out[:n.value]

    def rollout_tasks(self) -> np.ndarray:
        """pm_rollout_tasks -> ro_task_row_dt [n]: one row per distinct claimed or reported id, ascending by uid"""
        return self._rollout_list(lambda p, cap, n: lib().pm_rollout_tasks(self._h, p, cap, n), ro_task_row_dt)

    def rollout_groups(self) -> np.ndarray:
        """pm_rollout_groups -> ro_group_row_dt [n]: one row per live group that holds a task, in get_groups order"""
        return self._rollout_list(lambda p, cap, n: lib().pm_rollout_groups(self._h, p, cap, n), ro_group_row_dt)

    def rollout_workers(self, class_mask: int = (1 << RO_N) - 1) -> np.ndarray:
        """pm_rollout_workers -> ro_worker_row_dt [n]: the workers whose class bit is in class_mask, ascending"""
        return self._rollout_list(lambda p, cap, n: lib().pm_rollout_workers(self._h, int(class_mask), p, cap, n), ro_worker_row_dt)

    # ---- node directory
    def directory(self, status_mask: int = (1 << NS_N) - 1, membership: int = DIR_ANY, order: int = DIR_BY_ROW, offset: int = 0,
                  limit=None):
        """pm_directory -> (total, counts uint32 [NS_N], rows dir_row_dt [n]): the window [offset, offset + limit) of the listed
        rows in (class, base key, row) order; limit None = to the end, 0 = the counters alone"""
        q = np.zeros(1, dtype=dir_query_dt)
        q[0] = (int(status_mask), int(membership), int(order), int(offset), 0xFFFFFFFF if limit is None else int(limit))
        total, n, counts = C.c_uint32(0), C.c_uint32(0), np.zeros(NS_N, dtype=np.uint32)
        rc = lib().pm_directory(self._h, q.ctypes.data, C.byref(total), counts.ctypes.data, None, 0, C.byref(n))
        if rc != -5:                                           # (PM_ERANGE is the size query's answer)
            check(rc)
        if not n.value:
            return total.value, counts, np.zeros(0, dtype=dir_row_dt)
        rows = np.zeros(n.value, dtype=dir_row_dt)
        check(lib().pm_directory(self._h, q.ctypes.data, C.byref(total), counts.ctypes.data, rows.ctypes.data, len(rows),
                                 C.byref(n)))
        return total.value, counts, rows[:n.value]

    def group_directory(self, config_mask: int = 0xFFFFFFFFFFFFFFFF, holds: int = GDIR_ANY, size_min: int = 0,
                        size_max: int = 0xFFFFFFFF, health_mask: int = (1 << GH_N) - 1, rollout_mask: int = (1 << GR_N) - 1,
                        order: int = GDIR_BY_SLOT, offset: int = 0, limit=None, want_members: bool = True):
        """pm_group_directory -> (totals gdir_totals_dt record, by_config uint32 [n_cfgs], rows gdir_row_dt [n], members uint32
        [n_members] or None): the window [offset, offset + limit) of the listed groups in the chosen order; limit None = to the
        end, 0 = the counters alone"""
        q = np.zeros(1, dtype=gdir_query_dt)
        q[0] = (int(config_mask) & 0xFFFFFFFFFFFFFFFF, int(holds), int(size_min), int(size_max), int(health_mask),
                int(rollout_mask), int(order), int(offset), 0xFFFFFFFF if limit is None else int(limit))
        totals = np.zeros(1, dtype=gdir_totals_dt)
        by_config = np.zeros(PM_MAX_CONFIGS, dtype=np.uint32)
        n, nm = C.c_uint32(0), C.c_uint32(0)
        # the counters-only query first (limit 0: no sort, no row): its totals size the buffers for the ONE call that makes the window
        lim = int(q[0]["limit"])
        q[0]["limit"] = 0
        check(lib().pm_group_directory(self._h, q.ctypes.data, totals.ctypes.data, by_config.ctypes.data, len(by_config), None, 0,
                                       C.byref(n), None, 0, C.byref(nm)))
        q[0]["limit"] = lim
        total, off = int(totals[0]["total"]), int(q[0]["offset"])
        rows = np.zeros(0 if off >= total else min(lim, total - off), dtype=gdir_row_dt)
        members = np.zeros(int(totals[0]["members_total"]) if len(rows) else 0, dtype=np.uint32) if want_members else None
        if len(rows):
            check(lib().pm_group_directory(self._h, q.ctypes.data, totals.ctypes.data, by_config.ctypes.data, len(by_config),
                                           rows.ctypes.data, len(rows), C.byref(n),
                                           members.ctypes.data if want_members and len(members) else None,
                                           len(members) if want_members else 0, C.byref(nm)))
        return totals[0], by_config[:int(totals[0]["n_cfgs"])].copy(), rows[:n.value], None if members is None else members[:nm.value]

    def task_directory(self, config_mask: int = 0xFFFFFFFFFFFFFFFF, serve_mask: int = (1 << TKS_N) - 1,
                       rollout_mask: int = (1 << TKR_N) - 1, workers_min: int = 0, workers_max: int = 0xFFFFFFFF,
                       order: int = TDIR_BY_LIST, offset: int = 0, limit=None):
        """pm_task_directory -> (totals tdir_totals_dt record, by_config uint32 [n_cfgs], rows tdir_row_dt [n]): the window
        [offset, offset + limit) of the listed tasks in the chosen order; limit None = to the end, 0 = the counters alone"""
        q = np.zeros(1, dtype=tdir_query_dt)
        lim = 0xFFFFFFFF if limit is None else int(limit)
        # the counters-only query first (limit 0: no sort, no row): its total sizes the buffer for the call that makes the window
        q[0] = (int(config_mask) & 0xFFFFFFFFFFFFFFFF, int(serve_mask), int(rollout_mask), int(workers_min), int(workers_max),
                int(order), int(offset), 0, 0)
        totals = np.zeros(1, dtype=tdir_totals_dt)
        by_config = np.zeros(PM_MAX_CONFIGS, dtype=np.uint32)
        n = C.c_uint32(0)
        check(lib().pm_task_directory(self._h, q.ctypes.data, totals.ctypes.data, by_config.ctypes.data, len(by_config), None, 0,
                                      C.byref(n)))
        q[0]["limit"] = lim
        total, off = int(totals[0]["total"]), int(q[0]["offset"])
        rows = np.zeros(0 if off >= total else min(lim, total - off), dtype=tdir_row_dt)
        if len(rows):
            check(lib().pm_task_directory(self._h, q.ctypes.data, totals.ctypes.data, by_config.ctypes.data, len(by_config),
                                          rows.ctypes.data, len(rows), C.byref(n)))
        return totals[0], by_config[:int(totals[0]["n_cfgs"])].copy(), rows[:n.value]

    def compat_masks(self) -> np.ndarray:
        out = np.zeros(self.W, dtype=np.uint64)
        check(lib().pm_compat_masks(self._h, out.ctypes.data if self.W else None))
        return out

    def form_groups(self) -> int:
        n = C.c_uint32(0)
        check(lib().pm_form_groups(self._h, C.byref(n)))
        return n.value

    def merge_solo_groups(self) -> int:
        n = C.c_uint32(0)
        check(lib().pm_merge_solo_groups(self._h, C.byref(n)))
        return n.value

    def get_groups(self):
        """-> (group_of_worker int32[W], groups structured array, members uint32[] in BTreeSet order)"""
        ng, nm = C.c_uint32(0), C.c_uint32(0)
        check(lib().pm_get_groups(self._h, None, None, 0, C.byref(ng), None, 0, C.byref(nm)))
        gow = np.zeros(self.W, dtype=np.int32)
        groups = np.zeros(ng.value, dtype=group_dt)
        members = np.zeros(nm.value, dtype=np.uint32)
        check(lib().pm_get_groups(self._h, gow.ctypes.data if self.W else None,
                                  groups.ctypes.data if ng.value else None, ng.value, C.byref(ng),
                                  members.ctypes.data if nm.value else None, nm.value, C.byref(nm)))
        return gow, groups, members

    def match(self):
        task = np.zeros(self.W, dtype=np.uint32)
        count = np.zeros(self.W, dtype=np.uint32)
        check(lib().pm_match(self._h, task.ctypes.data if self.W else None, count.ctypes.data if self.W else None))
        return task, count

    def match_per_task(self):
        best = np.zeros(self.T, dtype=np.uint32)
        count = np.zeros(self.T, dtype=np.uint32)
        check(lib().pm_match_per_task(self._h, best.ctypes.data if self.T else None,
                                      count.ctypes.data if self.T else None))
        return best, count

    def newest_task(self) -> int:
        t = C.c_uint32(0)
        check(lib().pm_newest_task(self._h, C.byref(t)))
        return t.value

    def tick(self) -> dict:
        s = Stats()
        check(lib().pm_tick(self._h, C.byref(s)))
        return s.as_dict()

    def last_stats(self) -> dict:
        s = Stats()
        check(lib().pm_last_stats(self._h, C.byref(s)))
        return s.as_dict()

    def device_task_column(self):
        """(device pointer, n) of the published per-worker task column — for device-side consumers."""
        p, n = C.c_uint64(0), C.c_uint32(0)
        check(lib().pm_device_task_column(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    # ---- multi-GPU: ownership + the stepwise tick (the exchanges are the caller's, protocol_amd/dist.py)
    def set_stream(self, hip_stream: int | None):
        check(lib().pm_set_stream(self._h, C.c_void_p(hip_stream or 0)))

    def dist_configure(self, rank: int, world: int, shard_of_worker=None):
        sh = None if shard_of_worker is None else _arr(shard_of_worker, np.uint8)
        if sh is not None:
            assert len(sh) == self.W
        check(lib().pm_dist_configure(self._h, rank, world, sh.ctypes.data if sh is not None and len(sh) else None))

    def dist_tick_begin(self):
        check(lib().pm_dist_tick_begin(self._h))

    def dist_carve_wait(self):
        check(lib().pm_dist_carve_wait(self._h))

    def dist_match_begin(self) -> DistXfer:
        x = DistXfer()
        check(lib().pm_dist_match_begin(self._h, C.byref(x)))
        return x

    def dist_tick_end(self) -> dict:
        s = Stats()
        check(lib().pm_dist_tick_end(self._h, C.byref(s)))
        return s.as_dict()

    def match_per_task_device(self):
        """-> (device pointer of best u32[T], device pointer of count u32[T], T)"""
        b, c, n = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
        check(lib().pm_match_per_task_device(self._h, C.byref(b), C.byref(c), C.byref(n)))
        return b.value, c.value, n.value

    def hbm_triad_gbs(self, n_doubles: int = 1 << 27, reps: int = 5) -> float:
        """measured HBM rate (stream triad over 3 x n_doubles f64) — a debug export, not part of the ABI header"""
        L = lib()
        L.pm_debug_hbm_triad.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_double)]
        L.pm_debug_hbm_triad.restype = C.c_int32
        out = C.c_double(0)
        check(L.pm_debug_hbm_triad(self._h, n_doubles, reps, C.byref(out)))
        return out.value

    def debug_mem_lists_above(self, n: int):
        """test hook (pm_internal.h): candidate lists longer than n slots take the all-in-HBM carve path; 0 = off"""
        L = lib()
        L.pm_debug_mem_lists_above.argtypes = [C.c_void_p, C.c_uint32]
        L.pm_debug_mem_lists_above.restype = C.c_int32
        check(L.pm_debug_mem_lists_above(self._h, n))

    def debug_stream_abort_after(self, n: int):
        """test hook (include/pm_engine_debug.h): the streaming carve gives its launch up (CARVE_STATE_ABORTED) once n
        steps are committed, and the engine continues on the batch pipeline; 0 = off"""
        L = lib()
        L.pm_debug_stream_abort_after.argtypes = [C.c_void_p, C.c_uint32]
        L.pm_debug_stream_abort_after.restype = C.c_int32
        check(L.pm_debug_stream_abort_after(self._h, n))

    def debug_merge_streamed(self) -> int:
        """merge configurations whose selections went through the streaming carve since the engine was created"""
        L = lib()
        L.pm_debug_merge_streamed.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.pm_debug_merge_streamed.restype = C.c_int32
        n = C.c_uint32(0)
        check(L.pm_debug_merge_streamed(self._h, C.byref(n)))
        return n.value

    def debug_delta_pushes(self) -> int:
        """times the device's group state went up as a delta instead of the whole list since the engine was created"""
        L = lib()
        L.pm_debug_delta_pushes.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.pm_debug_delta_pushes.restype = C.c_int32
        n = C.c_uint32(0)
        check(L.pm_debug_delta_pushes(self._h, C.byref(n)))
        return n.value

    def debug_per_task_path(self) -> tuple:
        """(distinct valid masks the last match_per_task counted — 0 when it did not count —, whether it swept once per
        distinct mask) (include/pm_engine_debug.h)"""
        L = lib()
        L.pm_debug_per_task_path.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.pm_debug_per_task_path.restype = C.c_int32
        n, interned = C.c_uint32(0), C.c_uint32(0)
        check(L.pm_debug_per_task_path(self._h, C.byref(n), C.byref(interned)))
        return n.value, bool(interned.value)

    @staticmethod
    def debug_live_allocations() -> tuple:
        """(device bytes, pinned host bytes, events + streams) the engines of this process hold from the HIP runtime right
        now (include/pm_engine_debug.h): a destroyed engine gives back all it took"""
        L = lib()
        L.pm_debug_live_allocations.argtypes = [C.POINTER(C.c_uint64)]
        L.pm_debug_live_allocations.restype = None
        out = (C.c_uint64 * 3)()
        L.pm_debug_live_allocations(out)
        return tuple(int(v) for v in out)

    # ---- address book (include/pm_engine.h "address book")
    def enable_addresses(self, on: bool = True):
        """pm_addresses_enable: on = an empty book over the rows [0, W) (again: empties it); off frees it"""
        check(lib().pm_addresses_enable(self._h, int(on)))

    def set_addresses(self, first_row: int, addr20):
        """pm_addresses_set: rows [first_row, first_row + n) <- addr20 (uint8 [n, 20], or n 20-byte strings)"""
        a = _addr_bytes(addr20)
        check(lib().pm_addresses_set(self._h, first_row, a.ctypes.data if len(a) else None, len(a)))

    def rank_addresses(self, want: bool = True):
        """pm_addresses_rank: ranks the EIP-55 texts and installs them as set_addr_ranks would -> the ranks (uint32 [W]) or None"""
        out = np.zeros(self.W, dtype=np.uint32) if want else None
        check(lib().pm_addresses_rank(self._h, out.ctypes.data if want and self.W else None))
        return out

    def address_texts(self, rows=None, n: int | None = None) -> list:
        """pm_addresses_text -> the EIP-55 texts ("0x" + 40 characters) of the rows (None: the rows [0, n), n None: every row)"""
        if rows is None:
            n, ptr = (self.W if n is None else n), None
        else:
            rows = _arr(rows, np.uint32)
            n, ptr = len(rows), (rows.ctypes.data if len(rows) else None)
        out = np.zeros((max(n, 1), 43), dtype=np.uint8)
        check(lib().pm_addresses_text(self._h, ptr, n, out.ctypes.data))
        return [bytes(r[:42]).decode("ascii") for r in out[:n]]

    def keccak256_many(self, messages) -> np.ndarray:
        """pm_keccak256_many: keccak-256 of every message (bytes-like) -> uint8 [n, 32]"""
        msgs = [bytes(m) for m in messages]
        off = np.zeros(len(msgs) + 1, dtype=np.uint32)
        off[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
        buf = np.frombuffer(b"".join(msgs), dtype=np.uint8)
        out = np.zeros((max(len(msgs), 1), 32), dtype=np.uint8)
        check(lib().pm_keccak256_many(self._h, buf.ctypes.data if len(buf) else None, off.ctypes.data, len(msgs), out.ctypes.data))
        return out[:len(msgs)]

    def invite_digests(self, domain_id: int, pool_id: int, rows, nonces, expirations):
        """pm_invite_digests: rows [n], nonces uint8 [n, 32], expirations (seconds) [n] -> (digest, signing hash), uint8 [n, 32] each"""
        rows = _arr(rows, np.uint32)
        n = len(rows)
        nonces = _arr(nonces, np.uint8).reshape(n, 32)
        exp = _arr(expirations, np.uint64)
        assert len(exp) == n
        d, s = np.zeros((max(n, 1), 32), dtype=np.uint8), np.zeros((max(n, 1), 32), dtype=np.uint8)
        check(lib().pm_invite_digests(self._h, domain_id, pool_id, rows.ctypes.data if n else None, n,
                                      nonces.ctypes.data if n else None, exp.ctypes.data if n else None, d.ctypes.data, s.ctypes.data))
        return d[:n], s[:n]

    # ---- request gate (include/pm_engine.h "request gate")
    def ecrecover_many(self, hashes, sigs, want_pub: bool = False):
        """pm_ecrecover_many: hashes uint8 [n, 32], sigs uint8 [n, 65] -> (ok uint8 [n], addresses uint8 [n, 20]) and, when asked,
        the keys uint8 [n, 64]"""
        h = _arr(hashes, np.uint8).reshape(-1, 32)
        g = _arr(sigs, np.uint8).reshape(-1, 65)
        n = len(h)
        assert len(g) == n
        ok, addr = np.zeros(max(n, 1), dtype=np.uint8), np.zeros((max(n, 1), 20), dtype=np.uint8)
        pub = np.zeros((max(n, 1), 64), dtype=np.uint8) if want_pub else None
        check(lib().pm_ecrecover_many(self._h, h.ctypes.data if n else None, g.ctypes.data if n else None, n, addr.ctypes.data,
                                      pub.ctypes.data if want_pub else None, ok.ctypes.data))
        return (ok[:n], addr[:n], pub[:n]) if want_pub else (ok[:n], addr[:n])

    def verify_requests(self, packed):
        """pm_verify_requests: packed = protocol_amd.gate.pack_requests(...) -> (verdicts [n] of RQ_VERDICT, counts uint32 [RQ_N_CODES])"""
        buf, off, sigs, claimed, flags = packed
        n = len(off) - 1
        out, counts = np.zeros(max(n, 1), dtype=RQ_VERDICT), np.zeros(RQ_N_CODES, dtype=np.uint32)
        check(lib().pm_verify_requests(self._h, buf.ctypes.data if len(buf) else None, off.ctypes.data, sigs.ctypes.data if n else None,
                                       claimed.ctypes.data if n else None, None if flags is None else flags.ctypes.data, n,
                                       out.ctypes.data, counts.ctypes.data))
        return out[:n], counts

    # ---- request gate: admission (include/pm_engine.h "request gate: admission")
    def enable_admission(self, on=True) -> None:
        """pm_admission_enable (on: a bool, or ad_debug_prefix_bits(k))"""
        check(lib().pm_admission_enable(self._h, int(on)))

    def admit_requests(self, packed, now_ms: int):
        """pm_admit_requests: packed = protocol_amd.admission.pack_admissions(...) -> (verdicts [n] of RQ_VERDICT, counts uint32
        [AD_N_CODES])"""
        buf, off, sigs, claimed, flags, ts, nbuf, noff = packed
        n = len(off) - 1
        out, counts = np.zeros(max(n, 1), dtype=RQ_VERDICT), np.zeros(AD_N_CODES, dtype=np.uint32)
        check(lib().pm_admit_requests(self._h, int(now_ms), buf.ctypes.data if len(buf) else None, off.ctypes.data,
                                      sigs.ctypes.data if n else None, claimed.ctypes.data if n else None,
                                      None if flags is None else flags.ctypes.data, None if ts is None else ts.ctypes.data,
                                      nbuf.ctypes.data if nbuf is not None and len(nbuf) else None,
                                      None if noff is None else noff.ctypes.data, n, out.ctypes.data, counts.ctypes.data))
        return out[:n], counts

    def admission_rate_get(self, idx):
        """pm_admission_rate_get -> (window_start_ms uint64 [n], count uint32 [n])"""
        ix = _arr(idx, np.uint32)
        n = len(ix)
        win, cnt = np.zeros(max(n, 1), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint32)
        check(lib().pm_admission_rate_get(self._h, ix.ctypes.data if n else None, n, win.ctypes.data, cnt.ctypes.data))
        return win[:n], cnt[:n]

    def admission_rate_set(self, idx, window_start_ms, count) -> None:
        ix, win, cnt = _arr(idx, np.uint32), _arr(window_start_ms, np.uint64), _arr(count, np.uint32)
        assert len(win) == len(ix) == len(cnt)
        n = len(ix)
        check(lib().pm_admission_rate_set(self._h, ix.ctypes.data if n else None, win.ctypes.data if n else None,
                                          cnt.ctypes.data if n else None, n))

    def admission_nonces(self, now_ms: int):
        """pm_admission_nonces -> (n_live at now_ms, n_held)"""
        live, held = C.c_uint32(0), C.c_uint32(0)
        check(lib().pm_admission_nonces(self._h, int(now_ms), C.byref(live), C.byref(held)))
        return live.value, held.value

    def beats_get(self, idx) -> np.ndarray:
        ix = _arr(idx, np.uint32)
        n = len(ix)
        ms = np.zeros(max(n, 1), dtype=np.uint64)
        check(lib().pm_beats_get(self._h, ix.ctypes.data if n else None, n, ms.ctypes.data))
        return ms[:n]

    def beats_set(self, idx, last_beat_ms) -> None:
        ix, ms = _arr(idx, np.uint32), _arr(last_beat_ms, np.uint64)
        assert len(ms) == len(ix)
        n = len(ix)
        check(lib().pm_beats_set(self._h, ix.ctypes.data if n else None, ms.ctypes.data if n else None, n))

    def liveness_sweep_beats(self, now_ms: int, last_beat_ms=None, in_pool_bits=None, apply: bool = False):
        """pm_liveness_sweep_beats -> (n_transitions, census uint32 [NS_N]): pm_liveness_sweep over the later of the device's beat
        column and last_beat_ms (None: the device's column alone)"""
        b = _arr(last_beat_ms, np.uint64) if last_beat_ms is not None else None
        assert b is None or len(b) == self.W
        p = _arr(in_pool_bits, np.uint64) if in_pool_bits is not None else None
        assert p is None or len(p) == (self.W + 63) // 64
        n, census = C.c_uint32(0), np.zeros(NS_N, dtype=np.uint32)
        check(lib().pm_liveness_sweep_beats(self._h, int(now_ms), b.ctypes.data if b is not None and len(b) else None,
                                            p.ctypes.data if p is not None and len(p) else None, int(apply), C.byref(n),
                                            census.ctypes.data))
        return n.value, census

    def debug_address_sorts(self) -> dict:
        """ranks the address book ended on its one-word / all-words sort since creation (pm_debug_carve_prof words 98, 99)"""
        L = lib()
        L.pm_debug_carve_prof.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong), C.c_uint32]
        L.pm_debug_carve_prof.restype = C.c_int32
        out = (C.c_ulonglong * 100)()
        check(L.pm_debug_carve_prof(self._h, out, 100))
        return {"shallow": int(out[98]), "deep": int(out[99])}

    def debug_task_space(self) -> dict:
        """the task index space, the group list and the snapshot buffers (include/pm_engine_debug.h: pm_debug_carve_prof
        words 88..96)"""
        L = lib()
        L.pm_debug_carve_prof.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong), C.c_uint32]
        L.pm_debug_carve_prof.restype = C.c_int32
        out = (C.c_ulonglong * 97)()
        check(L.pm_debug_carve_prof(self._h, out, 97))
        keys = ("t_lo", "t_cap", "T", "t_dead", "regrowths", "compactions", "n_groups", "n_dead_groups", "retired_buffers")
        return dict(zip(keys, (int(v) for v in out[88:97])))

    def debug_row_networks(self, keys, sites, n_per_wave: int, slot_bits: int, ulps: int, upto: int):
        """test hook (include/pm_engine_debug.h): rows from keys[n_waves * n_per_wave] by the insertion and by the sorting
        networks, compared on the device -> (mismatch bits, rows that differ, the networks' rows as u64[n_waves, 64])"""
        import numpy as np
        L = lib()
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        sites = np.ascontiguousarray(sites, dtype=np.uint32)
        assert keys.size % n_per_wave == 0 and sites.size == 1 << slot_bits
        n_waves = keys.size // n_per_wave
        rows = np.zeros((n_waves, 64), dtype=np.uint64)
        mism = (C.c_uint32 * 2)()
        L.pm_debug_row_networks.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                            C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]
        L.pm_debug_row_networks.restype = C.c_int32
        check(L.pm_debug_row_networks(self._h, keys.ctypes.data, sites.ctypes.data, n_waves, n_per_wave, slot_bits, ulps, upto,
                                      rows.ctypes.data, mism))
        return int(mism[0]), int(mism[1]), rows

    def debug_row_certificates(self, keys, sites, n_per_wave: int, slot_bits: int, ulps: int, upto: int, tie_band: float) -> dict:
        """test hook (include/pm_engine_debug.h): three rows per wave from keys[n_waves * n_per_wave] — by the insertion, by the
        networks out of line and by their inline copy — and near_row_finish of each at every K = 1 .. PROP_KMAX ->
        rows u64[n_waves, 3, 64], tau / tau_hi / m1 / m2 u64[n_waves, 3], s1 u32[n_waves, 3], flags u32[n_waves, 3, PROP_KMAX],
        mine u64[n_waves, 3, PROP_KMAX, 64], mismatch (bits, rows that differ) of the first two as debug_row_networks has them"""
        import numpy as np
        L = lib()
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        sites = np.ascontiguousarray(sites, dtype=np.uint32)
        assert keys.size % n_per_wave == 0 and sites.size == 1 << slot_bits
        n_waves = keys.size // n_per_wave
        rows = np.zeros((n_waves, 3, 64), dtype=np.uint64)
        track = np.zeros((n_waves, 3, 5), dtype=np.uint64)
        flags = np.zeros((n_waves, 3, PROP_KMAX), dtype=np.uint32)
        mine = np.zeros((n_waves, 3, PROP_KMAX, 64), dtype=np.uint64)
        mism = (C.c_uint32 * 2)()
        L.pm_debug_row_certificates.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                                C.c_uint32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.POINTER(C.c_uint32)]
        L.pm_debug_row_certificates.restype = C.c_int32
        check(L.pm_debug_row_certificates(self._h, keys.ctypes.data, sites.ctypes.data, n_waves, n_per_wave, slot_bits, ulps, upto,
                                          tie_band, rows.ctypes.data, track.ctypes.data, flags.ctypes.data, mine.ctypes.data, mism))
        return {"rows": rows, "tau": track[:, :, 0].copy(), "tau_hi": track[:, :, 1].copy(), "m1": track[:, :, 2].copy(),
                "m2": track[:, :, 3].copy(), "s1": track[:, :, 4].astype(np.uint32), "flags": flags, "mine": mine,
                "mismatch": (int(mism[0]), int(mism[1]))}

    def debug_distance_keys(self, lat1, lon1, lat2, lon2, slots=None):
        """test hook (include/pm_engine_debug.h): the carve's distance key of the pairs (lat1, lon1) - (lat2, lon2) through the
        device functions the carve runs -> dict of f64 columns (sin_dlat, sin_dlon, cos1, u1[n, 3], cos2, u2[n, 3], hav_a,
        prox_a, candidate_key) + chord (bool: prox_a took the chord form), packed_prox / packed_hav (u64[n, 3]: the key
        packed with the slot at the library's three slot widths)"""
        import numpy as np
        L = lib()
        n = len(lat1)
        if slots is None:
            slots = np.zeros(n)
        inp = np.concatenate([np.asarray(lat1, np.float64), np.asarray(lat2, np.float64), np.asarray(lon1, np.float64),
                              np.asarray(lon2, np.float64), np.asarray(slots, np.float64)])
        assert inp.size == 5 * n
        out = np.zeros((n, 20), dtype=np.float64)
        L.pm_debug_distance_keys.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        L.pm_debug_distance_keys.restype = C.c_int32
        check(L.pm_debug_distance_keys(self._h, inp.ctypes.data, n, 0, out.ctypes.data))
        bits = out.view(np.uint64)
        return {"sin_dlat": out[:, 0].copy(), "sin_dlon": out[:, 1].copy(), "cos1": out[:, 2].copy(), "u1": out[:, 3:6].copy(),
                "cos2": out[:, 6].copy(), "u2": out[:, 7:10].copy(), "hav_a": out[:, 10].copy(), "prox_a": out[:, 11].copy(),
                "chord": out[:, 12] == 1.0, "candidate_key": out[:, 13].copy(), "packed_prox": bits[:, 14:17].copy(),
                "packed_hav": bits[:, 17:20].copy()}

    def debug_candidate_keys(self, lat1, lon1, lat2, lon2) -> "np.ndarray":
        """test hook (pm_debug_distance_keys mode 3): candidate_key's unpacked key of every pair alone, as u64 bit patterns —
        the kernel of debug_distance_keys, one column of its records copied back"""
        import numpy as np
        L = lib()
        n = len(lat1)
        inp = np.concatenate([np.asarray(lat1, np.float64), np.asarray(lat2, np.float64), np.asarray(lon1, np.float64),
                              np.asarray(lon2, np.float64), np.zeros(n)])
        assert inp.size == 5 * n
        out = np.zeros(n, dtype=np.uint64)
        L.pm_debug_distance_keys.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        L.pm_debug_distance_keys.restype = C.c_int32
        check(L.pm_debug_distance_keys(self._h, inp.ctypes.data, n, 3, out.ctypes.data))
        return out

    def debug_first_batch_arm(self):
        """test hook (include/pm_engine_debug.h): the next formation of this engine (carve_variant 3) leaves a snapshot of its
        first batch — candidate list, spatial index, neighbour rows — for debug_first_batch()"""
        L = lib()
        L.pm_debug_first_batch_arm.argtypes = [C.c_void_p]
        L.pm_debug_first_batch_arm.restype = C.c_int32
        check(L.pm_debug_first_batch_arm(self._h))

    def debug_first_batch(self) -> dict:
        """the armed snapshot: FB_HEAD's words by name, every other part of FB_PARTS as a numpy array of its type (`prop` as
        u64[n_seeds, 96])"""
        import numpy as np
        L = lib()
        L.pm_debug_first_batch_get.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.pm_debug_first_batch_get.restype = C.c_int32
        out = {}
        for part, (name, dt) in enumerate(FB_PARTS):
            nb = C.c_uint64(0)
            check(L.pm_debug_first_batch_get(self._h, part, None, 0, C.byref(nb)))
            a = np.zeros(nb.value // np.dtype(dt).itemsize, dtype=dt)
            assert a.nbytes == nb.value, (name, nb.value)
            if a.size:
                check(L.pm_debug_first_batch_get(self._h, part, a.ctypes.data, a.nbytes, C.byref(nb)))
            out[name] = a
        head = out.pop("head")
        assert head.size == len(FB_HEAD)
        out.update({k: int(v) for k, v in zip(FB_HEAD, head) if k})
        out["prop_keys"] = out.pop("prop_keys_lo") | (out.pop("prop_keys_hi") << 32)
        out["prop"] = out["prop"].reshape(-1, PROP_ROW)
        return out

    def debug_sin_band(self, x):
        """test hook (include/pm_engine_debug.h): the carve's sine, sin_band, on the device at each x"""
        import numpy as np
        L = lib()
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.zeros(x.size, dtype=np.float64)
        L.pm_debug_distance_keys.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        L.pm_debug_distance_keys.restype = C.c_int32
        check(L.pm_debug_distance_keys(self._h, x.ctypes.data, x.size, 1, out.ctypes.data))
        return out

    def debug_key_geometry(self) -> dict:
        """the library's key constants (include/pm_engine_debug.h, pm_debug_distance_keys mode 2)"""
        L = lib()
        out = (C.c_double * 8)()
        L.pm_debug_distance_keys.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        L.pm_debug_distance_keys.restype = C.c_int32
        check(L.pm_debug_distance_keys(self._h, None, 0, 2, out))
        return {"chord_min": out[0], "a_max_safe": out[1], "bands": (out[2], out[3], out[4]),
                "slot_bits": (int(out[5]), int(out[6]), int(out[7]))}

    def debug_carve_counters(self) -> dict:
        """how the last carve went (pm_internal.h, pm_debug_carve_prof words 32..45): how its validation launches ended,
        and what the proposer's spatial index did"""
        L = lib()
        L.pm_debug_carve_prof.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong), C.c_uint32]
        L.pm_debug_carve_prof.restype = C.c_int32
        out = (C.c_ulonglong * 98)()
        check(L.pm_debug_carve_prof(self._h, out, 98))
        w = [int(v) for v in out[32:56]]
        return {"why": w[:8], "batches": w[8], "void_launches": w[9], "pruned_batches": w[10], "prune_fallbacks": w[11],
                "cell_g": w[12], "n_indexed": w[13],
                # the streaming carve (carve_variant 0): did the last carve stream, seeds handed to the proposers, rows the
                # validator gave up waiting for, configurations that switched from the index walk to a candidate list,
                # configurations entered with a list, proposer workgroups, launches that gave up (-> batch pipeline),
                # steps that took the exact sweep; times a configuration's outstanding tickets were dropped and issued afresh
                "stream": w[14], "stream_tickets": w[15], "stream_timeouts": w[16], "stream_switches": w[17],
                "stream_listed": w[18], "stream_wgs": w[19], "stream_aborts": w[20], "slow_steps": w[21],
                "stream_pre_used": w[22], "stream_pre_lost": w[23], "stream_refreshes": int(out[97])}

    def debug_prune_mode(self, mode: int):
        """test hook (pm_internal.h): 0 the proposer always sweeps the whole candidate list, 1 it walks the spatial index
        when that pays (default), 2 whenever the carve has an index, 3 = 2 with every seed through the fallback"""
        L = lib()
        L.pm_debug_prune_mode.argtypes = [C.c_void_p, C.c_uint32]
        L.pm_debug_prune_mode.restype = C.c_int32
        check(L.pm_debug_prune_mode(self._h, mode))

    def lookup(self, worker: int) -> Assignment:
        a = Assignment()
        check(lib().pm_lookup_task_for_worker(self._h, worker, C.byref(a)))
        return a
