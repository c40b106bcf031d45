"""numpy restatement of the diagnostics reports (include/pm_engine.h, pm_explain_workers / pm_config_report /
pm_task_report), on the engine's own packed columns (protocol_amd.host.pack_workers / pack_configs / build_model_table).

  why_codes     the first clause of ComputeSpecs::meets each (worker, configuration) pair fails (PM_WHY_*, node.rs:377-541);
                over GPU alternatives the largest code when every one fails
  worker_state  PM_WS_*: in a group, not Healthy, no p2p id, else idle
  config_report one config_report_dt row per configuration
  task_report   (groups_running, workers_running, groups_allowed) by task position
"""
import numpy as np

from protocol_amd import engine as E

OK, NO_SPECS, CPU, RAM, STORAGE, GPU_NONE, GPU_COUNT, GPU_MODEL, GPU_MEM, GPU_TOTAL = range(10)
NONE = 0xFFFFFFFF


def _alt_codes(w, a, model_bits, words):
    """GpuSpecs::meets (node.rs:445-526) for one alternative over all rows: the first failing clause, 0 if none"""
    f = w["flags"].astype(np.uint32)
    n = len(f)
    code = np.zeros(n, dtype=np.uint8)
    todo = np.ones(n, dtype=bool)

    def fail(cond, c):
        hit = todo & cond
        code[hit] = c
        todo[hit] = False

    af = int(a["flags"])
    cnt = w["gpu_count"].astype(np.uint32)
    mem = w["gpu_mem_mb"].astype(np.uint32)
    cls = w["gpu_model_class"].astype(np.uint32)
    count_some = (f & E.W_GPU_COUNT) != 0
    mem_some = (f & E.W_GPU_MEM) != 0
    if af & E.G_COUNT:
        fail(np.where(count_some, cnt != int(a["count"]), int(a["count"]) > 0), GPU_COUNT)
    if af & E.G_MODEL:
        model_some = (f & E.W_GPU_MODEL) != 0
        row = int(a["model_row"])
        safe = np.where(model_some, cls, 0)
        bit = (model_bits[row * words + (safe >> 5)] >> (safe & 31)) & 1 if words else np.zeros(n, dtype=np.uint32)
        fail(~model_some | (bit == 0), GPU_MODEL)
    if af & E.G_MEM:
        fail(~mem_some | (mem < int(a["memory_mb"])), GPU_MEM)
    if af & E.G_MEM_MIN:
        fail(~mem_some | (mem < int(a["memory_mb_min"])), GPU_MEM)
    if af & E.G_MEM_MAX:
        fail(~mem_some | (mem > int(a["memory_mb_max"])), GPU_MEM)
    total = (cnt.astype(np.uint64) * mem.astype(np.uint64)) & 0xFFFFFFFF   # u32 wrapping product
    both = count_some & mem_some
    if af & E.G_TOT_MIN:
        fail(both & (total < int(a["total_memory_min"])), GPU_TOTAL)
    if af & E.G_TOT_MAX:
        fail(both & (total > int(a["total_memory_max"])), GPU_TOTAL)
    return code


def why_codes(workers: dict, cfg_rows, alt_rows, model_bits=None, n_classes: int = 0) -> np.ndarray:
    """uint8 [W, C]: the PM_WHY_* code of every (worker, configuration) pair"""
    f = np.asarray(workers["flags"]).astype(np.uint32)
    W, C = len(f), len(cfg_rows)
    words = (n_classes + 31) // 32
    bits = np.zeros(1, dtype=np.uint32) if model_bits is None else np.asarray(model_bits, dtype=np.uint32)
    w = {k: np.asarray(v) for k, v in workers.items()}
    out = np.zeros((W, C), dtype=np.uint8)
    for c in range(C):
        cfg = cfg_rows[c]
        cf = int(cfg["flags"])
        if not cf & E.R_HAS_REQ:
            continue                                            # (None, _) => true
        code = np.zeros(W, dtype=np.uint8)
        todo = np.ones(W, dtype=bool)

        def fail(cond, k):
            hit = todo & cond
            code[hit] = k
            todo[hit] = False

        fail((f & E.W_HAS_SPECS) == 0, NO_SPECS)
        if cf & E.R_CPU:
            fail((f & E.W_HAS_CPU) == 0, CPU)
            if cf & E.R_CPU_CORES:
                fail(((f & E.W_CPU_CORES) == 0) | (w["cpu_cores"].astype(np.uint32) < int(cfg["cpu_cores"])), CPU)
        if cf & E.R_RAM:
            fail(((f & E.W_RAM) == 0) | (w["ram_mb"].astype(np.uint32) < int(cfg["ram_mb"])), RAM)
        if cf & E.R_STORAGE:
            fail(((f & E.W_STORAGE) == 0) | (w["storage_gb"].astype(np.uint32) < int(cfg["storage_gb"])), STORAGE)
        n_alt = int(cfg["alt_count"])
        if n_alt:
            fail((f & E.W_HAS_GPU) == 0, GPU_NONE)
            per = np.stack([_alt_codes(w, alt_rows[int(cfg["alt_begin"]) + k], bits, words) for k in range(n_alt)])
            gpu = np.where((per == 0).any(axis=0), 0, per.max(axis=0)).astype(np.uint8)  # the alternative that got furthest
            hit = todo & (gpu != 0)
            code[hit] = gpu[hit]
        out[:, c] = code
    return out


def worker_state(flags, group_of) -> np.ndarray:
    f = np.asarray(flags).astype(np.uint32)
    g = np.asarray(group_of).astype(np.int64)
    s = np.full(len(f), E.WS_IDLE, dtype=np.uint32)
    s[(f & E.W_HAS_P2P) == 0] = E.WS_NO_P2P
    s[(f & E.W_HEALTHY) == 0] = E.WS_UNHEALTHY
    s[g >= 0] = E.WS_IN_GROUP
    return s


def config_report(why, flags, group_of, enabled: int, groups, task_masks) -> np.ndarray:
    """groups: [(config, n_members, task position or -1)] of the live groups; task_masks: the live tasks' masks"""
    W, C = why.shape
    f = np.asarray(flags).astype(np.uint32)
    elig = ((f & E.W_HEALTHY) != 0) & ((f & E.W_HAS_P2P) != 0)
    idle = elig & (np.asarray(group_of) < 0)
    out = np.zeros(C, dtype=E.config_report_dt)
    tm = np.asarray(task_masks, dtype=np.uint64)
    for c in range(C):
        r = out[c]
        r["enabled"] = (int(enabled) >> c) & 1
        counts = np.bincount(why[elig, c], minlength=10)[:10]
        r["why"] = counts
        r["eligible_meets"] = counts[0]
        r["idle_meets"] = int((idle & (why[:, c] == 0)).sum())
        mine = [g for g in groups if g[0] == c]
        r["groups"] = len(mine)
        r["members"] = sum(g[1] for g in mine)
        r["groups_without_task"] = sum(1 for g in mine if g[2] < 0)
        r["tasks_allowing"] = int(((tm >> np.uint64(c)) & np.uint64(1)).sum()) if len(tm) else 0
    return out


def task_report(groups, task_masks, n_cfgs: int):
    T = len(task_masks)
    running = np.zeros(T, dtype=np.uint32)
    workers = np.zeros(T, dtype=np.uint32)
    per_cfg = np.zeros(64, dtype=np.int64)
    for cfg, n, t in groups:
        per_cfg[cfg] += 1
        if t >= 0:
            running[t] += 1
            workers[t] += n
    tm = np.asarray(task_masks, dtype=np.uint64)
    allowed = np.zeros(T, dtype=np.int64)
    for c in range(n_cfgs):
        if per_cfg[c]:
            allowed += ((tm >> np.uint64(c)) & np.uint64(1)).astype(np.int64) * per_cfg[c]
    return running, workers, allowed.astype(np.uint32)


def groups_of_engine(eng):
    """[(config, n_members, task position or -1)] and group_of [W] from pm_get_groups (compacts the engine's list)"""
    group_of, groups, _members = eng.get_groups()
    out = [(int(g["config"]), int(g["n_members"]), -1 if int(g["task"]) == NONE else int(g["task"])) for g in groups]
    return out, np.asarray(group_of)
