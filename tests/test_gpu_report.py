"""The diagnostics reports on the GPU (pm_explain_workers, pm_config_report, pm_task_report) against the numpy model of
tests/report_model.py: every reason code, the worker states, both reports after ticks, task positions through insertions,
deletions and uploads, the churn stream with reports between all its calls (the oracle's digests and the delta pushes
unchanged), the refusals, and BASELINE configs[2] at full size."""
import json
import os
import sys

import numpy as np
import pytest

from protocol_amd import engine as E
from protocol_amd import host
from protocol_amd.churn import ChurnStream
from protocol_amd.swarm import baseline_config, make_swarm, wide_config_swarm

import report_model as RM

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from make_golden_churn import CHURN_SEED, CHURN_TICKS_PINNED, CHURN_TICKS_PLANNED, events_digest, sha  # noqa: E402

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "churn_digests.json")))


def model_inputs(sw):
    cfg_rows, alt_rows, req_models = host.pack_configs(sw.configs)
    bits = host.build_model_table(req_models, sw.model_names)
    return host.pack_workers(sw), cfg_rows, alt_rows, bits, len(sw.model_names)


def compat_bits(masks, C):
    return ((masks[:, None] >> np.arange(C, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)


def check_explain_all(eng, sw):
    cols, cfg_rows, alt_rows, bits, n_cls = model_inputs(sw)
    want = RM.why_codes(cols, cfg_rows, alt_rows, bits, n_cls)
    why, state = eng.explain_workers()
    assert why.shape == want.shape
    assert np.array_equal(why, want)
    assert np.array_equal(why == 0, compat_bits(eng.compat_masks(), len(cfg_rows)))
    return why, state


def check_reports(eng, flags, enabled, task_masks, why=None):
    """both reports against the model built from pm_get_groups (which compacts the list)"""
    groups, group_of = RM.groups_of_engine(eng)
    if why is None:
        why, _ = eng.explain_workers()
    _, state = eng.explain_workers()
    assert np.array_equal(state, RM.worker_state(flags, group_of))
    rep = eng.config_report()
    want = RM.config_report(why, flags, group_of, enabled, groups, task_masks)
    assert np.array_equal(rep, want), (rep, want)
    f = np.asarray(flags).astype(np.uint32)
    assert int(rep["why"].sum(axis=1).max()) == int((((f & E.W_HEALTHY) != 0) & ((f & E.W_HAS_P2P) != 0)).sum())
    assert int(rep["groups"].sum()) == len(groups) and int(rep["members"].sum()) == sum(g[1] for g in groups)
    got = eng.task_report()
    for g, w in zip(got, RM.task_report(groups, task_masks, why.shape[1])):
        assert np.array_equal(g, w)
    assert int(got[0].sum()) == sum(1 for g in groups if g[2] >= 0)
    return rep, got


@pytest.mark.parametrize("cfg", [0, 1])
@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_explain_every_row_on_baseline(cfg, seed):
    sw = baseline_config(cfg, seed=seed)
    eng = E.Engine()
    host.load_swarm(eng, sw)
    why, state = check_explain_all(eng, sw)
    assert (state == RM.worker_state(host.worker_flags(sw), np.full(sw.W, -1))).all()
    eng.tick()
    check_reports(eng, host.worker_flags(sw), sw.enabled_mask(), sw.task_masks(), why)
    eng.close()


@pytest.mark.parametrize("C", [1, 33, 63, 64])
def test_explain_and_reports_on_wide_configs(C):
    sw = wide_config_swarm(C, 600, 3000, C)
    eng = E.Engine()
    host.load_swarm(eng, sw)
    why, _ = check_explain_all(eng, sw)
    eng.tick()
    check_reports(eng, host.worker_flags(sw), sw.enabled_mask(), sw.task_masks(), why)
    eng.close()


def hand_rows():
    """(requirement, worker columns) pairs that reach every code, as one table: row i against config i"""
    base = E.W_HAS_SPECS | E.W_HEALTHY | E.W_HAS_P2P
    G = E.W_HAS_GPU
    rows = [  # (requirement, flags, count, mem, model class, cores, ram, storage, code)
        (None, E.W_HEALTHY | E.W_HAS_P2P, 0, 0, 0, 0, 0, 0, RM.OK),                  # no requirements, no specs
        ("ram_mb=1", E.W_HEALTHY | E.W_HAS_P2P, 0, 0, 0, 0, 0, 0, RM.NO_SPECS),
        ("cpu:cores=4", base | E.W_RAM, 0, 0, 0, 0, 10, 0, RM.CPU),                 # no cpu
        ("cpu:cores=4", base | E.W_HAS_CPU | E.W_CPU_CORES, 0, 0, 0, 2, 0, 0, RM.CPU),
        ("ram_mb=100", base | E.W_RAM, 0, 0, 0, 0, 10, 0, RM.RAM),
        ("storage_gb=100", base | E.W_STORAGE, 0, 0, 0, 0, 0, 10, RM.STORAGE),
        ("gpu:count=1", base | E.W_RAM, 0, 0, 0, 0, 10, 0, RM.GPU_NONE),
        ("gpu:count=2", base | G | E.W_GPU_COUNT, 1, 0, 0, 0, 0, 0, RM.GPU_COUNT),
        ("gpu:count=1", base | G | E.W_GPU_MEM, 0, 10, 0, 0, 0, 0, RM.GPU_COUNT),  # count None, required 1
        ("gpu:count=0", base | G | E.W_GPU_MEM, 0, 10, 0, 0, 0, 0, RM.OK),         # count None, required 0
        ("gpu:model=h100", base | G | E.W_GPU_COUNT | E.W_GPU_MODEL, 1, 0, 0, 0, 0, 0, RM.GPU_MODEL),
        ("gpu:memory_mb=100", base | G | E.W_GPU_COUNT | E.W_GPU_MEM, 1, 10, 0, 0, 0, 0, RM.GPU_MEM),
        ("gpu:memory_mb_max=5", base | G | E.W_GPU_COUNT | E.W_GPU_MEM, 1, 10, 0, 0, 0, 0, RM.GPU_MEM),
        ("gpu:total_memory_min=1", base | G | E.W_GPU_COUNT | E.W_GPU_MEM, 65536, 65536, 0, 0, 0, 0, RM.GPU_TOTAL),
        ("gpu:total_memory_max=0", base | G | E.W_GPU_COUNT | E.W_GPU_MEM, 65536, 65536, 0, 0, 0, 0, RM.OK),
        ("gpu:total_memory_max=15", base | G | E.W_GPU_COUNT | E.W_GPU_MEM, 2, 10, 0, 0, 0, 0, RM.GPU_TOTAL),
        ("gpu:count=8;gpu:count=1;gpu:memory_mb=100", base | G | E.W_GPU_COUNT | E.W_GPU_MEM, 1, 10, 0, 0, 0, 0,
         RM.GPU_MEM),                                                                # the largest code over alternatives
        ("gpu:count=1;gpu:model=h100;gpu:count=8", base | G | E.W_GPU_COUNT | E.W_GPU_MODEL, 1, 0, 0, 0, 0, 0,
         RM.GPU_MODEL),
        ("cpu:cores=4;ram_mb=100", base | E.W_HAS_CPU | E.W_CPU_CORES, 0, 0, 0, 8, 0, 0, RM.RAM),  # first failing clause
    ]
    return rows


def test_hand_built_rows_reach_every_code():
    rows = hand_rows()
    n = len(rows)
    cfg_rows, alt_rows, req_models = host.pack_configs([(f"c{i}", 1, 2, r[0]) for i, r in enumerate(rows)])
    bits = host.build_model_table(req_models, ["NVIDIA A100 80GB"])
    col = lambda k: np.array([r[k] for r in rows], dtype=np.uint32)
    cols = dict(flags=col(1), gpu_count=col(2), gpu_mem_mb=col(3), gpu_model_class=col(4), cpu_cores=col(5), ram_mb=col(6),
                storage_gb=col(7), price=np.zeros(n, np.uint32), addr_rank=np.arange(n, dtype=np.uint32),
                lat=np.zeros(n), lon=np.zeros(n))
    eng = E.Engine()
    eng.set_configs(cfg_rows, alt_rows)
    eng.set_model_table(bits, len(req_models), 1)
    eng.upload_workers(cols)
    why, state = eng.explain_workers()
    want = np.array([r[8] for r in rows], dtype=np.uint8)
    assert np.array_equal(np.diagonal(why), want), (np.diagonal(why), want)
    assert set(want.tolist()) == set(range(10))
    assert np.array_equal(why, RM.why_codes(cols, cfg_rows, alt_rows, bits, 1))
    assert np.array_equal(why == 0, compat_bits(eng.compat_masks(), n))
    assert state[0] == E.WS_IDLE and state[1] == E.WS_IDLE
    # a list in any order, with repeats; state for unhealthy / no-p2p rows
    pick = np.array([5, 0, 5, n - 1], dtype=np.uint32)
    w2, s2 = eng.explain_workers(pick)
    assert np.array_equal(w2, why[pick]) and np.array_equal(s2, state[pick])
    eng.on_worker_status(3, int(cols["flags"][3]) & ~E.W_HEALTHY, False)  # pending: not uploaded yet
    cols2 = dict(cols)
    cols2["flags"] = cols["flags"].copy()
    cols2["flags"][4] &= np.uint32(~E.W_HAS_P2P & 0xFFFFFFFF)
    eng.update_workers([4], {k: v[4:5] for k, v in cols2.items()})
    _, s3 = eng.explain_workers([3, 4])
    assert s3.tolist() == [E.WS_UNHEALTHY, E.WS_NO_P2P]
    rep = eng.config_report()
    assert int(rep["why"][3].sum()) == n - 2  # rows 3 and 4 are no longer eligible
    eng.close()


def test_reports_follow_task_positions():
    sw = make_swarm(7, 3000, 4000)
    eng = E.Engine()
    host.load_swarm(eng, sw)
    flags = host.worker_flags(sw)
    masks = sw.task_masks().copy()
    uids = sw.task_uid.copy()
    t_max = int(sw.created_at.max())
    eng.tick()
    check_reports(eng, flags, sw.enabled_mask(), masks)
    rng = np.random.default_rng(7)
    next_uid = 1 << 40
    cap0 = eng.debug_task_space()["t_cap"]
    regrown = False
    for k in range(5):  # insertions in front; the last one overruns the room in front (2 T + 65,536): the space regrows
        n = 400 if k < 3 else 35000
        m = masks[rng.integers(0, len(masks), n)]
        ca = (t_max + 1 + np.arange(n)[::-1]).astype(np.int64)
        u = np.arange(next_uid, next_uid + n, dtype=np.uint64)
        t_max += n
        next_uid += n
        eng.tasks_insert_front(m, ca, u)
        masks, uids = np.concatenate([m, masks]), np.concatenate([u, uids])
        check_reports(eng, flags, sw.enabled_mask(), masks)
        eng.tick()
        check_reports(eng, flags, sw.enabled_mask(), masks)
        regrown |= eng.debug_task_space()["t_cap"] != cap0
    assert regrown
    # deletions: claimed tasks first (their groups dissolve)
    _, groups, _ = eng.get_groups()
    claimed = sorted({int(g["task"]) for g in groups if int(g["task"]) != NONE})[:50]
    gone = np.concatenate([uids[claimed], uids[rng.choice(len(uids), 100, replace=False)]])
    eng.tasks_delete(gone)
    keep = ~np.isin(uids, gone)
    masks, uids = masks[keep], uids[keep]
    check_reports(eng, flags, sw.enabled_mask(), masks)
    eng.tick()
    check_reports(eng, flags, sw.enabled_mask(), masks)
    # a new snapshot: reversed order, half of the tasks
    order = np.arange(len(masks))[::2]
    created = np.arange(len(order), 0, -1).astype(np.int64)
    eng.upload_tasks(masks[order], created, uids[order])
    masks, uids = masks[order], uids[order]
    check_reports(eng, flags, sw.enabled_mask(), masks)
    eng.tick()
    check_reports(eng, flags, sw.enabled_mask(), masks)
    eng.close()


def _stream_model(live, lookup, W, flags, why, enabled, masks):
    """the reports' model from the life-cycle feed (id -> (config, members)) and the published rows, without
    pm_get_groups (it would compact the list and change what the next tick pushes)"""
    group_of = np.full(W, -1, dtype=np.int64)
    groups = []
    for k, (cfg, mem) in enumerate(live.values()):
        group_of[mem] = k
        t = lookup(mem[0]).task
        groups.append((cfg, len(mem), -1 if t == NONE else int(t)))
    return (RM.config_report(why, flags, group_of, enabled, groups, masks), RM.task_report(groups, masks, why.shape[1]),
            RM.worker_state(flags, group_of))


def _churn(with_reports):
    gold = GOLD["churn"]
    assert (gold["seed"], gold["ticks_planned"]) == (CHURN_SEED, CHURN_TICKS_PLANNED)
    eng = E.Engine(group_id_seed=1)
    cs = ChurnStream(CHURN_SEED, CHURN_TICKS_PLANNED)
    sw_all = cs.sw_all
    packed = host.pack_workers(sw_all)
    rows = lambda idx: {k: np.ascontiguousarray(v[idx]) for k, v in packed.items()}
    cfg_rows, alt_rows, req_models = host.pack_configs(sw_all.configs)
    bits = host.build_model_table(req_models, sw_all.model_names)
    why_all = RM.why_codes(packed, cfg_rows, alt_rows, bits, len(sw_all.model_names))
    eng.set_configs(cfg_rows, alt_rows)
    eng.set_model_table(bits, len(req_models), len(sw_all.model_names))
    eng.upload_workers(rows(np.arange(cs.W0)))
    eng.upload_tasks(cs.masks, cs.created, cs.uid)
    enabled = sw_all.enabled_mask()
    eng.set_enabled_mask(enabled)
    eng.enable_group_events()
    flags = packed["flags"].astype(np.int64).copy()
    masks = cs.masks.copy()
    live = {}
    events = []
    n_checked = [0]

    def drain():
        ev = eng.drain_group_events()
        for kind, gid, cfg, mem in ev:
            if kind == 1:
                live[gid] = (cfg, np.array(mem, dtype=np.int64))
            else:
                live.pop(gid)
        events.extend(ev)

    def report(W):
        if not with_reports:
            return
        drain()
        f = flags[:W].astype(np.uint32)
        rep, (run, wrk, alw), state = _stream_model(live, eng.lookup, W, f, why_all[:W], enabled, masks)
        got = eng.config_report()
        assert np.array_equal(got, rep)
        g_run, g_wrk, g_alw = eng.task_report()
        assert np.array_equal(g_run, run) and np.array_equal(g_wrk, wrk) and np.array_equal(g_alw, alw)
        why, st = eng.explain_workers()
        assert np.array_equal(why, why_all[:W]) and np.array_equal(st, state)
        n_checked[0] += 1

    def check(W, g, stats, tag):
        assert stats["n_formed"] == g["n_formed"] and stats["n_groups"] == g["n_groups"], (tag, stats)
        col = np.array([eng.lookup(w).task for w in range(W)], dtype=np.uint32)
        assert sha(col) == g["task_sha256"], f"{tag}: per-worker tasks differ from the oracle"
        drain()
        assert len(events) == g["n_events"] and events_digest(events) == g["events_sha256"], f"{tag}: life-cycle feed"
        events.clear()

    report(cs.W0)
    check(cs.W0, gold["cold"], eng.tick(), "cold")
    report(cs.W0)
    for k in range(CHURN_TICKS_PINNED):
        leave, idx_new, new_tasks = cs.step()
        flags[leave] &= ~E.W_HEALTHY
        eng.on_worker_status_many(leave, flags[leave], np.ones(len(leave), dtype=np.uint32))
        report(cs.W - cs.n_churn)  # status changes still pending upload
        eng.append_workers(rows(idx_new))
        report(cs.W)
        eng.tasks_insert_front(*new_tasks[:3])
        masks = np.concatenate([new_tasks[0], masks])
        report(cs.W)
        check(cs.W, gold["ticks"][k], eng.tick(), f"tick {k}")
        report(cs.W)
    pushes = eng.debug_delta_pushes()
    eng.close()
    return pushes, n_checked[0]


def test_churn_stream_with_reports_between_every_call():
    pushes, n = _churn(True)
    assert n == 2 + 4 * CHURN_TICKS_PINNED
    pushes_plain, _ = _churn(False)
    assert pushes == pushes_plain
    assert pushes >= CHURN_TICKS_PINNED - 2


def test_refusals():
    eng = E.Engine()
    L = E.lib()
    n = np.zeros(1, dtype=np.uint32)
    assert L.pm_config_report(eng._h, None, 0, n.ctypes.data_as(E.C.POINTER(E.C.c_uint32))) == E.PM_ESTATE
    assert L.pm_explain_workers(eng._h, None, 0, None, None) == E.PM_ESTATE
    assert L.pm_task_report(eng._h, None, None, None) == E.PM_ESTATE
    sw = make_swarm(3, 500, 600)
    cfg_rows, alt_rows, req_models = host.pack_configs(sw.configs)
    eng.set_configs(cfg_rows, alt_rows)
    eng.set_model_table(host.build_model_table(req_models, sw.model_names), len(req_models), len(sw.model_names))
    assert L.pm_config_report(eng._h, None, 0, None) == E.PM_ESTATE  # no workers yet
    eng.upload_workers(host.pack_workers(sw))
    assert L.pm_task_report(eng._h, None, None, None) == E.PM_ESTATE  # no tasks yet
    eng.config_report()
    eng.explain_workers([0, 599])
    with pytest.raises(E.EngineError) as ex:
        eng.explain_workers([0, 600])
    assert ex.value.code == E.PM_ERANGE
    out = np.zeros(len(cfg_rows), dtype=E.config_report_dt)
    got = E.C.c_uint32(0)
    assert L.pm_config_report(eng._h, out.ctypes.data, len(cfg_rows) - 1, E.C.byref(got)) == E.PM_ERANGE
    assert got.value == len(cfg_rows)
    eng.upload_tasks(sw.task_masks(), sw.created_at, sw.task_uid)
    eng.set_enabled_mask(sw.enabled_mask())
    eng.task_report()
    eng.dist_configure(0, 1)
    eng.dist_tick_begin()
    assert L.pm_config_report(eng._h, out.ctypes.data, len(out), E.C.byref(got)) == E.PM_ESTATE
    assert L.pm_explain_workers(eng._h, None, 0, None, None) == E.PM_ESTATE
    assert L.pm_task_report(eng._h, None, None, None) == E.PM_ESTATE
    eng.dist_carve_wait()
    eng.dist_match_begin()
    eng.dist_tick_end()
    check_reports(eng, host.worker_flags(sw), sw.enabled_mask(), sw.task_masks())
    eng.close()


def test_config2_at_full_size():
    sw = baseline_config(2, seed=1)
    eng = E.Engine()
    host.load_swarm(eng, sw)
    eng.tick()
    check_reports(eng, host.worker_flags(sw), sw.enabled_mask(), sw.task_masks())
    eng.close()
