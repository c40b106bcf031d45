"""The rollout ledger on the GPU (pm_rollout_* of include/pm_engine.h, kernels in pm_rollout.inc) against the model of
tests/rollout_model.py, which tests/test_rollout_model.py holds to the reference and to the named cases: every named case through
the C ABI, seeded swarms behind a real pm_tick at every tile edge of the scan and the sort, the key edges of the 64-bit sort, the
last-wins scatter, the life cycle, every error, what the ledger leaves alone, and determinism."""
import os
import re

import numpy as np
import pytest

from protocol_amd import build as B
from protocol_amd import engine as E
from protocol_amd import host
from protocol_amd.churn import ChurnStream
from protocol_amd.swarm import make_swarm
from helpers import engine_groups

import rollout_cases as RC
import rollout_model as M

pytestmark = pytest.mark.gpu
EINVAL, ESTATE, ERANGE = -1, -4, -5
ON = E.W_HEALTHY | E.W_HAS_P2P
ALL = (1 << M.RO_N) - 1


def _device_constants():
    """the tile sizes the scan and the sort work in, read from the device source: a change there moves the swarm sizes below"""
    dev = open(os.path.join(B.CSRC, "pm_device.h")).read()
    chunk = int(re.search(r"\bPM_RO_CHUNK\s*=\s*(\d+)", dev).group(1))
    kernels = open(os.path.join(B.CSRC, "pm_metrics.inc")).read()
    scan = kernels[kernels.index("void mx_scan_kernel("):kernels.index("void mx_copy_kernel(")]
    tile = int(re.search(r"base \+= (\d+)u", scan).group(1))
    ro = open(os.path.join(B.CSRC, "pm_rollout.inc")).read()
    block = {int(x) for x in re.findall(r"__launch_bounds__\((\d+)\)", ro)}
    return chunk, tile, block


RO_CHUNK, SCAN_TILE, BLOCKS = _device_constants()
SWARM_W = sorted({1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, RO_CHUNK + 1, SCAN_TILE + 1} | {b + 1 for b in BLOCKS})


def _cols(n, flags=ON):
    z = np.zeros(n, dtype=np.uint32)
    return dict(flags=np.full(n, flags, dtype=np.uint32), gpu_count=z, gpu_mem_mb=z, gpu_model_class=z, cpu_cores=z, ram_mb=z,
                storage_gb=z, price=z, lat=np.zeros(n), lon=np.zeros(n))


def _code(call):
    with pytest.raises(E.EngineError) as ei:
        call()
    return ei.value.code


def _reports(rows):
    """[(worker, state, uid)] -> ro_report_dt"""
    out = np.zeros(len(rows), dtype=E.ro_report_dt)
    for k, (w, st, uid) in enumerate(rows):
        out[k] = (w, st, uid)
    return out


def _reads(eng):
    """the four reads as the model's tuples (padding must be zero)"""
    s = eng.rollout_summary()
    t, g, w = eng.rollout_tasks(), eng.rollout_groups(), eng.rollout_workers(ALL)
    assert not t["_pad"].any() and not w["_pad"].any() and not w["_pad2"].any()
    return dict(
        summary=(tuple(s["by_class"].tolist()), tuple(s["by_state"].tolist()), int(s["groups_with_task"]),
                 int(s["groups_converged"]), int(s["distinct_uids"])),
        tasks=[(int(r["uid"]), int(r["task"]), int(r["groups"]), int(r["groups_converged"]), int(r["assigned"]),
                int(r["converged"]), tuple(r["reporters"].tolist())) for r in t],
        groups=[(int(r["group_id"]), int(r["slot"]), int(r["config"]), int(r["task"]), int(r["size"]), tuple(r["same"].tolist()),
                 int(r["other"]), int(r["silent"])) for r in g],
        workers=[(int(r["worker"]), int(r["group_slot"]), int(r["uid"]), int(r["cls"]), int(r["state"])) for r in w])


def _want(eng, W, task_uids, led):
    """the model over the engine's own groups (pm_get_groups) and the current task ids"""
    group_of, _, _ = eng.get_groups()
    return M.read(W, group_of, engine_groups(eng), task_uids, led)


def _check(eng, W, task_uids, led, tag=""):
    got, want = _reads(eng), _want(eng, W, task_uids, led)
    for k in ("summary", "tasks", "groups", "workers"):
        assert got[k] == want[k], (tag, k)
    uid, st = eng.rollout_get()
    assert list(zip(uid.tolist(), st.tolist())) == led.get(range(W)), tag
    for mask in (1 << M.CONVERGED, (1 << M.SILENT) | (1 << M.STRAY)):
        sub = eng.rollout_workers(mask)
        assert sub["worker"].tolist() == [w[0] for w in want["workers"] if (mask >> w[3]) & 1], (tag, mask)
    return want


# ------------------------------------------------------------------ the named cases

def _case_engine(case):
    eng = E.Engine(group_id_seed=3)
    cfg_rows, alt_rows, _ = host.pack_configs([("any", 1, 8, None)])
    eng.set_configs(cfg_rows, alt_rows)
    eng.upload_workers(_cols(case["W"]))
    T = len(case["tasks"])
    eng.upload_tasks(np.full(T, 1, dtype=np.uint64), np.arange(T, 0, -1).astype(np.int64), np.array(case["tasks"], dtype=np.uint64))
    run = RC.Run(case)
    g = np.zeros(len(run.groups), dtype=E.group_dt)
    members = []
    for k, (gid, cfg, mem, t) in enumerate(run.groups):
        g[k] = (gid, cfg, len(mem), len(members), M.NONE if t < 0 else t)
        members += mem
    eng.adopt_groups(g, np.array(members, dtype=np.uint32), 99)
    eng.rollout_enable(True)
    return eng, run


@pytest.mark.parametrize("per_call", [False, True], ids=["one_batch_per_step", "one_report_per_call"])
@pytest.mark.parametrize("case", RC.CASES, ids=[c["name"] for c in RC.CASES])
def test_named_cases_through_the_c_abi(case, per_call):
    eng, run = _case_engine(case)
    for step in case["steps"]:
        run.apply(step)
        kind, arg = step
        if kind == "report":
            reps = RC.reports_of(arg, host.task_state)                      # the states through pm_host_task_state
            assert reps == RC.reports_of(arg)
            if per_call:
                for r in reps:
                    eng.rollout_ingest(_reports([r]))
            else:
                eng.rollout_ingest(_reports(reps))
        elif kind == "delete":
            eng.tasks_delete(np.array(arg, dtype=np.uint64))
        elif kind == "dead":
            eng.on_worker_status(arg, 0, True)
        assert engine_groups(eng) == [(gid, cfg, mem, t) for gid, cfg, mem, t in run.group_list()], step
        _check(eng, case["W"], run.task_uids(), run.led, step)
    want = _check(eng, case["W"], run.task_uids(), run.led, "end")
    assert [w[3] for w in want["workers"]] == case["classes"] and want["summary"][3] == case["converged"]
    eng.close()


# ------------------------------------------------------------------ seeded swarms behind a real tick

def _swarm_reports(rng, W, groups, task_uids):
    """a rollout in flight: most groups converged or nearly, some members behind, on another task, on a task nobody has, silent;
    some free workers still report"""
    claimed = {}
    for _gid, _cfg, mem, t in groups:
        whole = rng.random() < 0.4
        for w in mem:
            claimed[w] = (int(task_uids[t]) if t >= 0 else None, whole)
    reps = []
    for w in range(W):
        uid, whole = claimed.get(w, (None, False))
        r = rng.random()
        if uid is not None and (whole or r < 0.5):
            reps.append((w, M.RUNNING, uid))
        elif uid is not None and r < 0.65:
            reps.append((w, int(rng.integers(0, M.TS_N)), uid))
        elif r < (0.8 if uid is not None else 0.3) and len(task_uids):
            reps.append((w, int(rng.integers(0, M.TS_N)), int(task_uids[rng.integers(0, len(task_uids))])))
        elif r < (0.9 if uid is not None else 0.5):
            reps.append((w, int(rng.integers(0, M.TS_N)), int(rng.integers(1, 1 << 62)) << int(rng.integers(0, 2))))
    return reps


@pytest.mark.parametrize("W", SWARM_W)
def test_seeded_swarms_behind_a_real_tick(W):
    sw = make_swarm(100 + W, 24, W)
    eng = E.Engine(group_id_seed=7)
    host.load_swarm(eng, sw)
    eng.rollout_enable(True)
    led = M.Ledger()
    uids = sw.task_uid.tolist()
    _check(eng, W, uids, led, "before the tick")
    eng.tick()
    groups = engine_groups(eng)
    rng = np.random.default_rng(W)
    reps = _swarm_reports(rng, W, groups, uids)
    eng.rollout_ingest(_reports(reps))
    led.ingest(reps)
    want = _check(eng, W, uids, led, "after the tick")
    if W >= 255:
        assert want["summary"][2] > 0 and want["summary"][3] > 0                               # groups with a task, converged ones
    if W >= 1023:
        assert all(want["summary"][0])                                                         # every class
    again = _swarm_reports(rng, W, groups, uids)[::3]                      # a second wave over a third of the rows
    eng.rollout_ingest(_reports(again))
    led.ingest(again)
    _check(eng, W, uids, led, "second wave")
    eng.close()


# ------------------------------------------------------------------ key edges of the sort

def _plain(W, task_uids=(), group_size=0):
    """W plain workers, the ledger on; with group_size, adopted groups of that size over the first tasks (group k claims task k)"""
    eng = E.Engine(group_id_seed=3)
    cfg_rows, alt_rows, _ = host.pack_configs([("any", 1, 8, None)])
    eng.set_configs(cfg_rows, alt_rows)
    eng.upload_workers(_cols(W))
    T = len(task_uids)
    eng.upload_tasks(np.full(T, 1, dtype=np.uint64), np.arange(T, 0, -1).astype(np.int64), np.array(task_uids, dtype=np.uint64))
    if group_size:
        n = min(T, W // group_size)
        g = np.zeros(n, dtype=E.group_dt)
        for k in range(n):
            g[k] = (0x9000 + k, 0, group_size, k * group_size, k)
        eng.adopt_groups(g, np.arange(n * group_size, dtype=np.uint32), 5)
    eng.rollout_enable(True)
    return eng


def _ingest_and_check(eng, W, uids, reps, tag):
    led = M.Ledger()
    eng.rollout_ingest(_reports(reps))
    led.ingest(reps)
    return _check(eng, W, list(uids), led, tag)


W_SORT = 2 * RO_CHUNK + 77


def test_sort_one_id_everywhere_is_a_single_run_across_every_chunk():
    uid = 0x0123456789ABCDEF
    eng = _plain(W_SORT, [uid], group_size=4)
    want = _ingest_and_check(eng, W_SORT, [uid], [(w, w % M.TS_N, uid) for w in range(W_SORT)], "one id")
    assert len(want["tasks"]) == 1 and sum(want["tasks"][0][6]) == W_SORT
    eng.close()


def test_sort_all_ids_distinct():
    rng = np.random.default_rng(5)
    ids = rng.permutation(W_SORT).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)           # (wraps: distinct, every byte busy)
    eng = _plain(W_SORT, ids[:8].tolist(), group_size=2)
    want = _ingest_and_check(eng, W_SORT, ids[:8].tolist(), [(w, M.RUNNING, int(ids[w])) for w in range(W_SORT)], "distinct")
    assert len(want["tasks"]) == W_SORT
    eng.close()


@pytest.mark.parametrize("k", range(8))
def test_sort_ids_that_differ_only_in_byte(k):
    """256 ids that differ in byte k alone, dealt in a scrambled order over more than one chunk: a pass that skipped byte k would
    leave them unsorted and split their runs"""
    W = RO_CHUNK + 300
    base = 0x5555555555555555 & ~(0xFF << (8 * k))
    rng = np.random.default_rng(k)
    digit = rng.integers(0, 256, W)
    ids = [base | (int(d) << (8 * k)) for d in digit]
    tasks = [base | (d << (8 * k)) for d in (0, 1, 128, 255)]
    eng = _plain(W, tasks, group_size=3)
    want = _ingest_and_check(eng, W, tasks, [(w, int(rng.integers(0, M.TS_N)), ids[w]) for w in range(W)], k)
    assert len(want["tasks"]) == len(set(digit.tolist()) | {0, 1, 128, 255})
    eng.close()


def test_sort_extreme_ids_and_adjacent_claimed_and_reported():
    """0, 0xFFFFFFFF, 2^63, 2^64 - 1; a claimed id nobody reports (1000) next to a reported id nobody claims (1001)"""
    tasks = [0, 0xFFFFFFFF, 1 << 63, M.ALL_ONES, 1000]
    W = 40
    eng = _plain(W, tasks, group_size=2)                                   # groups 0..4 over workers 0..9
    reps = [(w, M.RUNNING, tasks[w // 2]) for w in range(8)]              # the first four groups report their own ids
    reps += [(w, M.RUNNING, 1001) for w in range(10, 14)]                  # group 4 (claims 1000) stays silent
    reps += [(20, M.FAILED, 0), (21, M.PAUSED, 0xFFFFFFFF), (22, M.PENDING, 1 << 63), (23, M.UNKNOWN, M.ALL_ONES),
             (24, M.RUNNING, 0x100000000), (25, M.RUNNING, (1 << 63) - 1), (26, M.RUNNING, M.ALL_ONES - 1)]
    want = _ingest_and_check(eng, W, tasks, reps, "extremes")
    rows = {r[0]: r for r in want["tasks"]}
    assert rows[1000][2] == 1 and sum(rows[1000][6]) == 0 and rows[1001][2] == 0 and sum(rows[1001][6]) == 4
    assert rows[M.ALL_ONES][1] == M.NONE and rows[M.ALL_ONES][5] == 0 and rows[0][1] == 0 and rows[1 << 63][3] == 1
    eng.close()


# ------------------------------------------------------------------ last wins

@pytest.mark.parametrize("n", [2, 65, 257, 1025])
def test_last_report_of_a_worker_wins(n):
    W = 1100
    eng = _plain(W)
    led = M.Ledger()
    for order in ("set_set", "set_clear", "clear_set"):
        first = (7, M.TS_NONE, 0) if order == "clear_set" else (7, M.PENDING, 111)
        last = (7, M.TS_NONE, 0) if order == "set_clear" else (7, M.RUNNING, 222)
        mid = [(8 + (i % (W - 8)), i % M.TS_N, 1000 + i) for i in range(n - 2)]
        reps = [first] + mid + [last]
        assert len(reps) == n
        eng.rollout_ingest(_reports(reps))
        led.ingest(reps)
        uid, st = eng.rollout_get()
        assert list(zip(uid.tolist(), st.tolist())) == led.get(range(W)), order
        assert led.get([7]) == [(0, M.TS_NONE) if order == "set_clear" else (222, M.RUNNING)]
    # every report names one worker: the last of them stands
    reps = [(9, i % M.TS_N, i) for i in range(n)]
    eng.rollout_ingest(_reports(reps))
    uid, st = eng.rollout_get([9])
    assert (int(uid[0]), int(st[0])) == (n - 1, (n - 1) % M.TS_N)
    eng.close()


# ------------------------------------------------------------------ life cycle

def _churn_engine(seed, W0=220):
    cs = ChurnStream(seed, 3, W0=W0, n_churn=12, n_new=10, T0=40)
    sw = cs.sw_all
    packed = host.pack_workers(sw)
    eng = E.Engine(group_id_seed=1)
    cfg_rows, alt_rows, req_models = host.pack_configs(sw.configs)
    eng.set_configs(cfg_rows, alt_rows)
    eng.set_model_table(host.build_model_table(req_models, sw.model_names), len(req_models), len(sw.model_names))
    eng.upload_workers({k: np.ascontiguousarray(v[:cs.W0]) for k, v in packed.items()})
    eng.upload_tasks(cs.masks, cs.created, cs.uid)
    eng.set_enabled_mask(sw.enabled_mask())
    return cs, packed, eng


def test_reads_follow_the_life_cycle():
    cs, packed, eng = _churn_engine(3)
    pick = lambda idx: {k: np.ascontiguousarray(v[idx]) for k, v in packed.items()}
    uids = cs.uid.tolist()
    eng.rollout_enable(True)
    led = M.Ledger()
    rng = np.random.default_rng(11)
    eng.tick()

    def wave(tag):
        reps = _swarm_reports(rng, cs.W, engine_groups(eng), uids)
        eng.rollout_ingest(_reports(reps))
        led.ingest(reps)
        return _check(eng, cs.W, uids, led, tag)

    assert wave("after a tick")["summary"][2] > 0
    for k in range(2):
        leave, idx_new, new_tasks = cs.step()
        eng.on_worker_status_many(leave, np.zeros(len(leave), dtype=np.uint32), np.ones(len(leave), dtype=np.uint32))
        _check(eng, cs.W - len(idx_new), uids, led, "dead workers: their rows stay")
        eng.append_workers(pick(idx_new))
        assert led.get(idx_new.tolist()) == [(0, M.TS_NONE)] * len(idx_new)
        _check(eng, cs.W, uids, led, "appended rows start empty")
        before = eng.rollout_get()
        eng.tasks_insert_front(*new_tasks[:3])
        uids = new_tasks[2].tolist() + uids
        after = eng.rollout_get()
        assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
        _check(eng, cs.W, uids, led, "insert_front: positions move, rows do not")
        eng.tick()
        wave(f"churn {k}")
    # a reported task goes: its groups dissolve, its reporters stay
    want = _check(eng, cs.W, uids, led, "before the delete")
    victim = max((r for r in want["tasks"] if r[2]), key=lambda r: sum(r[6]))[0]
    eng.tasks_delete(np.array([victim], dtype=np.uint64))
    uids.remove(victim)
    want = _check(eng, cs.W, uids, led, "after pm_tasks_delete")
    row = [r for r in want["tasks"] if r[0] == victim][0]
    assert row[1] == M.NONE and row[2] == 0 and sum(row[6]) > 0
    slot = want["groups"][0][1]
    eng.dissolve_group(slot)
    _check(eng, cs.W, uids, led, "after pm_dissolve_group")
    eng.close()


def test_reads_after_a_solo_merge_and_both_uploads():
    W = 130
    eng = E.Engine(group_id_seed=5)
    cfg_rows, alt_rows, _ = host.pack_configs([("trio", 1, 3, None)])
    eng.set_configs(cfg_rows, alt_rows)
    eng.upload_workers(_cols(W))
    uids = [101, 102]
    eng.upload_tasks(np.array([1, 1], dtype=np.uint64), np.array([5, 4], dtype=np.int64), np.array(uids, dtype=np.uint64))
    g = np.zeros(W, dtype=E.group_dt)
    for i in range(W):
        g[i] = (0x7000 + i, 0, 1, i, M.NONE)
    eng.adopt_groups(g, np.arange(W, dtype=np.uint32), 77)
    eng.rollout_enable(True)
    led = M.Ledger()
    reps = [(w, M.RUNNING if w % 5 else M.PULLING, uids[w % 2]) for w in range(W)]
    eng.rollout_ingest(_reports(reps))
    led.ingest(reps)
    assert _check(eng, W, uids, led, "adopted solos without a task")["summary"][0][M.STRAY] == W
    stats = eng.tick()
    assert stats["n_merged"] > 0
    want = _check(eng, W, uids, led, "after the solo merge")
    assert want["summary"][2] > 0 and want["summary"][0][M.CONVERGED] > 0
    eng.upload_workers(_cols(W + 40), keep_groups=True)
    _check(eng, W + 40, uids, led, "upload keeping the groups: the rows stay, the new ones are empty")
    eng.upload_workers(_cols(W + 40), keep_groups=False)
    led.clear()
    want = _check(eng, W + 40, uids, led, "upload dropping the groups: every row empty")
    assert want["summary"][0][M.IDLE] == W + 40 and not want["tasks"]
    eng.rollout_ingest(_reports([(W + 39, M.FAILED, 5)]))
    eng.rollout_enable(True)                                                # again: empties
    _check(eng, W + 40, uids, led, "enabled again")
    eng.close()


# ------------------------------------------------------------------ errors

def test_errors_leave_the_ledger_as_it_was():
    W = 50
    uids = [11, 12, 13]
    eng = _plain(W, uids, group_size=3)
    L, h = E.lib(), eng._h
    reps = [(w, w % M.TS_N, uids[w % 3]) for w in range(0, W, 2)]
    eng.rollout_ingest(_reports(reps))
    before = eng.rollout_get()

    def unchanged():
        now = eng.rollout_get()
        assert now[0].tobytes() == before[0].tobytes() and now[1].tobytes() == before[1].tobytes()

    good = [(1, M.RUNNING, 5), (3, M.RUNNING, 6)]
    assert _code(lambda: eng.rollout_ingest(_reports(good + [(W, M.RUNNING, 1)]))) == ERANGE
    assert _code(lambda: eng.rollout_ingest(_reports(good + [(2, M.TS_N, 1)]))) == EINVAL
    assert _code(lambda: eng.rollout_ingest(_reports(good + [(2, 254, 1)]))) == EINVAL
    assert _code(lambda: eng.rollout_ingest(_reports(good + [(2, 256 + M.RUNNING, 1)]))) == EINVAL
    assert L.pm_rollout_ingest(h, None, 3) == EINVAL and L.pm_rollout_ingest(None, None, 0) == EINVAL
    assert L.pm_rollout_get(h, None, 2, None, None) == EINVAL
    assert _code(lambda: eng.rollout_get([0, W])) == ERANGE
    assert L.pm_rollout_summary(h, None) == EINVAL
    n = E.C.c_uint32(77)
    assert L.pm_rollout_tasks(h, None, 0, None) == EINVAL and L.pm_rollout_groups(h, None, 0, None) == EINVAL
    assert L.pm_rollout_workers(h, ALL, None, 0, None) == EINVAL
    for mask in (0, 1 << M.RO_N, ALL | (1 << 31)):
        assert L.pm_rollout_workers(h, mask, None, 0, E.C.byref(n)) == EINVAL
    unchanged()
    # the size query, a short buffer, a NULL buffer: *n set, nothing copied
    tasks, groups, workers = eng.rollout_tasks(), eng.rollout_groups(), eng.rollout_workers(ALL)
    assert len(tasks) and len(groups) and len(workers) == W
    for call, rows in ((lambda p, cap: L.pm_rollout_tasks(h, p, cap, E.C.byref(n)), tasks),
                       (lambda p, cap: L.pm_rollout_groups(h, p, cap, E.C.byref(n)), groups),
                       (lambda p, cap: L.pm_rollout_workers(h, ALL, p, cap, E.C.byref(n)), workers)):
        n.value = 77
        assert call(None, 0) == ERANGE and n.value == len(rows)
        buf = np.zeros(len(rows), dtype=rows.dtype)
        n.value = 77
        assert call(buf.ctypes.data, len(rows) - 1) == ERANGE and n.value == len(rows) and not buf.view(np.uint8).any()
        assert call(None, 1 << 20) == ERANGE
        assert call(buf.ctypes.data, len(rows)) == 0 and buf.tobytes() == rows.tobytes()   # reading consumes nothing
    unchanged()
    # a stepwise tick in progress
    eng.dist_configure(0, 1)
    eng.dist_tick_begin()
    for call in (lambda: eng.rollout_ingest(_reports(good)), lambda: eng.rollout_get([0]), eng.rollout_summary, eng.rollout_tasks,
                 eng.rollout_groups, eng.rollout_workers, lambda: eng.rollout_enable(True)):
        assert _code(call) == ESTATE
    eng.dist_carve_wait()
    eng.dist_match_begin()
    eng.dist_tick_end()
    unchanged()
    # a multi-GPU engine cannot be configured while the ledger is on, nor the ledger switched on in one
    assert _code(lambda: eng.dist_configure(0, 2, np.zeros(W, dtype=np.uint8))) == ESTATE
    unchanged()
    eng.rollout_enable(False)
    for call in (lambda: eng.rollout_ingest(_reports(good)), lambda: eng.rollout_get([0]), eng.rollout_summary, eng.rollout_tasks,
                 eng.rollout_groups, eng.rollout_workers):
        assert _code(call) == ESTATE
    eng.dist_configure(0, 2, np.zeros(W, dtype=np.uint8))
    assert _code(lambda: eng.rollout_enable(True)) == ESTATE
    eng.dist_configure(0, 1)
    eng.rollout_enable(True)
    # a task table without ids: the ingest and the get go on, the four reads do not
    eng.reset_groups()
    eng.upload_tasks(np.full(2, 1, dtype=np.uint64), np.array([2, 1], dtype=np.int64), None)
    eng.rollout_ingest(_reports(good))
    assert eng.rollout_get([1, 3])[0].tolist() == [5, 6]
    for call in (eng.rollout_summary, eng.rollout_tasks, eng.rollout_groups, eng.rollout_workers):
        assert _code(call) == ESTATE
    assert eng.rollout_get([1, 3])[0].tolist() == [5, 6]
    eng.close()
    # no workers uploaded
    eng = E.Engine()
    eng.rollout_enable(True)
    for call in (lambda: eng.rollout_ingest(_reports([])), lambda: eng.rollout_get([]), eng.rollout_summary, eng.rollout_tasks,
                 eng.rollout_groups, eng.rollout_workers):
        assert _code(call) == ESTATE
    eng.close()


# ------------------------------------------------------------------ what the ledger leaves alone, determinism

def test_the_ledger_leaves_the_tick_alone():
    """the same churn with the ledger on (ingests and all four reads between the ticks) and off: groups, published table, group
    events and change feed word for word"""
    (ca, pa, a), (cb, pb, b) = _churn_engine(2, W0=600), _churn_engine(2, W0=600)
    for eng in (a, b):
        eng.enable_group_events(True)
        eng.enable_assignment_changes(True)
    a.rollout_enable(True)
    rng = np.random.default_rng(1)
    uids = ca.uid.tolist()

    seen = [[]]                                                             # the groups as `same` last saw them on both sides

    def feed():                                                             # (pm_get_groups compacts the list: not called here)
        reps = _swarm_reports(rng, ca.W, seen[0], uids)
        a.rollout_ingest(_reports(reps))
        a.rollout_summary(), a.rollout_tasks(), a.rollout_groups(), a.rollout_workers(ALL)

    def same(tag):
        seen[0] = engine_groups(a)
        assert seen[0] == engine_groups(b), tag
        assert a.drain_group_events() == b.drain_group_events(), tag
        ra, rb = a.drain_assignment_changes(), b.drain_assignment_changes()
        assert ra[0].tobytes() == rb[0].tobytes() and ra[1].tobytes() == rb[1].tobytes() and ra[2] == rb[2], tag
        for w in range(ca.W):
            x, y = a.lookup(w), b.lookup(w)
            assert (x.task, x.group_slot, x.group_index, x.group_size, x.next_worker, x.group_id) == \
                   (y.task, y.group_slot, y.group_index, y.group_size, y.next_worker, y.group_id), (tag, w)

    feed()
    sa, sb = a.tick(), b.tick()
    counters = ("n_groups", "n_formed", "n_merged")
    assert {c: sa[c] for c in counters} == {c: sb[c] for c in counters}
    feed()
    same("first tick")
    for k in range(3):
        (la, ia, ta), (lb, ib, tb) = ca.step()[:3], cb.step()[:3]
        for eng, cs, packed, leave, idx_new, new_tasks in ((a, ca, pa, la, ia, ta), (b, cb, pb, lb, ib, tb)):
            eng.on_worker_status_many(leave, np.zeros(len(leave), dtype=np.uint32), np.ones(len(leave), dtype=np.uint32))
            eng.append_workers({kk: np.ascontiguousarray(v[idx_new]) for kk, v in packed.items()})
            eng.tasks_insert_front(*new_tasks[:3])
            if eng is a:
                uids = new_tasks[2].tolist() + uids
                feed()
        sa, sb = a.tick(), b.tick()
        assert {c: sa[c] for c in counters} == {c: sb[c] for c in counters}, k
        feed()
        same(k)
    a.close(), b.close()


def test_reads_are_deterministic_and_batching_does_not_matter():
    W = 2 * RO_CHUNK + 513
    sw = make_swarm(9, 24, W)
    engines = []
    rng = np.random.default_rng(4)
    reps = None
    for split in (1, 7, 300):
        eng = E.Engine(group_id_seed=7)
        host.load_swarm(eng, sw)
        eng.rollout_enable(True)
        eng.tick()
        if reps is None:
            reps = _swarm_reports(rng, W, engine_groups(eng), sw.task_uid.tolist())
            reps += [(w, M.FAILED, 77) for w in range(0, W, 9)]             # rows named twice
        r = _reports(reps)
        for part in np.array_split(r, split):
            eng.rollout_ingest(part)
        engines.append(eng)

    def image(eng):
        return b"".join(np.asarray(x).tobytes() for x in (eng.rollout_summary(), eng.rollout_tasks(), eng.rollout_groups(),
                                                          eng.rollout_workers(ALL), *eng.rollout_get()))

    first = image(engines[0])
    assert image(engines[0]) == first                                       # the same state read twice
    for eng in engines[1:]:
        assert image(eng) == first
    for eng in engines:
        eng.close()
