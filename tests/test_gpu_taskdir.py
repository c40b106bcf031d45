"""The task directory on the GPU (pm_task_directory of include/pm_engine.h, kernels in pm_taskdir.inc) against the model of
tests/taskdir_model.py, which tests/test_taskdir_model.py holds to the definitions: the named cases through the C ABI, tables at
every edge of the live bitmap, the workgroup, the radix chunk and the scan tile, tombstones, insertions in front, a rebuild of the
index space, a family behind a real pm_tick, windows, rollout on and off, every error, what the call leaves alone, and
determinism.  Every comparison is exact: every listed row and every counter of every query is compared with the model, which is
fed from the engine's other reads (pm_get_groups, pm_rollout_get) and the caller's own task list, and every row and total is
cross-checked against pm_task_report, pm_rollout_tasks and pm_config_report taken at the same moment."""
import gc
import os
import re

import numpy as np
import pytest

from protocol_amd import build as B
from protocol_amd import engine as E
from protocol_amd import host
from protocol_amd.churn import ChurnStream
from helpers import engine_groups

import taskdir_cases as TC
import taskdir_model as M

pytestmark = pytest.mark.gpu
EINVAL, ESTATE, ERANGE = -1, -4, -5
ON = E.W_HEALTHY | E.W_HAS_P2P
FIELDS = ("config_mask", "serve_mask", "rollout_mask", "workers_min", "workers_max", "order", "offset", "limit")


def _device_constants():
    """the sizes the passes, the sort and the scan work in, read from the device source: a change there moves the sizes below"""
    dev = open(os.path.join(B.CSRC, "pm_device.h")).read()
    chunk = int(re.search(r"\bPM_RO_CHUNK\s*=\s*(\d+)", dev).group(1))
    kernels = open(os.path.join(B.CSRC, "pm_metrics.inc")).read()
    scan = kernels[kernels.index("void mx_scan_kernel("):kernels.index("void mx_copy_kernel(")]
    tile = int(re.search(r"base \+= (\d+)u", scan).group(1))
    src = open(os.path.join(B.CSRC, "pm_taskdir.inc")).read()
    block = {int(x) for x in re.findall(r"__launch_bounds__\((\d+)\)", src)}
    slack = int(re.search(r"PM_TASK_DEAD_SLACK = (\d+);", open(os.path.join(B.CSRC, "pm_engine_tasks.inc")).read()).group(1))
    return chunk, tile, block, slack


RO_CHUNK, SCAN_TILE, BLOCKS, DEAD_SLACK = _device_constants()
assert BLOCKS == {256}, "the sizes below are laid out for workgroups of 256"
BLOCK, WORD = 256, 64
T_EDGES = sorted({n + d for n in (WORD, BLOCK, RO_CHUNK, SCAN_TILE) for d in (-1, 0, 1)})


def _cols(n):
    z = np.zeros(n, dtype=np.uint32)
    return dict(flags=np.full(n, ON, dtype=np.uint32), gpu_count=z, gpu_mem_mb=z, gpu_model_class=z, cpu_cores=z, ram_mb=z,
                storage_gb=z, price=z, lat=np.zeros(n), lon=np.zeros(n))


def _reports(rows):
    out = np.zeros(len(rows), dtype=E.ro_report_dt)
    for k, (w, st, uid) in enumerate(rows):
        out[k] = (w, st, uid)
    return out


def _soa(tasks):
    return (np.array([t[2] for t in tasks], dtype=np.uint64), np.array([t[1] for t in tasks], dtype=np.int64),
            np.array([t[0] for t in tasks], dtype=np.uint64))


def _tuples(rows):
    assert not rows["_pad"].any() and not rows["_pad2"].any()
    return [(int(r["uid"]), int(r["created_at"]), int(r["topo_mask"]), int(r["task"]), int(r["groups_allowed"]), int(r["groups_running"]),
             int(r["workers_running"]), int(r["groups_converged"]), int(r["converged"]), tuple(r["reporters"].tolist()),
             int(r["serve"]), int(r["rollout"])) for r in rows]


def _totals(t):
    return (int(t["tasks"]), int(t["total"]), tuple(t["by_serve"].tolist()), tuple(t["by_rollout"].tolist()), int(t["unrestricted"]),
            int(t["workers_running"]), int(t["reporters"]), int(t["orphan_uids"]), int(t["orphan_reporters"]), int(t["n_cfgs"]))


def _read(eng, q):
    t, by_config, rows = eng.task_directory(*[q[k] for k in FIELDS[:7]], None if q["limit"] == M.TO_END else q["limit"])
    return _totals(t), by_config.tolist(), _tuples(rows)


def _state(eng, tasks):
    """the model's inputs from the engine's other reads (pm_get_groups, pm_rollout_get) and the caller's task list"""
    ledger = None
    try:
        uid, state = eng.rollout_get()
        ledger = list(zip(uid.tolist(), state.tolist()))
    except E.EngineError as err:
        assert err.code == ESTATE                                           # the rollout ledger is off
    return engine_groups(eng), ledger, list(tasks), eng.C


def _cross(eng, full, ro):
    """the unfiltered list against pm_task_report, pm_rollout_tasks and pm_config_report at the same moment"""
    totals, by_config, rows = full
    running, workers, allowed = eng.task_report()
    assert [r[5] for r in rows] == running.tolist() and [r[6] for r in rows] == workers.tolist()
    assert [r[4] for r in rows] == allowed.tolist() and [r[3] for r in rows] == list(range(len(rows)))
    assert by_config == eng.config_report()["tasks_allowing"].tolist()
    if not ro:
        assert totals[7:9] == (0, 0) and totals[3] == (0, 0, 0) and all(r[7:10] == (0, 0, (0,) * 8) and r[11] == M.TKR_NONE for r in rows)
        return
    rt = eng.rollout_tasks()
    by_task = {int(r["task"]): r for r in rt if int(r["task"]) != M.NONE}
    assert len(by_task) == sum(int(r["task"]) != M.NONE for r in rt)
    for r in rows:
        x = by_task.get(r[3])
        want = (int(x["groups_converged"]), int(x["converged"]), tuple(x["reporters"].tolist())) if x is not None else (0, 0, (0,) * 8)
        assert r[7:10] == want, r
    lost = [r for r in rt if int(r["task"]) == M.NONE]
    assert totals[7:9] == (len(lost), sum(int(r["reporters"].sum()) for r in lost))


def _check(eng, tasks, queries, tag=""):
    """the directory FIRST (pm_get_groups compacts the group list), then the model over what the other reads give"""
    got = [_read(eng, q) for q in queries]
    full = _read(eng, M.query())
    state = _state(eng, tasks)
    for q, g in zip(queries + [M.query()], got + [full]):
        want = M.directory(*state, q)
        assert g[0] == want[0] and g[1] == want[1], (tag, q, g[0], want[0])
        assert g[2] == want[2], (tag, q)
    _cross(eng, full, state[1] is not None)
    return state, got


def _every_query(ro=True, n_cfgs=1):
    filters = [dict(), dict(serve_mask=1 << M.TKS_STARVED), dict(serve_mask=(1 << M.TKS_RUNNING) | (1 << M.TKS_WAITING)),
               dict(workers_min=1, workers_max=3), dict(config_mask=1 << (n_cfgs - 1)), dict(config_mask=0x5555555555555555)]
    if ro:
        filters += [dict(rollout_mask=1 << M.TKR_ROLLING), dict(rollout_mask=(1 << M.TKR_CONVERGED) | (1 << M.TKR_UNHELD), workers_max=2,
                                                                serve_mask=(1 << M.TKS_RUNNING) | (1 << M.TKS_STARVED))]
    orders = (M.BY_LIST, M.BY_OLDEST, M.BY_WORKERS_DESC) + ((M.BY_REPORTERS_DESC,) if ro else ())
    return [M.query(order=o, **f) for o in orders for f in filters[:3]] + [M.query(order=orders[k % len(orders)], **f)
                                                                            for k, f in enumerate(filters[3:])]


def _engine(W, tasks, groups, n_cfgs=1, reports=None, ro=True, seed=3):
    """an engine that holds exactly `tasks` = [(uid, created_at, mask)] and `groups` = [(id, config, members, task position or -1)]"""
    eng = E.Engine(group_id_seed=seed)
    cfg_rows, alt_rows, _ = host.pack_configs([(f"c{k}", 1, 4096, None) for k in range(n_cfgs)])
    eng.set_configs(cfg_rows, alt_rows)
    return _fill(eng, W, tasks, groups, reports, ro)


def _fill(eng, W, tasks, groups, reports=None, ro=True):
    """a table of W rows (the upload drops what the engine held), exactly `tasks` and `groups`, a fresh ledger"""
    eng.upload_workers(_cols(W))
    eng.upload_tasks(*_soa(tasks))
    g = np.zeros(len(groups), dtype=E.group_dt)
    members = []
    for k, (gid, cfg, mem, t) in enumerate(groups):
        g[k] = (gid, cfg, len(mem), len(members), M.NONE if t < 0 else t)
        members += list(mem)
    if len(g):
        eng.adopt_groups(g, np.array(members, dtype=np.uint32), 99)
    if ro:
        eng.rollout_enable(True)
        if reports:
            eng.rollout_ingest(_reports(reports))
    return eng


def _table(T, rng, n_cfgs=3, G=150, W=600, dup=True):
    """T tasks (distinct ids but, with dup, a few duplicates and one id of all ones), G groups over consecutive rows that hold
    random tasks — several groups a task — and reports that name tasks, strangers and the id of all ones"""
    ids = (rng.permutation(4 * T)[:T] + 1000).astype(np.uint64).tolist()
    if dup and T > 8:
        ids[T // 2] = ids[1]
        ids[T - 1] = ids[T // 3]
        ids[T // 4] = M.ALL_ONES
    some = lambda: (int.from_bytes(rng.bytes(9), "little") & ((1 << (n_cfgs + 1)) - 1) & M.ALL_ONES) or 1   # (one bit past the installed ones)
    masks = [(M.ALL_ONES, 0, some())[int(rng.choice(3, p=[0.2, 0.05, 0.75]))] for _ in range(T)]
    tasks = [(ids[t], 10_000_000 - 3 * t, masks[t]) for t in range(T)]
    groups, at = [], 0
    hot = rng.integers(0, T, 6)                                             # a few tasks held by many groups
    for k in range(G):
        n = 1 + k % 3
        t = -1 if k % 7 == 0 else int(hot[k % 6]) if k % 2 else int(rng.integers(0, T))
        groups.append((0x5000 + k, int(rng.integers(0, n_cfgs - 1)) if n_cfgs > 1 else 0, list(range(at, at + n)), t))
        at += n
    assert at < W
    reports = []
    for w in range(W):
        x = rng.random()
        if x < 0.15:
            continue
        g = next((g for g in groups if g[2][0] <= w <= g[2][-1]), None)
        if g is not None and g[3] >= 0 and x < 0.75:
            reports.append((w, M.TS_RUNNING if x < 0.65 else 1, ids[g[3]]))
        else:
            reports.append((w, (M.TS_RUNNING, 0, 4, 7)[int(rng.integers(0, 4))], (ids[int(rng.integers(0, T))], 7, 8, M.ALL_ONES)[int(rng.integers(0, 4))]))
    return tasks, groups, reports


# ------------------------------------------------------------------ the named cases

@pytest.mark.parametrize("case", TC.CASES, ids=[c["name"] for c in TC.CASES])
def test_named_cases_through_the_c_abi(case):
    ro = case["ledger"] is not None
    reports = [(w, st, uid) for w, (uid, st) in enumerate(case["ledger"]) if st != M.TS_NONE] if ro else None
    eng = _engine(case["W"], case["tasks"], case["groups"], case["n_cfgs"], reports, ro)
    for q, positions, totals in case["queries"]:
        got = _read(eng, q)
        assert [r[3] for r in got[2]] == positions and (totals is None or got[0] == totals), (q, got[0])
    _check(eng, case["tasks"], [q for q, _, _ in case["queries"]] + _every_query(ro, case["n_cfgs"]), case["name"])
    eng.close()


# ------------------------------------------------------------------ every edge of the passes, the sort and the scan

@pytest.mark.parametrize("T", T_EDGES)
def test_tables_at_every_edge(T):
    rng = np.random.default_rng(T)
    tasks, groups, reports = _table(T, rng)
    eng = _engine(600, tasks, groups, 3, reports)
    state, got = _check(eng, tasks, _every_query(True, 3), T)
    assert got[0][0][1] == T and len(got[0][2]) == T and got[0][0][7] >= 2   # everything listed; strangers and the id of all ones
    assert len({r[10] for r in got[0][2]}) == 3 and len({r[11] for r in got[0][2]}) == 3
    assert max(r[5] for r in got[0][2]) > 3                                 # a task held by several groups
    eng.close()


def test_rollout_off_at_the_edges():
    for T in (WORD + 1, RO_CHUNK + 1):
        rng = np.random.default_rng(T)
        tasks, groups, _ = _table(T, rng)
        eng = _engine(600, tasks, groups, 3, None, ro=False)
        _, got = _check(eng, tasks, _every_query(False, 3), ("off", T))
        assert got[0][0][3] == (0, 0, 0) and all(r[11] == M.TKR_NONE for r in got[0][2])
        eng.rollout_enable(True)                                            # switched on: empty columns, every held task rolling
        _, got = _check(eng, tasks, _every_query(True, 3), ("on, empty", T))
        assert got[0][0][3][M.TKR_CONVERGED] == 0 and got[0][0][6] == 0
        eng.close()


def test_64_configurations():
    rng = np.random.default_rng(64)
    tasks, groups, reports = _table(BLOCK + 1, rng, n_cfgs=64, G=100)
    tasks[3] = (tasks[3][0], tasks[3][1], 1 << 63)
    eng = _engine(600, tasks, groups, 64, reports)
    _, got = _check(eng, tasks, _every_query(True, 64) + [M.query(config_mask=1 << 63)], "64 configurations")
    assert got[-1][0][1] >= 1 and 3 in [r[3] for r in got[-1][2]]
    eng.close()


# ------------------------------------------------------------------ tombstones, insertions in front, a rebuilt index space

def _drop(eng, tasks, positions):
    """pm_tasks_delete of the tasks at `positions` (ids carried once), and the caller's list without them"""
    gone = set(int(p) for p in positions)
    ids = [tasks[p][0] for p in sorted(gone)]
    carried = {}
    for t in tasks:
        carried[t[0]] = carried.get(t[0], 0) + 1
    assert all(carried[u] == 1 for u in ids)
    eng.tasks_delete(np.array(ids, dtype=np.uint64))
    return [t for p, t in enumerate(tasks) if p not in gone]


def test_tombstones_in_the_window():
    T = 3 * WORD + BLOCK                                                    # (a fresh upload of a multiple of 64 starts on a word)
    rng = np.random.default_rng(8)
    tasks, groups, reports = _table(T, rng, dup=False)
    eng = _engine(600, tasks, groups, 3, reports)
    sp = eng.debug_task_space()
    assert sp["t_lo"] % WORD == 0
    qs = _every_query(True, 3)
    _check(eng, tasks, qs, "whole")
    # a wholly dead word, the last slot, holes on both sides of a word edge and of the workgroup edge; then the first slot
    tasks = _drop(eng, tasks, list(range(WORD, 2 * WORD)) + [T - 1, 2 * WORD - 1 + WORD, 3 * WORD, BLOCK - 1, BLOCK, BLOCK + 7])
    state, got = _check(eng, tasks, qs, "tombstones")
    assert eng.debug_task_space()["t_dead"] == WORD + 6 and got[0][0][0] == len(tasks)
    tasks = _drop(eng, tasks, [0, 1])
    _check(eng, tasks, qs, "a dead first slot")
    assert eng.debug_task_space()["t_lo"] == sp["t_lo"] + 2
    # 37 new tasks in front: not a multiple of 64, the list starts inside a word
    new = [(900_000 + k, 20_000_000 - k, int(rng.integers(0, 16))) for k in range(37)]
    eng.tasks_insert_front(*_soa(new))
    tasks = new + tasks
    _check(eng, tasks, qs, "insert_front")
    assert eng.debug_task_space()["t_lo"] % WORD != 0
    eng.rollout_ingest(_reports([(w, M.TS_RUNNING, 900_003) for w in range(590, 600)]))
    _, got = _check(eng, tasks, qs, "reports for a new task")
    assert got[0][2][3][9][M.TS_RUNNING] == 10
    eng.close()


def test_one_engine_across_index_space_sizes():
    """One engine; the table 65 tasks, then the smallest whose sort histogram takes two tiles of the scan, then 65 again, then
    the smallest with two chunks (the sizes as tests/test_gpu_addresses.py takes them from the source).  At each size both sorted
    orders — behind the id join's own sort of the live rows — and a page in scan order between them and the next size's.  The
    scratch keeps what the largest size made it: a buffer sized for an earlier n, or the wrong result buffer behind the passes,
    is a list that is not the model's."""
    two_chunks, two_tiles = RO_CHUNK + 1, (SCAN_TILE // 256) * RO_CHUNK + 1
    assert SCAN_TILE % 256 == 0 and 256 * -(-two_tiles // RO_CHUNK) > SCAN_TILE >= 256 * -(-(two_tiles - 1) // RO_CHUNK)
    eng = E.Engine(group_id_seed=3)
    cfg_rows, alt_rows, _ = host.pack_configs([(f"c{k}", 1, 4096, None) for k in range(3)])
    eng.set_configs(cfg_rows, alt_rows)
    for step, T in enumerate((65, two_tiles, 65, two_chunks)):
        rng = np.random.default_rng(40 + step)
        tasks, groups, reports = _table(T, rng)
        _fill(eng, 600, tasks, groups, reports)
        qs = [M.query(order=M.BY_WORKERS_DESC), M.query(order=M.BY_LIST, offset=T // 2, limit=40),
              M.query(order=M.BY_REPORTERS_DESC, offset=T // 3, limit=40), M.query(order=M.BY_OLDEST, offset=T // 2, limit=40)]
        _, got = _check(eng, tasks, qs, (step, T))
        assert got[0][0][1] == T and len(got[0][2]) == T
    eng.close()


def test_a_rebuilt_index_space_lists_the_same():
    T0 = DEAD_SLACK + 300
    rng = np.random.default_rng(12)
    tasks0, groups, reports = _table(T0, rng, dup=False, G=60)
    keep = {g[3] for g in groups if g[3] >= 0} | set(range(0, T0, 97))      # the held tasks, the first row and a few others stay
    free = [p for p in range(T0) if p not in keep]
    eng = _engine(600, tasks0, groups, 3, reports)
    # n rows go, T0 - n stay: the tombstones stand up to n == (T0 - n) + PM_TASK_DEAD_SLACK
    n_gone = (T0 + DEAD_SLACK) // 2
    assert n_gone + 2 <= len(free)
    tasks = _drop(eng, tasks0, free[:n_gone])
    sp = eng.debug_task_space()
    assert (sp["compactions"], sp["T"], sp["t_dead"]) == (0, T0 - n_gone, T0 - n_gone + DEAD_SLACK)
    qs = _every_query(True, 3)
    before = _check(eng, tasks, qs, "at the threshold: mostly tombstones")[1]
    gone_ids = {tasks0[p][0] for p in free[n_gone:n_gone + 2]}
    tasks = _drop(eng, tasks, [p for p, t in enumerate(tasks) if t[0] in gone_ids])
    sp = eng.debug_task_space()
    assert (sp["compactions"], sp["t_dead"], sp["T"]) == (1, 0, T0 - n_gone - 2)
    after = _check(eng, tasks, qs, "rebuilt")[1]
    strip = lambda rows: [r[:3] + r[4:] for r in rows if r[0] not in gone_ids]   # (positions move by the two rows that went)
    assert strip(after[0][2]) == strip(before[0][2]) and len(after[0][2]) == len(before[0][2]) - 2
    eng.close()


# ------------------------------------------------------------------ windows and buffers

def test_windows_and_buffers():
    T = RO_CHUNK + 77
    rng = np.random.default_rng(21)
    tasks, groups, reports = _table(T, rng)
    eng = _engine(600, tasks, groups, 3, reports)
    L, h = E.lib(), eng._h
    for order in (M.BY_LIST, M.BY_OLDEST, M.BY_WORKERS_DESC, M.BY_REPORTERS_DESC):
        whole = _read(eng, M.query(order=order))
        total = whole[0][1]
        assert total == T
        for off, lim in ((0, 10), (T // 2, 33), (total - 1, 5), (total - 1, M.TO_END), (total, 3), (total + 9, M.TO_END), (0, 0),
                         (M.TO_END, M.TO_END), (5, M.TO_END - 1)):
            got = _read(eng, M.query(order=order, offset=off, limit=lim))
            n = 0 if off >= total else min(lim, total - off)
            assert got[0] == whole[0] and got[1] == whole[1] and got[2] == whole[2][off:off + n], (order, off, lim)
    # the buffers: a short or missing row buffer is PM_ERANGE with the totals, by_config and *n_rows written and no row copied
    q = np.zeros(1, dtype=E.tdir_query_dt)
    q[0] = (M.ALL_ONES, 7, 7, 0, M.NONE, M.BY_WORKERS_DESC, 3, 20, 0)
    want = _read(eng, M.query(order=M.BY_WORKERS_DESC, offset=3, limit=20))
    t, c, n = np.zeros(1, dtype=E.tdir_totals_dt), np.full(64, 77, dtype=np.uint32), E.C.c_uint32(77)
    buf = np.zeros(20, dtype=E.tdir_row_dt)
    assert L.pm_task_directory(h, q.ctypes.data, t.ctypes.data, c.ctypes.data, 64, None, 0, E.C.byref(n)) == ERANGE
    assert n.value == 20 and _totals(t[0]) == want[0] and c[:3].tolist() == want[1] and (c[3:] == 77).all()
    assert L.pm_task_directory(h, q.ctypes.data, t.ctypes.data, None, 0, buf.ctypes.data, 19, E.C.byref(n)) == ERANGE
    assert n.value == 20 and not buf.view(np.uint8).any()
    c[:] = 77
    assert L.pm_task_directory(h, q.ctypes.data, t.ctypes.data, c.ctypes.data, 2, buf.ctypes.data, 20, E.C.byref(n)) == ERANGE
    assert n.value == 20 and not buf.view(np.uint8).any() and (c == 77).all() and _totals(t[0]) == want[0]
    assert L.pm_task_directory(h, q.ctypes.data, t.ctypes.data, None, 0, buf.ctypes.data, 20, E.C.byref(n)) == 0
    assert n.value == 20 and _tuples(buf) == want[2]
    eng.close()


# ------------------------------------------------------------------ behind a real tick

def _churn_engine(seed, W0=220, carve_wgs=None):
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
    if carve_wgs is not None:
        eng.set_carve_workgroups(carve_wgs)
    tasks = list(zip(cs.uid.tolist(), cs.created.tolist(), cs.masks.tolist()))
    return cs, packed, eng, tasks


def _life_queries(n_cfgs):
    return [M.query(order=M.BY_WORKERS_DESC), M.query(order=M.BY_OLDEST, serve_mask=1 << M.TKS_STARVED),
            M.query(order=M.BY_REPORTERS_DESC, rollout_mask=(1 << M.TKR_ROLLING) | (1 << M.TKR_CONVERGED), offset=1, limit=20),
            M.query(config_mask=((1 << n_cfgs) - 2) or 1, limit=0)]


def test_reads_follow_the_life_cycle():
    cs, packed, eng, tasks = _churn_engine(3)
    pick = lambda idx: {k: np.ascontiguousarray(v[idx]) for k, v in packed.items()}
    LQ = _life_queries(eng.C)
    eng.rollout_enable(True)
    rng = np.random.default_rng(11)
    _check(eng, tasks, LQ, "before a tick: no groups")
    eng.tick()
    state, _ = _check(eng, tasks, LQ, "behind a tick: the pending groups are taken in")
    assert len(state[0]) > 3 and any(g[3] >= 0 for g in state[0])
    # every member of a group reports its group's task, running, but every fifth row; a few strangers
    reports = []
    for _, _, members, t in state[0]:
        reports += [(w, M.TS_RUNNING, tasks[t][0]) for w in members if t >= 0 and w % 5]
    eng.rollout_ingest(_reports(reports + [(w, 4, 123456789) for w in range(0, cs.W, 31)]))
    _, got = _check(eng, tasks, LQ + [M.query()], "reported")
    assert got[-1][0][3][M.TKR_CONVERGED] > 0 and got[-1][0][3][M.TKR_ROLLING] > 0
    for k in range(2):
        leave, idx_new, new_tasks = cs.step()
        eng.on_worker_status_many(leave, np.zeros(len(leave), dtype=np.uint32), np.ones(len(leave), dtype=np.uint32))
        _check(eng, tasks, LQ, "dead workers: their groups dissolve, tombstones stay in the group list")
        eng.append_workers(pick(idx_new))
        eng.tasks_insert_front(*new_tasks[:3])
        tasks = list(zip(new_tasks[2].tolist(), new_tasks[1].tolist(), new_tasks[0].tolist())) + tasks
        _check(eng, tasks, LQ, "insert_front: positions move")
        eng.tick()
        _check(eng, tasks, LQ, f"churn {k}")
    state, _ = _check(eng, tasks, LQ, "again")
    victim = [t for _, _, _, t in state[0] if t >= 0][0]
    tasks = _drop(eng, tasks, [victim])                                     # a claimed task goes and takes its groups with it
    state2, got = _check(eng, tasks, LQ + [M.query()], "after pm_tasks_delete")
    assert len(state2[0]) < len(state[0]) and got[-1][0][7] >= 2            # its reporters report an orphan now
    eng.close()


# ------------------------------------------------------------------ errors

def test_errors_leave_everything_as_it_was():
    rng = np.random.default_rng(9)
    tasks, groups, reports = _table(300, rng)
    eng = _engine(600, tasks, groups, 3, reports)
    L, h = E.lib(), eng._h
    good = M.query(order=M.BY_WORKERS_DESC, offset=2, limit=30)
    before = _read(eng, good)
    assert len(before[2]) == 30

    def call(q, totals=True, n=True, rows=None, cap=0):
        qa = np.zeros(1, dtype=E.tdir_query_dt)
        if q is not None:
            qa[0] = tuple(q[k] for k in FIELDS) + (0,)
        t, nn, c = np.full(14, 77, dtype=np.uint32), E.C.c_uint32(77), np.full(64, 77, dtype=np.uint32)
        rc = L.pm_task_directory(h, qa.ctypes.data if q is not None else None, t.ctypes.data if totals else None, c.ctypes.data, 64,
                                 rows, cap, E.C.byref(nn) if n else None)
        return rc, t.tolist(), nn.value, c.tolist()

    untouched = lambda code: (code, [77] * 14, 77, [77] * 64)
    assert call(None) == untouched(EINVAL) and call(good, totals=False)[0] == EINVAL and call(good, n=False)[0] == EINVAL
    assert L.pm_task_directory(None, None, None, None, 0, None, 0, None) == EINVAL
    for bad in (dict(good, config_mask=0), dict(good, serve_mask=0), dict(good, serve_mask=8), dict(good, serve_mask=7 | (1 << 31)),
                dict(good, rollout_mask=0), dict(good, rollout_mask=1 << M.TKR_N), dict(good, order=4), dict(good, order=0xFFFFFFFF),
                dict(good, workers_min=5, workers_max=4)):
        assert call(bad) == untouched(EINVAL), bad
    assert _read(eng, good) == before
    # the ledger off: a rollout filter and the order by reporters are refused, "all" passes
    eng.rollout_enable(False)
    assert call(dict(good, rollout_mask=1 << M.TKR_ROLLING)) == untouched(ESTATE)
    assert call(dict(good, order=M.BY_REPORTERS_DESC)) == untouched(ESTATE)
    assert call(dict(good, limit=0))[0] == 0
    _check(eng, tasks, [good], "rollout off")
    eng.dist_configure(0, 2, np.zeros(600, dtype=np.uint8))                 # a multi-GPU engine
    assert call(good) == untouched(ESTATE)
    eng.dist_configure(0, 1)
    eng.rollout_enable(True)
    eng.rollout_ingest(_reports(reports))
    assert _read(eng, good) == before
    eng.dist_tick_begin()                                                   # a stepwise tick in progress
    assert call(good) == untouched(ESTATE)
    eng.dist_carve_wait()
    eng.dist_match_begin()
    eng.dist_tick_end()
    _check(eng, tasks, [good], "behind the stepwise tick")
    # rollout on over a task table uploaded without ids
    eng.upload_tasks(*_soa(tasks)[:2])
    assert call(good) == untouched(ESTATE)
    eng.rollout_enable(False)
    t, by_config, rows = eng.task_directory()
    assert int(t["total"]) == len(tasks) and not rows["uid"].any() and rows["task"].tolist() == list(range(len(tasks)))
    eng.close()
    # no configurations, no workers, no tasks; an empty table is a table
    eng = E.Engine()
    for step in (lambda: eng.set_configs(*host.pack_configs([("any", 1, 8, None)])[:2]), lambda: eng.upload_workers(_cols(4)),
                 lambda: eng.upload_tasks(np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.uint64))):
        with pytest.raises(E.EngineError) as ei:
            eng.task_directory()
        assert ei.value.code == ESTATE
        step()
    eng.rollout_enable(True)
    eng.rollout_ingest(_reports([(1, M.TS_RUNNING, 5), (2, 0, 5), (3, 1, 6)]))
    t, by_config, rows = eng.task_directory()
    assert _totals(t) == (0, 0, (0, 0, 0), (0, 0, 0), 0, 0, 0, 2, 3, 1) and by_config.tolist() == [0] and not len(rows)
    eng.close()


# ------------------------------------------------------------------ what the directory leaves alone, determinism

def _feed(eng):
    for q in _life_queries(eng.C) + [M.query()]:
        _read(eng, q)


def test_the_task_directory_leaves_the_engine_alone():
    """two engines fed identically, one of them also asked the directory between every step: the groups, pm_last_stats' state
    counters, the published rows and the ledger end bit-identical, and the engines give back what they took"""
    gc.collect()
    base = E.Engine.debug_live_allocations()
    (ca, pa, a, _), (cb, pb, b, _) = _churn_engine(2, W0=400), _churn_engine(2, W0=400)
    for eng in (a, b):
        eng.rollout_enable(True)
    image = lambda eng: b"".join(np.asarray(x).tobytes() for x in (*eng.rollout_get(), *eng.get_groups()))
    counters = ("n_groups", "n_formed", "n_merged", "carve_steps", "pair_evals")
    _feed(a)
    sa, sb = a.tick(), b.tick()
    assert {c: sa[c] for c in counters} == {c: sb[c] for c in counters}
    _feed(a)                                                                # behind the tick, before anything took its groups in
    assert engine_groups(a) == engine_groups(b)
    for k in range(2):
        (la, ia, ta), (lb, ib, tb) = ca.step()[:3], cb.step()[:3]
        for eng, packed, leave, idx_new, new_tasks in ((a, pa, la, ia, ta), (b, pb, lb, ib, tb)):
            eng.on_worker_status_many(leave, np.zeros(len(leave), dtype=np.uint32), np.ones(len(leave), dtype=np.uint32))
            eng.append_workers({kk: np.ascontiguousarray(v[idx_new]) for kk, v in packed.items()})
            if eng is a:
                _feed(a)
            eng.tasks_insert_front(*new_tasks[:3])
            eng.rollout_ingest(_reports([(int(w), 2, int(new_tasks[2][0])) for w in idx_new]))
            if eng is a:
                _feed(a)
        sa, sb = a.tick(), b.tick()
        assert {c: sa[c] for c in counters} == {c: sb[c] for c in counters}, k
        _feed(a)
        la, lb = a.last_stats(), b.last_stats()
        assert {c: la[c] for c in counters} == {c: lb[c] for c in counters}, k
        assert engine_groups(a) == engine_groups(b), k
        for w in range(ca.W):
            x, y = a.lookup(w), b.lookup(w)
            assert (x.task, x.group_slot, x.group_index, x.group_size, x.next_worker, x.group_id) == \
                   (y.task, y.group_slot, y.group_index, y.group_size, y.next_worker, y.group_id), (k, w)
        before = image(a)
        _feed(a)
        assert image(a) == before == image(b)
    a.close(), b.close()
    del a, b
    gc.collect()
    assert E.Engine.debug_live_allocations() == base


def test_reads_are_deterministic_and_the_grid_does_not_matter():
    def image(eng):
        out = []
        for q in _every_query(True, eng.C) + [M.query(order=M.BY_REPORTERS_DESC, offset=5, limit=77)]:
            t, by_config, rows = eng.task_directory(*[q[k] for k in FIELDS[:7]], None if q["limit"] == M.TO_END else q["limit"])
            out.append(t.tobytes() + by_config.tobytes() + rows.tobytes())
        return b"".join(out)

    def swarm(carve_wgs=None):
        cs, _, eng, tasks = _churn_engine(9, W0=500, carve_wgs=carve_wgs)
        eng.rollout_enable(True)
        eng.tick()
        eng.rollout_ingest(_reports([(w, M.TS_RUNNING if w % 3 else 1, tasks[w % 7][0]) for w in range(0, cs.W, 2)]))
        return eng

    eng = swarm()
    first = image(eng)
    assert image(eng) == first                                              # two identical calls, byte for byte
    eng.rollout_summary(), eng.task_report(), eng.rollout_tasks()
    assert image(eng) == first                                              # and after unrelated reads
    one, many = swarm(1), swarm(64)                                         # the same swarm carved by one workgroup, and by many
    assert image(one) == first and image(many) == first
    eng.close(), one.close(), many.close()
