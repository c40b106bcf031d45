"""The group directory on the GPU (pm_group_directory of include/pm_engine.h, kernels in pm_groupdir.inc) against the model of
tests/groupdir_model.py, which tests/test_groupdir_model.py holds to the definitions: the named cases through the C ABI, groups
installed with pm_adopt_groups at every edge of the member pass, the group pass, the scan and the sort, a family behind a real
pm_tick, windows, both ledgers on and off, the life cycle, every error, what the call leaves alone, and determinism.  Every
comparison is exact, every listed row and every counter of every query is compared."""
import gc
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

import groupdir_cases as GC
import groupdir_model as M

pytestmark = pytest.mark.gpu
EINVAL, ESTATE, ERANGE = -1, -4, -5
ON = E.W_HEALTHY | E.W_HAS_P2P
TASKS = [11, 12, 13, M.ALL_ONES]
LOST_OR_DEGRADED = (1 << M.GH_LOST) | (1 << M.GH_DEGRADED)


def _device_constants():
    """the tile sizes the passes, the scan and the sort work in, read from the device source: a change there moves the sizes below"""
    dev = open(os.path.join(B.CSRC, "pm_device.h")).read()
    chunk = int(re.search(r"\bPM_RO_CHUNK\s*=\s*(\d+)", dev).group(1))
    kernels = open(os.path.join(B.CSRC, "pm_metrics.inc")).read()
    scan = kernels[kernels.index("void mx_scan_kernel("):kernels.index("void mx_copy_kernel(")]
    tile = int(re.search(r"base \+= (\d+)u", scan).group(1))
    src = open(os.path.join(B.CSRC, "pm_groupdir.inc")).read()
    block = {int(x) for x in re.findall(r"__launch_bounds__\((\d+)\)", src)}
    return chunk, tile, block


RO_CHUNK, SCAN_TILE, BLOCKS = _device_constants()
assert BLOCKS == {256}, "the member-pass shapes below are laid out for workgroups of 256"
BLOCK = 256


def _cols(n, flags=ON, ranks=None):
    z = np.zeros(n, dtype=np.uint32)
    c = dict(flags=np.full(n, flags, dtype=np.uint32), gpu_count=z, gpu_mem_mb=z, gpu_model_class=z, cpu_cores=z, ram_mb=z,
             storage_gb=z, price=z, lat=np.zeros(n), lon=np.zeros(n))
    if ranks is not None:
        c["addr_rank"] = np.asarray(ranks, dtype=np.uint32)
    return c


def _reports(rows):
    out = np.zeros(len(rows), dtype=E.ro_report_dt)
    for k, (w, st, uid) in enumerate(rows):
        out[k] = (w, st, uid)
    return out


def _tuples(rows):
    assert not rows["_pad"].any()
    return [(int(r["group_id"]), int(r["slot"]), int(r["config"]), int(r["size"]), int(r["task"]), int(r["member_begin"]),
             int(r["health"]), int(r["rollout"]), tuple(r["by_status"].tolist()), int(r["converged"]), int(r["behind"]),
             int(r["other"]), int(r["silent"])) for r in rows]


def _read(eng, q):
    t, by_config, rows, members = eng.group_directory(q["config_mask"], q["holds"], q["size_min"], q["size_max"], q["health_mask"],
                                                      q["rollout_mask"], q["order"], q["offset"],
                                                      None if q["limit"] == M.TO_END else q["limit"])
    totals = (int(t["total"]), int(t["members_total"]), tuple(t["by_health"].tolist()), tuple(t["by_rollout"].tolist()),
              int(t["n_cfgs"]))
    return totals, by_config.tolist(), _tuples(rows), members.tolist()


def _state(eng, ranks, task_uids):
    """the model's inputs from the engine's other reads: pm_get_groups, the ledgers"""
    statuses = ledger = None
    try:
        statuses = eng.liveness_get()[0].tolist()
    except E.EngineError as err:
        assert err.code == ESTATE                                           # liveness is off
    try:
        uid, state = eng.rollout_get()
        ledger = list(zip(uid.tolist(), state.tolist()))
    except E.EngineError as err:
        assert err.code == ESTATE                                           # the rollout ledger is off
    return engine_groups(eng), statuses, ledger, list(ranks), list(task_uids), eng.C


def _check(eng, ranks, task_uids, queries, tag=""):
    """the directory FIRST (pm_get_groups compacts the list: the directory must number the slots over the tombstones), then the
    model over what the other reads give"""
    got = [_read(eng, q) for q in queries]
    state = _state(eng, ranks, task_uids)
    for q, g in zip(queries, got):
        want = M.directory(*state, q)
        assert g[0] == want[0] and g[1] == want[1], (tag, q)
        assert g[2] == want[2], (tag, q)
        assert g[3] == want[3], (tag, q)
    return state, got


def _every_query(live=True, ro=True, n_cfgs=1):
    filters = [dict(), dict(holds=M.WITH_TASK, size_min=2), dict(holds=M.WITHOUT_TASK), dict(size_min=1, size_max=64)]
    if live:
        filters += [dict(health_mask=LOST_OR_DEGRADED), dict(health_mask=1 << M.GH_SOUND)]
    if ro:
        filters += [dict(rollout_mask=1 << M.GR_ROLLING), dict(rollout_mask=(1 << M.GR_CONVERGED) | (1 << M.GR_NO_TASK))]
    if live and ro:
        filters += [dict(health_mask=1 << M.GH_DEGRADED, rollout_mask=1 << M.GR_ROLLING, holds=M.WITH_TASK)]
    if n_cfgs > 1:
        filters += [dict(config_mask=0xAAAAAAAAAAAAAAAA), dict(config_mask=1 << (n_cfgs - 1))]
    return [M.query(order=o, **f) for o in (M.BY_SLOT, M.BY_ID_TEXT, M.BY_SIZE_DESC) for f in filters]


def _engine(W, groups, n_cfgs=1, ranks=None, statuses=None, reports=None, live=True, ro=True, tasks=TASKS, seed=3):
    """an engine that holds exactly `groups` = [(id, config, members, task position or -1)]"""
    eng = E.Engine(group_id_seed=seed)
    cfg_rows, alt_rows, _ = host.pack_configs([(f"c{k}", 1, 4096, None) for k in range(n_cfgs)])
    eng.set_configs(cfg_rows, alt_rows)
    return _fill(eng, W, groups, ranks, statuses, reports, live, ro, tasks)


def _fill(eng, W, groups, ranks=None, statuses=None, reports=None, live=True, ro=True, tasks=TASKS):
    """a table of W rows (the upload drops what the engine held), the tasks, exactly `groups`, fresh ledgers"""
    eng.upload_workers(_cols(W, ranks=ranks))
    T = len(tasks)
    eng.upload_tasks(np.full(T, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64), np.arange(T, 0, -1).astype(np.int64), np.array(tasks, dtype=np.uint64))
    g = np.zeros(len(groups), dtype=E.group_dt)
    members = []
    for k, (gid, cfg, mem, t) in enumerate(groups):
        g[k] = (gid, cfg, len(mem), len(members), M.NONE if t < 0 else t)
        members += list(mem)
    if len(g):
        eng.adopt_groups(g, np.array(members, dtype=np.uint32), 99)
    if live:
        eng.liveness_enable(True)
        if statuses is not None:
            eng.liveness_set(np.arange(W, dtype=np.uint32), np.asarray(statuses, dtype=np.uint8), np.zeros(W, dtype=np.uint32))
    if ro:
        eng.rollout_enable(True)
        if reports is not None:
            eng.rollout_ingest(_reports(reports))
    return eng


def _random_ledgers(W, rng, tasks=TASKS, healthy=0.8):
    statuses = np.where(rng.random(W) < healthy, M.HEALTHY, rng.integers(0, M.NS_N, W))
    reports = [(w, int(rng.choice([M.RUNNING, M.RUNNING, M.RUNNING, 0, 5])), int(tasks[rng.integers(0, len(tasks))]))
               for w in range(W) if rng.random() < 0.9]
    return statuses, reports


def _even_groups(G, rng, n_cfgs=1, sizes=(1, 2, 3), cfg=None, ids=None):
    """G groups over consecutive rows -> (groups, W)"""
    ids = ids if ids is not None else GC.distinct_ids(G, rng)
    groups, at = [], 0
    for k in range(G):
        n = int(sizes[k % len(sizes)])
        groups.append((ids[k], (k % n_cfgs) if cfg is None else cfg, list(range(at, at + n)), int(rng.integers(-1, 3))))
        at += n
    return groups, at + 5                                                   # (five free rows behind them)


# ------------------------------------------------------------------ the named cases

@pytest.mark.parametrize("case", GC.CASES, ids=[c["name"] for c in GC.CASES])
def test_named_cases_through_the_c_abi(case):
    live, ro = case["statuses"] is not None, case["ledger"] is not None
    reports = [(w, st, uid) for w, (uid, st) in enumerate(case["ledger"]) if st != M.TS_NONE] if ro else None
    eng = _engine(case["W"], case["groups"], case["n_cfgs"], case["ranks"], case["statuses"], reports, live, ro,
                  tasks=case["tasks"] or [1])
    tasks = case["tasks"] or [1]
    for q, slots, totals in case["queries"]:
        got = _read(eng, q)
        assert got[0] == totals and [r[1] for r in got[2]] == slots, q
    _check(eng, case["ranks"], tasks, [q for q, _, _ in case["queries"]] + _every_query(live, ro, case["n_cfgs"]), case["name"])
    eng.close()


# ------------------------------------------------------------------ the member pass

def _member_shapes():
    """W = 4097: a group that is exactly one wave, the next wave, 65 members over two waves, two rows across the workgroup edge,
    two groups interleaved lane by lane, a group of 1, 300 members scattered over the table, and a group that is dissolved"""
    W = 4097
    rng = np.random.default_rng(41)
    fixed = [list(range(0, 64)), list(range(64, 128)), list(range(128, 193)), [BLOCK - 1, BLOCK],
             list(range(320, 384, 2)), list(range(321, 384, 2)), [400], list(range(450, 460))]
    rest = np.setdiff1d(np.arange(W), np.concatenate([np.array(m) for m in fixed]))
    scattered = sorted(rng.choice(rest, 300, replace=False).tolist())
    assert scattered[0] < BLOCK and scattered[-1] > W - BLOCK
    ids = GC.distinct_ids(len(fixed) + 1, rng)
    groups = [(ids[k], 0, m, [0, 1, 2, -1][k % 4]) for k, m in enumerate(fixed + [scattered])]
    return W, groups


@pytest.mark.parametrize("live,ro", [(True, True), (True, False), (False, True), (False, False)])
def test_member_pass_shapes_and_ledgers_on_and_off(live, ro):
    W, groups = _member_shapes()
    rng = np.random.default_rng(7)
    statuses, reports = _random_ledgers(W, rng, healthy=0.5)
    statuses[0:64] = M.HEALTHY                                              # one sound, converged group: a whole wave on one word
    statuses[[BLOCK - 1, BLOCK, 400]] = [M.DEAD, M.HEALTHY, M.UNHEALTHY]    # a lost group across the workgroup edge, a degraded group of 1
    reports = [r for r in reports if r[0] >= 64] + [(w, M.RUNNING, TASKS[0]) for w in range(64)]
    ranks = rng.integers(0, 50, W)                                          # equal ranks inside the groups: the members by row
    eng = _engine(W, groups, 1, ranks, statuses, reports, live, ro)
    queries = _every_query(live, ro)
    (gr, st, led, *_), got = _check(eng, ranks, TASKS, queries, "adopted")
    if live:
        assert got[0][2][0][6] == M.GH_SOUND and len({r[6] for r in got[0][2]}) == 3
        assert set(range(M.NS_N)) <= {s for r in got[0][2] for s in range(M.NS_N) if r[8][s]}  # every status on some member
    else:
        assert all(r[6] == M.GH_NONE and not any(r[8]) for r in got[0][2]) and got[0][0][2] == (0, 0, 0)
    if ro:
        assert got[0][2][0][7] == M.GR_CONVERGED and got[0][2][0][9] == 64
        assert all(sum(r[9:]) == (r[3] if r[4] != M.NONE else 0) for r in got[0][2])
    else:
        assert all(r[7] == M.GR_NONE and r[9:] == (0, 0, 0, 0) for r in got[0][2]) and got[0][0][3] == (0, 0, 0)
    # the group of rows 450..459 goes (a tombstone in the list, no compaction), rows are appended behind the groups
    eng.dissolve_group(7)
    first = eng.append_workers(_cols(70, ranks=np.arange(70)))
    ranks = np.concatenate([ranks, np.arange(70)])
    if ro:
        eng.rollout_ingest(_reports([(first + 3, M.RUNNING, TASKS[0])]))
    state, got = _check(eng, ranks, TASKS, queries, "a tombstone and appended rows")
    assert len(state[0]) == len(groups) - 1 and got[0][0][0] == len(groups) - 1 and got[0][2][-1][1] == len(groups) - 2
    eng.close()


# ------------------------------------------------------------------ the group pass and the census

G_EDGES = sorted({1, 63, 64, 65, 255, 256, 257, BLOCK + 1, SCAN_TILE + 1})


@pytest.mark.parametrize("G", G_EDGES)
@pytest.mark.parametrize("spread", ["one_config", "64_configs", "config_63"])
def test_group_pass_and_census_at_every_edge(G, spread):
    rng = np.random.default_rng(G)
    n_cfgs = 1 if spread == "one_config" else 64
    groups, W = _even_groups(G, rng, n_cfgs, cfg=63 if spread == "config_63" else None)
    statuses, reports = _random_ledgers(W, rng)
    eng = _engine(W, groups, n_cfgs, None, statuses, reports)
    queries = _every_query(True, True, n_cfgs)
    _, got = _check(eng, range(W), TASKS, queries, (G, spread))
    assert got[0][0][0] == G and sum(got[0][1]) == G
    if spread == "config_63":
        assert got[0][1] == [0] * 63 + [G]
    eng.close()


@pytest.mark.parametrize("which", ["first", "last", "every_other"])
def test_tombstones_in_the_list(which):
    G = 2 * BLOCK + 3
    rng = np.random.default_rng(2)
    groups, W = _even_groups(G, rng, 4)
    statuses, reports = _random_ledgers(W, rng)
    eng = _engine(W, groups, 4, None, statuses, reports)
    gone = {"first": [0], "last": [G - 1], "every_other": list(range(0, G, 2))}[which]
    for gid in [groups[k][0] for k in gone]:                                # (by id: a slot number would move with the list)
        assert eng.dissolve_group_by_id(gid)
    state, got = _check(eng, range(W), TASKS, _every_query(True, True, 4), which)
    assert got[0][0][0] == G - len(gone) and [r[1] for r in got[0][2]] == list(range(G - len(gone)))
    eng.close()


# ------------------------------------------------------------------ the sort

@pytest.mark.parametrize("G", [RO_CHUNK - 1, RO_CHUNK, RO_CHUNK + 1, 2 * RO_CHUNK + 77])
def test_sorted_orders_at_the_chunk_edges(G):
    rng = np.random.default_rng(G)
    ids = GC.id_edge_set() + GC.distinct_ids(G, rng)
    ids = list(dict.fromkeys(ids))[:G]
    rng.shuffle(ids)
    groups, W = _even_groups(G, rng, 2, sizes=rng.integers(1, 6, 64), ids=[int(i) for i in ids])
    eng = _engine(W, groups, 2, None, *_random_ledgers(W, rng))
    qs = [M.query(order=M.BY_ID_TEXT), M.query(order=M.BY_SIZE_DESC), M.query(order=M.BY_ID_TEXT, health_mask=LOST_OR_DEGRADED),
          M.query(order=M.BY_ID_TEXT, offset=RO_CHUNK - 5, limit=11), M.query(order=M.BY_SIZE_DESC, offset=RO_CHUNK - 5, limit=11),
          M.query(order=M.BY_SLOT, offset=RO_CHUNK - 5, limit=11)]
    _, got = _check(eng, range(W), TASKS, qs, G)
    texts = [format(r[0], "x") for r in got[0][2]]
    assert len(texts) == G and texts == sorted(texts)
    assert [(-r[3], r[1]) for r in got[1][2]] == sorted((-r[3], r[1]) for r in got[1][2])
    eng.close()


def test_one_engine_across_index_space_sizes():
    """One engine; the list 65 groups, then the smallest whose sort histogram takes two tiles of the scan, then 65 again, then
    the smallest with two chunks (the sizes as tests/test_gpu_addresses.py takes them from the source).  At each size both sorted
    orders and a page in scan order between them and the next size's.  The scratch keeps what the largest size made it: a buffer
    sized for an earlier n, or the wrong result buffer behind the passes, is a list that is not the model's."""
    two_chunks, two_tiles = RO_CHUNK + 1, (SCAN_TILE // 256) * RO_CHUNK + 1
    assert SCAN_TILE % 256 == 0 and 256 * -(-two_tiles // RO_CHUNK) > SCAN_TILE >= 256 * -(-(two_tiles - 1) // RO_CHUNK)
    eng = E.Engine(group_id_seed=3)
    cfg_rows, alt_rows, _ = host.pack_configs([(f"c{k}", 1, 4096, None) for k in range(2)])
    eng.set_configs(cfg_rows, alt_rows)
    for step, G in enumerate((65, two_tiles, 65, two_chunks)):
        rng = np.random.default_rng(40 + step)
        groups, W = _even_groups(G, rng, 2, sizes=(1, 2, 1, 3))
        _fill(eng, W, groups, None, *_random_ledgers(W, rng))
        qs = [M.query(order=M.BY_ID_TEXT), M.query(order=M.BY_SLOT, offset=G // 2, limit=40),
              M.query(order=M.BY_SIZE_DESC, offset=G // 3, limit=40), M.query(order=M.BY_SLOT, health_mask=LOST_OR_DEGRADED)]
        _, got = _check(eng, range(W), TASKS, qs, (step, G))
        texts = [format(r[0], "x") for r in got[0][2]]
        assert len(texts) == G and texts == sorted(texts)
    eng.close()


def _id_sets():
    n = 2 * RO_CHUNK + 77
    rng = np.random.default_rng(19)
    sets = {"edge_set": GC.id_edge_set()}
    for k in range(8):                       # seven of eight bytes agree, byte k alone differs: a pass that skipped it leaves them unsorted
        base = 0x5566778899AABBCC & ~(0xFF << (8 * k))
        digits = rng.permutation(256)
        sets[f"only_byte_{k}"] = [base | (int(d) << (8 * k)) for d in digits]
    # the same across a chunk edge: RO_CHUNK - 128 fillers in front in slot order, so the 256 straddle the first chunk's end
    fill = [0x1000 + i for i in range(RO_CHUNK - 128)]
    sets["only_byte_0_across_a_chunk_edge"] = fill + sets["only_byte_0"]
    sets["only_byte_7_across_a_chunk_edge"] = fill + sets["only_byte_7"]
    sets["every_length_long_list"] = GC.distinct_ids(n, rng)
    return sets


ID_SETS = _id_sets()


@pytest.mark.parametrize("name", list(ID_SETS))
def test_by_id_text_id_edges(name):
    ids = ID_SETS[name]
    rng = np.random.default_rng(len(ids))
    groups, W = _even_groups(len(ids), rng, 1, sizes=(1,), ids=ids)
    eng = _engine(W, groups, 1, None, live=False, ro=False)
    _, got = _check(eng, range(W), TASKS, [M.query(order=M.BY_ID_TEXT), M.query(order=M.BY_ID_TEXT, offset=len(ids) // 2, limit=9)], name)
    assert [r[0] for r in got[0][2]] == sorted(ids, key=lambda x: format(x, "x"))
    eng.close()


@pytest.mark.parametrize("sizes", ["all_equal", "one_to_300"])
def test_by_size_desc(sizes):
    rng = np.random.default_rng(23)
    sz = [3] * (RO_CHUNK + 9) if sizes == "all_equal" else rng.permutation(np.arange(1, 301)).tolist()
    groups, W = _even_groups(len(sz), rng, 1, sizes=sz)
    eng = _engine(W, groups, 1, None, *_random_ledgers(W, rng))
    _, got = _check(eng, range(W), TASKS, [M.query(order=M.BY_SIZE_DESC), M.query(order=M.BY_SIZE_DESC, size_min=2, size_max=299,
                                                                                     offset=7, limit=50)], sizes)
    if sizes == "all_equal":
        assert [r[1] for r in got[0][2]] == list(range(len(sz)))            # the stable tie falls to the slot
    else:
        assert [r[3] for r in got[0][2]] == list(range(300, 0, -1))
    eng.close()


# ------------------------------------------------------------------ behind a real tick, windows

def _swarm_engine(W, seed=None, carve_wgs=None):
    sw = make_swarm(100 + W if seed is None else seed, 24, W)
    eng = E.Engine(group_id_seed=7)
    host.load_swarm(eng, sw)
    if carve_wgs is not None:
        eng.set_carve_workgroups(carve_wgs)
    eng.liveness_enable(True)
    eng.rollout_enable(True)
    eng.tick()
    rng = np.random.default_rng(W)
    statuses = np.where(rng.random(W) < 0.85, M.HEALTHY, rng.integers(0, M.NS_N, W))
    eng.liveness_set(np.arange(W, dtype=np.uint32), statuses.astype(np.uint8), np.zeros(W, dtype=np.uint32))
    uids = sw.task_uid.tolist()
    reps = [(int(w), int(rng.choice([M.RUNNING, M.RUNNING, M.RUNNING, 1])), int(uids[rng.integers(0, len(uids))]) if rng.random() < 0.9
             else int(rng.integers(1, 1 << 63))) for w in range(W) if rng.random() < 0.9]
    eng.rollout_ingest(_reports(reps))
    return sw, eng


@pytest.mark.parametrize("W", [65, 257, 1025, 4097])
def test_seeded_swarms_behind_a_real_tick(W):
    sw, eng = _swarm_engine(W)
    state, got = _check(eng, sw.addr_rank().tolist(), sw.task_uid.tolist(), _every_query(True, True, eng.C), W)
    if W >= 1025:
        assert len(state[0]) > 20 and any(t >= 0 for _, _, _, t in state[0])
        assert all(got[0][0][2]) and got[0][0][3][M.GR_ROLLING]
    # the status census of the grouped rows is the node directory's
    total, counts, _ = eng.directory(membership=E.DIR_GROUPED, limit=0)
    assert total == got[0][0][1] and counts.tolist() == [sum(r[8][s] for r in got[0][2]) for s in range(M.NS_N)]
    # the rollout counters are the rollout ledger's own reads of the same engine
    ro_rows = {int(r["slot"]): r for r in eng.rollout_groups()}
    summary = eng.rollout_summary()
    assert int(summary["groups_converged"]) == got[0][0][3][M.GR_CONVERGED]
    assert int(summary["groups_with_task"]) == got[0][0][3][M.GR_CONVERGED] + got[0][0][3][M.GR_ROLLING]
    for r in got[0][2]:
        if r[4] == M.NONE:
            assert r[1] not in ro_rows and r[7] == M.GR_NO_TASK
            continue
        g = ro_rows[r[1]]
        same = g["same"].tolist()
        assert (r[9], r[10], r[11], r[12]) == (same[M.RUNNING], sum(same) - same[M.RUNNING], int(g["other"]), int(g["silent"]))
    eng.close()


@pytest.fixture(scope="module")
def big():
    """2 RO_CHUNK + 77 adopted groups, every class present; the unpaged lists of every order, read once"""
    G = 2 * RO_CHUNK + 77
    rng = np.random.default_rng(31)
    groups, W = _even_groups(G, rng, 3)
    eng = _engine(W, groups, 3, rng.integers(0, 9, W), *_random_ledgers(W, rng))
    full = {o: _read(eng, M.query(order=o)) for o in (M.BY_SLOT, M.BY_ID_TEXT, M.BY_SIZE_DESC)}
    yield eng, G, full
    eng.close()


@pytest.mark.parametrize("order", [M.BY_SLOT, M.BY_ID_TEXT, M.BY_SIZE_DESC])
def test_windows_at_every_edge(big, order):
    eng, total, full = big
    totals, by_config, rows, members = full[order]
    assert totals[0] == total == len(rows) and len(members) == totals[1]
    windows = [(0, 1), (total - 1, 1), (total, 5), (total + 1, 5), (7, M.TO_END), (total - 1, M.TO_END), (0, 0), (5, 0),
               (RO_CHUNK - 3, 7), (2 * RO_CHUNK - 1, 2), (0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF, 1), (3, 0xFFFFFFFE)]
    for off, lim in windows:
        got = _read(eng, M.query(order=order, offset=off, limit=lim))
        first, n = M.window(total, off, lim)
        want = rows[first:first + n]
        m0 = want[0][5] if n else 0
        assert got[0] == totals and got[1] == by_config, (off, lim)
        assert got[2] == [r[:5] + (r[5] - m0,) + r[6:] for r in want], (off, lim)
        assert got[3] == members[m0:m0 + sum(r[3] for r in want)], (off, lim)
    parts = [_read(eng, M.query(order=order, offset=o, limit=1000)) for o in range(0, total, 1000)]
    assert [r[:5] + r[6:] for p in parts for r in p[2]] == [r[:5] + r[6:] for r in rows]
    assert [w for p in parts for w in p[3]] == members


def test_member_buffers(big):
    eng, total, full = big
    L, h = E.lib(), eng._h
    totals, by_config, rows, members = full[M.BY_ID_TEXT]
    q = np.zeros(1, dtype=E.gdir_query_dt)
    q[0] = (M.ALL_CONFIGS, 0, 0, M.NONE, 7, 7, M.BY_ID_TEXT, 10, 20)
    want = rows[10:30]
    n_mem = sum(r[3] for r in want)
    t = np.zeros(1, dtype=E.gdir_totals_dt)
    buf, n, nm = np.zeros(20, dtype=E.gdir_row_dt), E.C.c_uint32(77), E.C.c_uint32(77)
    mem = np.full(n_mem, 0xABABABAB, dtype=np.uint32)
    # members NULL: the rows come, *n_members is written
    assert L.pm_group_directory(h, q.ctypes.data, t.ctypes.data, None, 0, buf.ctypes.data, 20, E.C.byref(n), None, 0, E.C.byref(nm)) == 0
    assert (n.value, nm.value) == (20, n_mem) and [r[:5] + r[6:] for r in _tuples(buf)] == [r[:5] + r[6:] for r in want]
    assert [r[5] for r in _tuples(buf)] == [r[5] - want[0][5] for r in want]
    # cap_members one short: PM_ERANGE, the counts written, no row and no member copied
    buf[:] = 0
    rc = L.pm_group_directory(h, q.ctypes.data, t.ctypes.data, None, 0, buf.ctypes.data, 20, E.C.byref(n), mem.ctypes.data, n_mem - 1,
                              E.C.byref(nm))
    assert rc == ERANGE and (n.value, nm.value) == (20, n_mem) and not buf.view(np.uint8).any() and (mem == 0xABABABAB).all()
    assert int(t[0]["total"]) == total
    rc = L.pm_group_directory(h, q.ctypes.data, t.ctypes.data, None, 0, buf.ctypes.data, 20, E.C.byref(n), mem.ctypes.data, n_mem,
                              E.C.byref(nm))
    assert rc == 0 and mem.tolist() == members[want[0][5]:want[0][5] + n_mem]


# ------------------------------------------------------------------ the life cycle

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
    return cs, packed, eng


def _life_queries(n_cfgs):
    return [M.query(), M.query(order=M.BY_ID_TEXT), M.query(order=M.BY_SIZE_DESC, health_mask=LOST_OR_DEGRADED),
            M.query(order=M.BY_ID_TEXT, rollout_mask=1 << M.GR_ROLLING, offset=1, limit=20),
            M.query(config_mask=((1 << n_cfgs) - 2) or 1, holds=M.WITH_TASK, limit=0)]


def test_reads_follow_the_life_cycle():
    cs, packed, eng = _churn_engine(3)
    pick = lambda idx: {k: np.ascontiguousarray(v[idx]) for k, v in packed.items()}
    ranks, uids = packed["addr_rank"], cs.uid.tolist()
    LQ = _life_queries(eng.C)
    eng.liveness_enable(True)
    eng.rollout_enable(True)
    rng = np.random.default_rng(11)
    _check(eng, ranks[:cs.W], uids, LQ, "before a tick: no groups")
    eng.tick()
    state, _ = _check(eng, ranks[:cs.W], uids, LQ, "behind a tick: the pending groups are taken in")
    assert len(state[0]) > 3
    eng.liveness_set(np.arange(cs.W, dtype=np.uint32), np.where(rng.random(cs.W) < 0.7, M.HEALTHY, rng.integers(0, M.NS_N, cs.W)).astype(np.uint8),
                     np.zeros(cs.W, dtype=np.uint32))
    eng.rollout_ingest(_reports([(w, M.RUNNING, int(uids[rng.integers(0, 3)])) for w in range(0, cs.W, 2)]))
    for k in range(2):
        leave, idx_new, new_tasks = cs.step()
        eng.on_worker_status_many(leave, np.zeros(len(leave), dtype=np.uint32), np.ones(len(leave), dtype=np.uint32))
        _check(eng, ranks[:cs.W - len(idx_new)], uids, LQ, "dead workers: their groups dissolve, tombstones stay in the list")
        eng.append_workers(pick(idx_new))
        _check(eng, ranks[:cs.W], uids, LQ, "appended rows")
        eng.tasks_insert_front(*new_tasks[:3])
        uids = new_tasks[2].tolist() + uids
        _check(eng, ranks[:cs.W], uids, LQ, "insert_front: claimed positions move")
        eng.tick()
        _check(eng, ranks[:cs.W], uids, LQ, f"churn {k}")
    state, _ = _check(eng, ranks[:cs.W], uids, LQ, "again")
    victim = [uids[t] for _, _, _, t in state[0] if t >= 0][0]
    eng.tasks_delete(np.array([victim], dtype=np.uint64))                   # a claimed task goes and takes its groups with it
    uids.remove(victim)
    state2, _ = _check(eng, ranks[:cs.W], uids, LQ, "after pm_tasks_delete")
    assert len(state2[0]) < len(state[0])
    assert eng.dissolve_group_by_id(state2[0][1][0])
    state3, _ = _check(eng, ranks[:cs.W], uids, LQ, "after pm_dissolve_group_by_id")
    assert len(state3[0]) == len(state2[0]) - 1
    eng.close()


def test_reads_follow_a_merge():
    W = 40
    rng = np.random.default_rng(4)
    eng = E.Engine(group_id_seed=5)
    cfg_rows, alt_rows, _ = host.pack_configs([("solo", 1, 1, None), ("merge", 2, 4, None)])
    eng.set_configs(cfg_rows, alt_rows)
    eng.upload_workers(_cols(W))
    eng.upload_tasks(np.full(2, 3, dtype=np.uint64), np.array([2, 1], dtype=np.int64), np.array([11, 12], dtype=np.uint64))
    ids = GC.distinct_ids(12, rng)
    g = np.zeros(12, dtype=E.group_dt)
    for k in range(12):
        g[k] = (ids[k], 0, 1, k, M.NONE)                                    # twelve solo groups
    eng.adopt_groups(g, np.arange(12, dtype=np.uint32), 77)
    eng.liveness_enable(True)
    eng.rollout_enable(True)
    qs = _every_query(True, True, 2)
    before, _ = _check(eng, range(W), [11, 12], qs, "solo groups")
    assert eng.merge_solo_groups() > 0
    after, got = _check(eng, range(W), [11, 12], qs, "merged")
    assert len(after[0]) < len(before[0]) and max(r[3] for r in got[0][2]) > 1
    eng.close()


def test_reads_after_both_uploads():
    rng = np.random.default_rng(6)
    groups, W = _even_groups(70, rng, 2)
    statuses, reports = _random_ledgers(W, rng)
    eng = _engine(W, groups, 2, np.arange(W)[::-1], statuses, reports)
    qs = _every_query(True, True, 2)
    before, _ = _check(eng, np.arange(W)[::-1], TASKS, qs, "adopted")
    more = np.concatenate([np.arange(W)[::-1], np.arange(W, W + 40)])
    eng.upload_workers(_cols(W + 40, ranks=more), keep_groups=True)
    state, _ = _check(eng, more, TASKS, qs, "upload keeping the groups: groups and ledgers stay")
    assert state[0] == before[0] and state[1][:W] == before[1]
    eng.upload_workers(_cols(W + 40, ranks=more), keep_groups=False)
    state, got = _check(eng, more, TASKS, qs, "upload dropping the groups")
    assert not state[0] and got[0][0][:2] == (0, 0)
    eng.close()


# ------------------------------------------------------------------ errors

def test_errors_leave_everything_as_it_was():
    rng = np.random.default_rng(9)
    groups, W = _even_groups(50, rng, 3)
    statuses, reports = _random_ledgers(W, rng)
    eng = _engine(W, groups, 3, None, statuses, reports)
    L, h = E.lib(), eng._h
    good = M.query(order=M.BY_ID_TEXT, offset=2, limit=30)
    before = _read(eng, good)
    assert len(before[2]) == 30
    n_mem = len(before[3])

    def call(q, totals=True, n=True, nm=True, rows=None, cap=0, cfgs=True, cap_cfgs=64, mem=None, cap_mem=0):
        qa = np.zeros(1, dtype=E.gdir_query_dt)
        if q is not None:
            qa[0] = tuple(q[k] for k in ("config_mask", "holds", "size_min", "size_max", "health_mask", "rollout_mask", "order",
                                         "offset", "limit"))
        t = np.full(9, 77, dtype=np.uint32)
        nn, mm, c = E.C.c_uint32(77), E.C.c_uint32(77), np.full(64, 77, dtype=np.uint32)
        rc = L.pm_group_directory(h, qa.ctypes.data if q is not None else None, t.ctypes.data if totals else None,
                                  c.ctypes.data if cfgs else None, cap_cfgs, rows, cap, E.C.byref(nn) if n else None, mem, cap_mem,
                                  E.C.byref(mm) if nm else None)
        return rc, t.tolist(), nn.value, mm.value, c.tolist()

    def unchanged():
        assert _read(eng, good) == before

    untouched = (EINVAL, [77] * 9, 77, 77, [77] * 64)
    assert call(None) == untouched and call(good, totals=False)[0] == EINVAL and call(good, n=False)[0] == EINVAL
    assert call(good, nm=False)[0] == EINVAL
    assert L.pm_group_directory(None, None, None, None, 0, None, 0, None, None, 0, None) == EINVAL
    for bad in (dict(good, config_mask=0), dict(good, health_mask=0), dict(good, health_mask=8), dict(good, health_mask=7 | (1 << 31)),
                dict(good, rollout_mask=0), dict(good, rollout_mask=1 << M.GR_N), dict(good, holds=3), dict(good, holds=0xFFFFFFFF),
                dict(good, order=3), dict(good, order=0xFFFFFFFF), dict(good, size_min=5, size_max=4)):
        assert call(bad) == untouched, bad
    unchanged()
    t_want = [before[0][0], before[0][1], *before[0][2], *before[0][3], 3]
    c_want = before[1] + [77] * 61
    # the size query, short buffers, a NULL row buffer: totals, by_config and the counts written, nothing copied
    buf = np.zeros(30, dtype=E.gdir_row_dt)
    assert call(good) == (ERANGE, t_want, 30, n_mem, c_want)
    assert call(good, rows=buf.ctypes.data, cap=29) == (ERANGE, t_want, 30, n_mem, c_want) and not buf.view(np.uint8).any()
    assert call(good, rows=None, cap=1 << 20)[0] == ERANGE
    assert call(good, rows=buf.ctypes.data, cap=30, cap_cfgs=2) == (ERANGE, t_want, 30, n_mem, [77] * 64) and not buf.view(np.uint8).any()
    assert call(good, rows=buf.ctypes.data, cap=30, cfgs=False) == (0, t_want, 30, n_mem, [77] * 64)
    assert [r[:5] + r[6:] for r in _tuples(buf)] == [r[:5] + r[6:] for r in before[2]]
    assert call(dict(good, limit=0)) == (0, t_want, 0, 0, c_want)                             # the counters-only query
    assert call(dict(good, offset=before[0][0])) == (0, t_want, 0, 0, c_want)
    unchanged()
    # a class filter whose ledger is off; the "all" mask passes
    eng.rollout_enable(False)
    assert call(dict(good, rollout_mask=1 << M.GR_ROLLING)) == (ESTATE, [77] * 9, 77, 77, [77] * 64)
    assert call(dict(good, limit=0))[0] == 0
    eng.liveness_enable(False)
    assert call(dict(good, health_mask=LOST_OR_DEGRADED))[0] == ESTATE
    _check(eng, range(W), TASKS, [good, M.query()], "both ledgers off")
    eng.dist_configure(0, 2, np.zeros(W, dtype=np.uint8))                   # a multi-GPU engine (it refuses the ledgers, so: here)
    assert call(good) == (ESTATE, [77] * 9, 77, 77, [77] * 64)
    eng.dist_configure(0, 1)
    eng.liveness_enable(True)
    eng.liveness_set(np.arange(W, dtype=np.uint32), np.asarray(statuses, dtype=np.uint8), np.zeros(W, dtype=np.uint32))
    eng.rollout_enable(True)
    eng.rollout_ingest(_reports(reports))
    unchanged()
    # a stepwise tick in progress
    eng.dist_configure(0, 1)
    eng.dist_tick_begin()
    assert call(good) == (ESTATE, [77] * 9, 77, 77, [77] * 64)
    eng.dist_carve_wait()
    eng.dist_match_begin()
    eng.dist_tick_end()
    _check(eng, range(W), TASKS, [good, M.query()], "behind the stepwise tick")
    eng.close()
    # no configurations, no workers; an empty table is a table
    eng = E.Engine()
    with pytest.raises(E.EngineError) as ei:
        eng.group_directory()
    assert ei.value.code == ESTATE
    cfg_rows, alt_rows, _ = host.pack_configs([("any", 1, 8, None)])
    eng.set_configs(cfg_rows, alt_rows)
    with pytest.raises(E.EngineError) as ei:
        eng.group_directory()
    assert ei.value.code == ESTATE
    eng.upload_workers(_cols(0))
    totals, by_config, rows, members = eng.group_directory()
    assert int(totals["total"]) == 0 and int(totals["n_cfgs"]) == 1 and by_config.tolist() == [0] and not len(rows) and not len(members)
    eng.close()


# ------------------------------------------------------------------ what the directory leaves alone, determinism

def _feed(eng):
    for q in _life_queries(eng.C) + [M.query(order=M.BY_SIZE_DESC)]:
        _read(eng, q)


def test_the_group_directory_leaves_the_engine_alone():
    """two engines fed identically, one of them also asked the directory between every step: the groups, the published rows,
    pm_last_stats' counters and the ledgers end bit-identical, and the engines give back what they took.  The counters compared
    are the ones that are a function of the engine's state (n_groups, n_formed, n_merged, carve_steps, pair_evals): `proposals`,
    fast steps, launches and candidates scanned count how the streaming carve's row makers and its validator met in time and
    differ between two runs of ONE engine (tests/test_gpu_metrics.py says so of the same comparison), so they say nothing here.
    The allocations are read behind gc.collect(), as tests/test_gpu_lifetime.py reads them: an engine that an earlier test
    dropped without closing is freed whenever the collector runs, and must not be freed between the two readings."""
    gc.collect()
    base = E.Engine.debug_live_allocations()
    (ca, pa, a), (cb, pb, b) = _churn_engine(2, W0=600), _churn_engine(2, W0=600)
    for eng in (a, b):
        eng.liveness_enable(True)
        eng.rollout_enable(True)

    def image(eng):
        return b"".join(np.asarray(x).tobytes() for x in (*eng.liveness_get(), *eng.rollout_get(), *eng.get_groups()))

    counters = ("n_groups", "n_formed", "n_merged", "carve_steps", "pair_evals")
    _feed(a)
    sa, sb = a.tick(), b.tick()
    assert {c: sa[c] for c in counters} == {c: sb[c] for c in counters}
    _feed(a)                                                                # behind the tick, before anything took its groups in
    la, lb = a.last_stats(), b.last_stats()
    assert {c: la[c] for c in counters} == {c: lb[c] for c in counters}
    assert engine_groups(a) == engine_groups(b)
    for k in range(3):
        (la, ia, ta), (lb, ib, tb) = ca.step()[:3], cb.step()[:3]
        for eng, packed, leave, idx_new, new_tasks in ((a, pa, la, ia, ta), (b, pb, lb, ib, tb)):
            eng.on_worker_status_many(leave, np.zeros(len(leave), dtype=np.uint32), np.ones(len(leave), dtype=np.uint32))
            if eng is a:
                _feed(a)                                                    # (dissolved groups still in the list)
            eng.append_workers({kk: np.ascontiguousarray(v[idx_new]) for kk, v in packed.items()})
            if eng is a:
                _feed(a)
            eng.tasks_insert_front(*new_tasks[:3])
            eng.rollout_ingest(_reports([(int(w), 2, 5) for w in idx_new]))
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
        for q in _every_query(True, True, eng.C) + [M.query(order=M.BY_ID_TEXT, offset=5, limit=77)]:
            t, by_config, rows, members = eng.group_directory(q["config_mask"], q["holds"], q["size_min"], q["size_max"],
                                                              q["health_mask"], q["rollout_mask"], q["order"], q["offset"],
                                                              None if q["limit"] == M.TO_END else q["limit"])
            out.append(t.tobytes() + by_config.tobytes() + rows.tobytes() + members.tobytes())
        return b"".join(out)

    W = 2 * RO_CHUNK + 513
    _, eng = _swarm_engine(W, seed=9)
    first = image(eng)
    assert image(eng) == first                                              # the same state read twice
    eng.liveness_get(), eng.rollout_summary(), eng.directory(limit=5), eng.rollout_groups()
    assert image(eng) == first                                              # and after unrelated reads
    _, one = _swarm_engine(W, seed=9, carve_wgs=1)                          # the same swarm carved by one workgroup, and by many
    _, many = _swarm_engine(W, seed=9, carve_wgs=64)
    assert image(one) == first and image(many) == first
    eng.close(), one.close(), many.close()
