"""The node directory on the GPU (pm_directory of include/pm_engine.h, kernels in pm_directory.inc) against the model of
tests/directory_model.py, which tests/test_directory_model.py holds to the reference and to the named cases: every named case
through the C ABI, seeded swarms behind a real pm_tick at every tile edge of the scan and the sort, windows, the rank edges of the
sort, the life cycle, every error, what the call leaves alone, and determinism.  Every comparison is exact."""
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

import directory_cases as DC
import directory_model as M

pytestmark = pytest.mark.gpu
EINVAL, ESTATE, ERANGE = -1, -4, -5
ON = E.W_HEALTHY | E.W_HAS_P2P
MASKS = (M.ALL, M.NOT_DEAD, 1 << M.DISCOVERED)


def _device_constants():
    """the tile sizes the scan and the sort work in, read from the device source: a change there moves the swarm sizes below"""
    dev = open(os.path.join(B.CSRC, "pm_device.h")).read()
    chunk = int(re.search(r"\bPM_RO_CHUNK\s*=\s*(\d+)", dev).group(1))
    kernels = open(os.path.join(B.CSRC, "pm_metrics.inc")).read()
    scan = kernels[kernels.index("void mx_scan_kernel("):kernels.index("void mx_copy_kernel(")]
    tile = int(re.search(r"base \+= (\d+)u", scan).group(1))
    src = open(os.path.join(B.CSRC, "pm_directory.inc")).read()
    block = {int(x) for x in re.findall(r"__launch_bounds__\((\d+)\)", src)}
    return chunk, tile, block


RO_CHUNK, SCAN_TILE, BLOCKS = _device_constants()
SWARM_W = sorted({1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, RO_CHUNK + 1, SCAN_TILE + 1} | {b + 1 for b in BLOCKS})


def _cols(n, flags=ON, ranks=None):
    z = np.zeros(n, dtype=np.uint32)
    c = dict(flags=np.full(n, flags, dtype=np.uint32), gpu_count=z, gpu_mem_mb=z, gpu_model_class=z, cpu_cores=z, ram_mb=z,
             storage_gb=z, price=z, lat=np.zeros(n), lon=np.zeros(n))
    if ranks is not None:
        c["addr_rank"] = np.asarray(ranks, dtype=np.uint32)
    return c


def _code(call):
    with pytest.raises(E.EngineError) as ei:
        call()
    return ei.value.code


def _tuples(rows):
    """dir_row_dt -> the model's rows (padding must be zero)"""
    assert not rows["_pad"].any() and not rows["_pad2"].any()
    return [(int(r["worker"]), int(r["status"]), int(r["cls"]), int(r["state"]), int(r["counter"]), int(r["group_slot"]),
             int(r["group_id"]), int(r["group_size"]), int(r["config"]), int(r["task"]), int(r["uid"])) for r in rows]


def _read(eng, q):
    total, counts, rows = eng.directory(q["status_mask"], q["membership"], q["order"], q["offset"],
                                        None if q["limit"] == M.TO_END else q["limit"])
    return total, counts.tolist(), _tuples(rows)


def _state(eng, ranks, uids):
    """the model's inputs from the engine's other reads: the ledgers, pm_get_groups"""
    st, cnt = eng.liveness_get()
    group_of, _, _ = eng.get_groups()
    ledger = None
    try:
        uid, state = eng.rollout_get()
        ledger = list(zip(uid.tolist(), state.tolist()))
    except E.EngineError as err:
        assert err.code == ESTATE                                           # the rollout ledger is off
    return st.tolist(), cnt.tolist(), group_of.tolist(), engine_groups(eng), list(uids), ledger, list(ranks)


def _check(eng, ranks, uids, queries, tag=""):
    """the directory FIRST (pm_get_groups compacts the list: the directory must number the slots over the tombstones), then the
    model over what the other reads give"""
    got = [_read(eng, q) for q in queries]
    state = _state(eng, ranks, uids)
    for q, g in zip(queries, got):
        want = M.directory(*state, q)
        assert g[0] == want[0] and g[1] == want[1], (tag, q)
        assert g[2] == want[2], (tag, q)
    return state


def _every_query():
    return [M.query(status_mask=m, membership=mem, order=o) for o in (M.BY_ROW, M.BY_ADDRESS)
            for mem in (M.ANY, M.GROUPED, M.UNGROUPED) for m in MASKS]


def _set_statuses(eng, statuses, counters):
    W = len(statuses)
    eng.liveness_set(np.arange(W, dtype=np.uint32), np.asarray(statuses, dtype=np.uint8), np.asarray(counters, dtype=np.uint32))


def _reports(rows):
    out = np.zeros(len(rows), dtype=E.ro_report_dt)
    for k, (w, st, uid) in enumerate(rows):
        out[k] = (w, st, uid)
    return out


# ------------------------------------------------------------------ the named cases

def _case_engine(case):
    run = DC.Run(case)
    eng = E.Engine(group_id_seed=3)
    cfg_rows, alt_rows, _ = host.pack_configs([("any", 1, 8, None)])
    eng.set_configs(cfg_rows, alt_rows)
    eng.upload_workers(_cols(run.W, ranks=run.ranks))
    T = len(case["tasks"])
    eng.upload_tasks(np.full(T, 1, dtype=np.uint64), np.arange(T, 0, -1).astype(np.int64), np.array(case["tasks"], dtype=np.uint64))
    g = np.zeros(len(case["groups"]), dtype=E.group_dt)
    members = []
    for k, (mem, t) in enumerate(case["groups"]):
        g[k] = (0x6000 + k, 0, len(mem), len(members), M.NONE if t < 0 else t)
        members += sorted(mem)
    if len(g):
        eng.adopt_groups(g, np.array(members, dtype=np.uint32), 99)
    if case.get("delete"):
        eng.tasks_delete(np.array(case["delete"], dtype=np.uint64))
    eng.liveness_enable(True)
    _set_statuses(eng, run.statuses, run.counters)
    if case["reports"] is not None:
        eng.rollout_enable(True)
        eng.rollout_ingest(_reports(case["reports"]))
    return eng, run


@pytest.mark.parametrize("case", DC.CASES, ids=[c["name"] for c in DC.CASES])
def test_named_cases_through_the_c_abi(case):
    eng, run = _case_engine(case)
    for q, total, workers in case["queries"]:
        got, want = _read(eng, q), run.read(q)
        assert got == (want[0], want[1], want[2]), q
        assert got[0] == total and [r[0] for r in got[2]] == workers, q
    state = _check(eng, run.ranks, run.task_uids, [q for q, _, _ in case["queries"]] + _every_query(), case["name"])
    assert state[2] == run.group_of and state[3] == run.groups and state[5] == run.ledger
    eng.close()


# ------------------------------------------------------------------ seeded swarms behind a real tick

def _swarm_engine(W, seed=None, rollout=True):
    sw = make_swarm(100 + W if seed is None else seed, 24, W)
    eng = E.Engine(group_id_seed=7)
    host.load_swarm(eng, sw)
    eng.liveness_enable(True)
    if rollout:
        eng.rollout_enable(True)
    eng.tick()
    rng = np.random.default_rng(W)
    statuses = rng.integers(0, M.NS_N, W)
    counters = rng.integers(0, 1 << 32, W, dtype=np.uint64).astype(np.uint32)
    _set_statuses(eng, statuses, counters)
    if rollout:
        uids = sw.task_uid.tolist()
        reps = [(int(w), int(rng.integers(0, E.TS_N)), int(uids[rng.integers(0, len(uids))]) if rng.random() < 0.7
                 else int(rng.integers(1, 1 << 63))) for w in range(W) if rng.random() < 0.6]
        eng.rollout_ingest(_reports(reps))
    return sw, eng, statuses


@pytest.mark.parametrize("W", SWARM_W)
def test_seeded_swarms_behind_a_real_tick(W):
    sw, eng, statuses = _swarm_engine(W)
    ranks = sw.addr_rank().tolist()
    state = _check(eng, ranks, sw.task_uid.tolist(), _every_query(), W)
    assert state[0] == statuses.tolist()
    if W >= 255:
        assert any(g >= 0 for g in state[2]) and any(g < 0 for g in state[2])                 # grouped rows and free ones
        assert any(t >= 0 for _, _, _, t in state[3])                                          # a claim
        assert len(set(state[0])) == M.NS_N                                                    # every status
    eng.close()


# ------------------------------------------------------------------ windows

@pytest.fixture(scope="module")
def big():
    """a 4,097-row swarm behind a tick, every status present; its unpaged lists and the model's inputs, computed once"""
    W = 4097
    assert W > SCAN_TILE and W > 4 * RO_CHUNK
    sw, eng, _ = _swarm_engine(W)
    ranks = sw.addr_rank().tolist()
    state = _check(eng, ranks, sw.task_uid.tolist(), [M.query(), M.query(order=M.BY_ADDRESS)], "big")
    full = {o: _read(eng, M.query(order=o)) for o in (M.BY_ROW, M.BY_ADDRESS)}
    yield eng, state, full
    eng.close()


@pytest.mark.parametrize("order", [M.BY_ROW, M.BY_ADDRESS])
def test_windows_at_every_edge(big, order):
    eng, state, full = big
    total, counts, rows = full[order]
    assert total == 4097 and len(rows) == total
    cls = [r[2] for r in rows]
    assert cls == sorted(cls) and set(cls) == set(range(M.DC_N))
    last = {c: max(i for i, x in enumerate(cls) if x == c) for c in range(M.DC_N)}             # a class's last row
    windows = [(0, 1), (total - 1, 1), (total, 5), (total + 1, 5), (7, M.TO_END), (total - 1, M.TO_END), (0, 0), (5, 0),
               (SCAN_TILE - 3, 7), (RO_CHUNK - 3, 7), (SCAN_TILE // 4 - 3, 7), (0xFFFFFFFF, 0xFFFFFFFF), (3, 0xFFFFFFFE)]
    for c in range(M.DC_N):
        windows += [(last[c] - 4, 5), (last[c], 5), (last[c], 1), (last[c] + 1, 3), (last[c] - 1, 3)]
    for off, lim in windows:
        got = _read(eng, M.query(order=order, offset=off, limit=lim))
        first, n = M.window(total, off, lim)
        assert got == (total, counts, rows[first:first + n]), (off, lim)
    for page in (1, 64, 1000):
        offs = range(0, total, page) if page > 1 else list(range(0, 130)) + list(range(total - 3, total))
        parts = [_read(eng, M.query(order=order, offset=o, limit=page)) for o in offs]
        assert all(p[0] == total and p[1] == counts for p in parts)
        joined = [r for p in parts for r in p[2]]
        assert joined == (rows if page > 1 else rows[:130] + rows[total - 3:]), page


def test_filtered_windows_against_the_model(big):
    eng, state, full = big
    for q in (M.query(status_mask=M.NOT_DEAD, membership=M.GROUPED, order=M.BY_ADDRESS, offset=100, limit=50),
              M.query(status_mask=1 << M.DISCOVERED, order=M.BY_ADDRESS, offset=3, limit=M.TO_END),
              M.query(status_mask=(1 << M.DEAD) | (1 << M.HEALTHY), membership=M.UNGROUPED, offset=50, limit=1000),
              M.query(status_mask=1 << M.BANNED, limit=0)):
        want = M.directory(*state, q)
        assert _read(eng, q) == (want[0], want[1], want[2]), q


# ------------------------------------------------------------------ BY_ADDRESS: the sort's rank edges

def _plain(W, ranks=None, statuses=None, group_size=0):
    eng = E.Engine(group_id_seed=3)
    cfg_rows, alt_rows, _ = host.pack_configs([("any", 1, 8, None)])
    eng.set_configs(cfg_rows, alt_rows)
    return _fill(eng, W, ranks, statuses, group_size)


def _fill(eng, W, ranks=None, statuses=None, group_size=0):
    """a table of W rows (the upload drops what the engine held), three tasks, groups over the first half, the statuses"""
    eng.upload_workers(_cols(W, ranks=ranks))
    eng.upload_tasks(np.full(3, 1, dtype=np.uint64), np.array([3, 2, 1], dtype=np.int64), np.array([11, 12, 13], dtype=np.uint64))
    if group_size:
        n = W // (2 * group_size)
        g = np.zeros(n, dtype=E.group_dt)
        for k in range(n):
            g[k] = (0x9000 + k, 0, group_size, k * group_size, k % 4 if k % 4 < 3 else M.NONE)
        eng.adopt_groups(g, np.arange(n * group_size, dtype=np.uint32), 5)
    eng.liveness_enable(True)
    if statuses is not None:
        _set_statuses(eng, statuses, np.arange(W))
    return eng


W_SORT = 2 * RO_CHUNK + 77
SORT_QUERIES = [M.query(order=M.BY_ADDRESS), M.query(order=M.BY_ADDRESS, status_mask=M.NOT_DEAD, offset=RO_CHUNK - 5, limit=40),
                M.query(order=M.BY_ROW)]


def _rank_sets():
    rng = np.random.default_rng(8)
    digit = rng.integers(0, 256, W_SORT).astype(np.uint64)
    sets = {"a_permutation": rng.permutation(W_SORT), "all_equal": np.full(W_SORT, 0x01020304),
            "all_zero": np.zeros(W_SORT), "all_ones": np.full(W_SORT, 0xFFFFFFFF),
            "descending": np.arange(W_SORT)[::-1], "few_values": rng.integers(0, 3, W_SORT) * 0x7FFFFFFF}
    for k in range(4):                                   # only byte k differs: a pass that skipped it would leave them unsorted
        sets[f"only_byte_{k}"] = (np.uint64(0x55555555) & ~np.uint64(0xFF << (8 * k))) | (digit << np.uint64(8 * k))
    return {k: np.asarray(v, dtype=np.uint64).astype(np.uint32) for k, v in sets.items()}


RANKS = _rank_sets()


@pytest.mark.parametrize("name", list(RANKS))
def test_by_address_rank_edges(name):
    ranks = RANKS[name]
    statuses = np.random.default_rng(3).integers(0, M.NS_N, W_SORT)
    eng = _plain(W_SORT, ranks, statuses, group_size=3)
    _check(eng, ranks.tolist(), [11, 12, 13], SORT_QUERIES, name)
    total, _, rows = _read(eng, M.query(order=M.BY_ADDRESS))
    keys = [(r[2], int(ranks[r[0]]), r[0]) for r in rows]
    assert total == W_SORT and keys == sorted(keys)
    eng.close()


def test_one_engine_across_index_space_sizes():
    """One engine; the table 65 rows, then the smallest whose sort histogram takes two tiles of the scan, then 65 again, then the
    smallest with two chunks (the sizes as tests/test_gpu_addresses.py takes them from the source).  At each size the sorted order,
    whole and a window, and a page in scan order between them and the next size's.  The scratch keeps what the largest size
    made it: a buffer sized for an earlier n, or the wrong result buffer behind the sort's five passes, is a list that is not
    the model's."""
    two_chunks, two_tiles = RO_CHUNK + 1, (SCAN_TILE // 256) * RO_CHUNK + 1
    assert SCAN_TILE % 256 == 0 and 256 * -(-two_tiles // RO_CHUNK) > SCAN_TILE >= 256 * -(-(two_tiles - 1) // RO_CHUNK)
    eng = E.Engine(group_id_seed=3)
    cfg_rows, alt_rows, _ = host.pack_configs([("any", 1, 8, None)])
    eng.set_configs(cfg_rows, alt_rows)
    for step, W in enumerate((65, two_tiles, 65, two_chunks)):
        rng = np.random.default_rng(40 + step)
        ranks = rng.integers(0, 1 << 32, W, dtype=np.uint64).astype(np.uint32)
        _fill(eng, W, ranks, rng.integers(0, M.NS_N, W), group_size=3)
        qs = [M.query(order=M.BY_ADDRESS), M.query(order=M.BY_ROW, offset=W // 2, limit=40),
              M.query(order=M.BY_ADDRESS, status_mask=M.NOT_DEAD, offset=W // 3, limit=40), M.query(order=M.BY_ROW)]
        state = _check(eng, ranks.tolist(), [11, 12, 13], qs, (step, W))
        assert len(state[0]) == W and len(set(state[0])) == M.NS_N
    eng.close()


def test_by_address_follows_rewritten_ranks():
    W = RO_CHUNK + 300
    rng = np.random.default_rng(12)
    ranks = rng.permutation(W).astype(np.uint32)
    statuses = rng.integers(0, M.NS_N, W)
    eng = _plain(W, ranks, statuses, group_size=2)
    q = [M.query(order=M.BY_ADDRESS), M.query(order=M.BY_ADDRESS, offset=500, limit=100)]
    _check(eng, ranks.tolist(), [11, 12, 13], q, "uploaded")
    idx = rng.choice(W, 200, replace=False).astype(np.uint32)
    cols = _cols(len(idx), ranks=rng.integers(0, 1 << 32, len(idx), dtype=np.uint64).astype(np.uint32))
    eng.update_workers(idx, cols)
    ranks[idx] = cols["addr_rank"]
    _check(eng, ranks.tolist(), [11, 12, 13], q, "pm_update_workers")
    ranks = ranks[::-1].copy()
    eng.set_addr_ranks(ranks)
    _check(eng, ranks.tolist(), [11, 12, 13], q, "pm_set_addr_ranks")
    first = eng.append_workers(_cols(5, ranks=[7, 7, 0, 0xFFFFFFFF, 7]))
    assert first == W
    ranks = np.concatenate([ranks, np.array([7, 7, 0, 0xFFFFFFFF, 7], dtype=np.uint32)])
    _check(eng, ranks.tolist(), [11, 12, 13], q + [M.query()], "appended with ranks")
    first = eng.append_workers(_cols(3))                                    # without ranks: the row index
    ranks = np.concatenate([ranks, np.arange(first, first + 3, dtype=np.uint32)])
    _check(eng, ranks.tolist(), [11, 12, 13], q + [M.query()], "appended without ranks")
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


LIFE_QUERIES = [M.query(), M.query(order=M.BY_ADDRESS), M.query(status_mask=M.NOT_DEAD, membership=M.GROUPED, order=M.BY_ADDRESS),
                M.query(membership=M.UNGROUPED, offset=3, limit=40)]


def test_reads_follow_the_life_cycle():
    cs, packed, eng = _churn_engine(3)
    pick = lambda idx: {k: np.ascontiguousarray(v[idx]) for k, v in packed.items()}
    ranks = packed["addr_rank"]
    uids = cs.uid.tolist()
    eng.liveness_enable(True)
    eng.rollout_enable(True)
    rng = np.random.default_rng(11)
    _check(eng, ranks[:cs.W], uids, LIFE_QUERIES, "before a tick")
    eng.tick()
    state = _check(eng, ranks[:cs.W], uids, LIFE_QUERIES, "behind a tick: the pending groups are taken in")
    assert any(g >= 0 for g in state[2])
    _set_statuses(eng, rng.integers(0, M.NS_N, cs.W), rng.integers(0, 99, cs.W))
    for k in range(2):
        leave, idx_new, new_tasks = cs.step()
        eng.on_worker_status_many(leave, np.zeros(len(leave), dtype=np.uint32), np.ones(len(leave), dtype=np.uint32))
        _check(eng, ranks[:cs.W - len(idx_new)], uids, LIFE_QUERIES, "dead workers: groups dissolve, the rows stay")
        eng.append_workers(pick(idx_new))
        state = _check(eng, ranks[:cs.W], uids, LIFE_QUERIES, "appended rows")
        assert all(g < 0 for g in state[2][cs.W - len(idx_new):])
        eng.tasks_insert_front(*new_tasks[:3])
        uids = new_tasks[2].tolist() + uids
        _check(eng, ranks[:cs.W], uids, LIFE_QUERIES, "insert_front: claimed positions move")
        eng.rollout_ingest(_reports([(int(w), 2, int(uids[0])) for w in idx_new]))
        eng.tick()
        _check(eng, ranks[:cs.W], uids, LIFE_QUERIES, f"churn {k}")
    # a sweep between two calls: the counters follow the census it returned
    beats = np.where(rng.random(cs.W) < 0.5, 1_000_000, 1).astype(np.uint64)
    n, census = eng.liveness_sweep(1_000_000 + E.LIVE_TTL_MS // 2, beats)
    total, counts, _ = eng.directory(limit=0)
    assert n > 0 and total == cs.W and counts.tolist() == census.tolist()
    state = _check(eng, ranks[:cs.W], uids, LIFE_QUERIES, "after pm_liveness_sweep")
    # a claimed task goes: its groups dissolve; then one more group by hand; the list holds tombstones while the directory reads it
    victim = [uids[t] for _, _, _, t in state[3] if t >= 0][0]
    eng.tasks_delete(np.array([victim], dtype=np.uint64))
    uids.remove(victim)
    eng.dissolve_group(0)
    state2 = _check(eng, ranks[:cs.W], uids, LIFE_QUERIES, "after pm_tasks_delete and pm_dissolve_group")
    assert len(state2[3]) < len(state[3]) - 1
    eng.close()


def test_reads_after_both_uploads():
    W = 130
    ranks = np.arange(W, dtype=np.uint32)[::-1].copy()
    eng = _plain(W, ranks, np.arange(W) % M.NS_N, group_size=2)
    eng.rollout_enable(True)
    eng.rollout_ingest(_reports([(w, w % E.TS_N, 11 + w % 3) for w in range(0, W, 2)]))
    before = _check(eng, ranks.tolist(), [11, 12, 13], LIFE_QUERIES, "adopted")
    more = np.concatenate([ranks, np.arange(W, W + 40, dtype=np.uint32)])
    eng.upload_workers(_cols(W + 40, ranks=more), keep_groups=True)
    state = _check(eng, more.tolist(), [11, 12, 13], LIFE_QUERIES, "upload keeping the groups: rows, groups and ledgers stay")
    assert state[0][:W] == before[0] and state[3] == before[3] and state[0][W:] == [M.HEALTHY] * 40
    eng.upload_workers(_cols(W + 40, flags=E.W_HAS_P2P, ranks=more), keep_groups=False)
    state = _check(eng, more.tolist(), [11, 12, 13], LIFE_QUERIES, "upload dropping the groups: every ledger starts over")
    assert not state[3] and set(state[0]) == {M.DISCOVERED} and state[5] == [(0, M.TS_NONE)] * (W + 40)
    eng.rollout_enable(False)
    total, counts, rows = eng.directory()
    assert total == W + 40 and not rows["uid"].any() and set(rows["state"].tolist()) == {M.TS_NONE}
    eng.close()


# ------------------------------------------------------------------ errors

def test_errors_leave_everything_as_it_was():
    W = 50
    eng = _plain(W, None, np.arange(W) % M.NS_N, group_size=3)
    L, h = E.lib(), eng._h
    good = M.query(order=M.BY_ADDRESS, offset=2, limit=30)
    before = _read(eng, good)
    assert len(before[2]) == 30

    def call(q, total=True, n=True, rows=None, cap=0, counts=True):
        qa = np.zeros(1, dtype=E.dir_query_dt)
        if q is not None:
            qa[0] = (q["status_mask"], q["membership"], q["order"], q["offset"], q["limit"])
        t, nn, c = E.C.c_uint32(77), E.C.c_uint32(77), np.full(M.NS_N, 77, dtype=np.uint32)
        rc = L.pm_directory(h, qa.ctypes.data if q is not None else None, E.C.byref(t) if total else None,
                            c.ctypes.data if counts else None, rows, cap, E.C.byref(nn) if n else None)
        return rc, t.value, nn.value, c.tolist()

    def unchanged():
        assert _read(eng, good) == before

    assert call(None)[0] == EINVAL and call(good, total=False)[0] == EINVAL and call(good, n=False)[0] == EINVAL
    assert L.pm_directory(None, None, None, None, None, 0, None) == EINVAL
    for bad in (dict(good, status_mask=0), dict(good, status_mask=1 << M.NS_N), dict(good, status_mask=M.ALL | (1 << 31)),
                dict(good, membership=3), dict(good, membership=0xFFFFFFFF), dict(good, order=2), dict(good, order=0xFFFFFFFF)):
        assert call(bad)[:3] == (EINVAL, 77, 77), bad
    unchanged()
    # the size query, a short buffer, a NULL buffer: *total, counts and *n_rows set, nothing copied; counts may be NULL
    buf = np.zeros(30, dtype=E.dir_row_dt)
    assert call(good) == (ERANGE, before[0], 30, before[1])
    assert call(good, rows=buf.ctypes.data, cap=29) == (ERANGE, before[0], 30, before[1]) and not buf.view(np.uint8).any()
    assert call(good, rows=None, cap=1 << 20)[0] == ERANGE
    assert call(good, rows=buf.ctypes.data, cap=30, counts=False)[:3] == (0, before[0], 30) and _tuples(buf) == before[2]
    assert call(dict(good, limit=0)) == (0, before[0], 0, before[1])                          # the counters-only query
    assert call(dict(good, offset=before[0])) == (0, before[0], 0, before[1])
    unchanged()
    # a stepwise tick in progress
    eng.dist_configure(0, 1)
    eng.dist_tick_begin()
    assert _code(eng.directory) == ESTATE
    eng.dist_carve_wait()
    eng.dist_match_begin()
    eng.dist_tick_end()
    _check(eng, range(W), [11, 12, 13], [good, M.query()], "behind the stepwise tick")    # (it was a tick: the free rows are grouped now)
    before = _read(eng, good)
    # liveness off; a multi-GPU engine
    eng.liveness_enable(False)
    assert _code(eng.directory) == ESTATE and call(good)[:3] == (ESTATE, 77, 77)
    eng.dist_configure(0, 2, np.zeros(W, dtype=np.uint8))
    assert _code(eng.directory) == ESTATE
    eng.dist_configure(0, 1)
    eng.liveness_enable(True)
    _set_statuses(eng, np.arange(W) % M.NS_N, np.arange(W))
    unchanged()
    eng.close()
    # no workers uploaded; an empty table is a table
    eng = E.Engine()
    eng.liveness_enable(True)
    assert _code(eng.directory) == ESTATE
    eng.upload_workers(_cols(0))
    total, counts, rows = eng.directory()
    assert total == 0 and not counts.any() and not len(rows)
    eng.close()


# ------------------------------------------------------------------ what the directory leaves alone, determinism

def test_the_directory_leaves_the_ledgers_and_the_tick_alone():
    """the same churn with directory calls between the ticks and without: the ledgers byte for byte around a call, the groups of
    every tick the same on both sides"""
    (ca, pa, a), (cb, pb, b) = _churn_engine(2, W0=600), _churn_engine(2, W0=600)
    for eng in (a, b):
        eng.liveness_enable(True)
        eng.rollout_enable(True)

    def image(eng):
        return b"".join(np.asarray(x).tobytes() for x in (*eng.liveness_get(), *eng.rollout_get(), *eng.get_groups()))

    def feed():
        for q in LIFE_QUERIES:
            a.directory(q["status_mask"], q["membership"], q["order"], q["offset"], None if q["limit"] == M.TO_END else q["limit"])

    feed()
    sa, sb = a.tick(), b.tick()
    counters = ("n_groups", "n_formed", "n_merged")
    assert {c: sa[c] for c in counters} == {c: sb[c] for c in counters}
    feed()                                                                  # behind the tick, before anything took its groups in
    assert engine_groups(a) == engine_groups(b)
    for k in range(3):
        (la, ia, ta), (lb, ib, tb) = ca.step()[:3], cb.step()[:3]
        for eng, packed, leave, idx_new, new_tasks in ((a, pa, la, ia, ta), (b, pb, lb, ib, tb)):
            eng.on_worker_status_many(leave, np.zeros(len(leave), dtype=np.uint32), np.ones(len(leave), dtype=np.uint32))
            eng.append_workers({kk: np.ascontiguousarray(v[idx_new]) for kk, v in packed.items()})
            eng.tasks_insert_front(*new_tasks[:3])
            eng.rollout_ingest(_reports([(int(w), 2, 5) for w in idx_new]))
            if eng is a:
                feed()                                                      # (dissolved groups still in the list)
        sa, sb = a.tick(), b.tick()
        assert {c: sa[c] for c in counters} == {c: sb[c] for c in counters}, k
        feed()
        assert engine_groups(a) == engine_groups(b), k
        for w in range(0, ca.W, 7):
            x, y = a.lookup(w), b.lookup(w)
            assert (x.task, x.group_slot, x.group_index, x.group_size, x.next_worker, x.group_id) == \
                   (y.task, y.group_slot, y.group_index, y.group_size, y.next_worker, y.group_id), (k, w)
        before = image(a)
        feed()
        assert image(a) == before == image(b)
    a.close(), b.close()


def test_reads_are_deterministic():
    W = 2 * RO_CHUNK + 513

    def image(eng):
        out = []
        for q in _every_query() + [M.query(order=M.BY_ADDRESS, offset=1000, limit=77)]:
            total, counts, rows = eng.directory(q["status_mask"], q["membership"], q["order"], q["offset"],
                                                None if q["limit"] == M.TO_END else q["limit"])
            out.append(np.uint32(total).tobytes() + counts.tobytes() + rows.tobytes())
        return b"".join(out)

    _, eng, _ = _swarm_engine(W, seed=9)
    first = image(eng)
    assert image(eng) == first                                              # the same state read twice
    _, other, _ = _swarm_engine(W, seed=9)                                  # the same swarm on a fresh engine
    assert image(other) == first
    eng.close(), other.close()
