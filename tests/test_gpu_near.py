"""pm_nearest_workers on the GPU against the model of tests/near_model.py (the reference's candidate filter, seed rule and
stable proximity sort over the oracle's calculate_distance), and against the carve itself.

Fixtures are "separated" wherever the test builds its own coordinates (near_model.separated_coordinates: from every origin
used, two distances are bit-equal in the oracle or more than 1e-9 apart relatively, and every pair has a <= 0.999): there
the index lists must be exact, position by position.  On swarms with other coordinates a position may differ from the
model's only between workers whose oracle distances agree within spread_model.TOL = 1e-12 (the spread tests' derivation:
hav_a's error reaches d multiplied by at most 16 for a <= 0.999), km must be within TOL, and nothing nearer may be left out.
Shapes are small: the kernel's risks are its edges (a wave's 64 rows, the four-wave stride of 256, buffers of max(2 k, k + 64)
keys, the cut to k), not its size."""
import json
import os
import sys

import numpy as np
import pytest

from oracle import oracle_ffi as orc
from protocol_amd import engine as E
from protocol_amd import host
from protocol_amd.churn import ChurnStream
from protocol_amd.swarm import make_swarm

import near_model as NM

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from make_golden_churn import CHURN_SEED, CHURN_TICKS_PINNED, CHURN_TICKS_PLANNED, events_digest, sha  # noqa: E402

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
SEED = E.NEAR_SEED
BASE = E.W_HEALTHY | E.W_HAS_P2P
LOC = BASE | E.W_HAS_LOC
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "churn_digests.json")))
KS = (1, 2, 63, 64, 65, 128, 255, 256)


def make_cols(flags, lat, lon):
    W = len(flags)
    z = np.zeros(W, dtype=np.uint32)
    return dict(flags=np.asarray(flags, dtype=np.uint32).copy(), gpu_count=z, gpu_mem_mb=z, gpu_model_class=z, cpu_cores=z,
                ram_mb=z, storage_gb=z, price=z, addr_rank=np.arange(W, dtype=np.uint32)[::-1].copy(),
                lat=np.ascontiguousarray(lat, dtype=np.float64), lon=np.ascontiguousarray(lon, dtype=np.float64))


def make_engine(cols, configs=(("a", 1, 300, None),), enabled=None, **kw):
    eng = E.Engine(group_id_seed=5, **kw)
    cfg_rows, alt_rows, _ = host.pack_configs(list(configs))
    eng.set_configs(cfg_rows, alt_rows)
    eng.upload_workers(cols)
    eng.upload_tasks(np.array([3, 1, 2], dtype=np.uint64), np.array([30, 20, 10], dtype=np.int64),
                     np.array([7, 8, 9], dtype=np.uint64))
    eng.set_enabled_mask((1 << len(configs)) - 1 if enabled is None else enabled)
    return eng


def check_call(eng, queries, pool, k, compat, flags, group_of, lat, lon, exact, tag=""):
    rows, workers, km = eng.nearest_workers(queries, pool, k)
    assert rows.shape == (len(queries),) and workers.shape == km.shape == (len(queries), k)
    for i, (o, c) in enumerate(queries):
        want = NM.nearest(o, c, pool, k, compat, flags, group_of, lat, lon)
        NM.check_query(rows[i], workers[i], km[i], want, exact, f"{tag} query {i} ({o}, {c}) pool {pool} k {k}")
    return rows, workers, km


def all_ok(W):
    return np.full(W, 1, dtype=np.uint64), np.full(W, -1, dtype=np.int64)


# ------------------------------------------------------------------ shapes

@pytest.mark.parametrize("W", [1, 2, 63, 64, 65, 255, 256, 257, 1025, 3000])
def test_shape_sweep(W):
    """every k at every W, from a located origin by index and from the seed; a tenth of the rows unlocated, a tenth not
    Healthy, so the candidate count sits below, at and above k"""
    rng = np.random.default_rng(100 + W)
    flags = np.full(W, LOC, dtype=np.uint32)
    flags[rng.random(W) < 0.1] = BASE
    flags[rng.random(W) < 0.1] &= ~np.uint32(E.W_HEALTHY)
    o = W // 2
    flags[o] = LOC
    first = int(np.flatnonzero(flags == LOC)[0])     # the seed
    lat, lon = NM.separated_coordinates(rng, W, origins=[o, first], twins=min(W // 8, 20), mirrors=min(W // 16, 4))
    cols = make_cols(flags, lat, lon)
    eng = make_engine(cols)
    compat, gof = all_ok(W)
    for k in KS:
        rows, _, _ = check_call(eng, [(o, 0), (SEED, 0)], E.NEAR_IDLE, k, compat, flags, gof, lat, lon, True, f"W {W}")
        assert int(rows[1]["origin"]) == first
    eng.close()


def test_zero_candidates():
    flags = np.array([LOC, E.W_HAS_P2P | E.W_HAS_LOC, E.W_HEALTHY, LOC], dtype=np.uint32)
    lat, lon = np.array([1.0, 2.0, 3.0, 4.0]), np.zeros(4)
    eng = make_engine(make_cols(flags, lat, lon), configs=(("a", 1, 4, None), ("b", 1, 4, "gpu:count=8")))
    compat = np.full(4, 1, dtype=np.uint64)      # nobody has specs: configuration 1 is met by no one
    gof = np.full(4, -1)
    rows, workers, km = check_call(eng, [(0, 1), (SEED, 1), (1, 1), (3, 0)], E.NEAR_ELIGIBLE, 5, compat, flags, gof, lat, lon, True)
    assert rows["n"].tolist() == [0, 0, 0, 1] and int(rows[1]["origin"]) == NONE and workers[3].tolist() == [0] + [NONE] * 4
    eng.close()


# ------------------------------------------------------------------ the selection under stress

def stress_engine(lat, lon, flags=None):
    W = len(lat)
    flags = np.full(W, LOC, dtype=np.uint32) if flags is None else flags
    return make_engine(make_cols(flags, lat, lon)), flags


@pytest.fixture(scope="module")
def stress():
    """3,000 separated coordinates and their oracle distance from row 0"""
    rng = np.random.default_rng(4242)
    W = 3000
    lat, lon = NM.separated_coordinates(rng, W, origins=[0], twins=30, mirrors=6)
    d = orc.distance_column(float(lat[0]), float(lon[0]), lat, lon)
    return W, lat, lon, d


@pytest.mark.parametrize("layout", ["descending", "ascending"])
def test_stress_monotone_layouts(stress, layout):
    """descending: every candidate beats the threshold of the rows before it, so every buffer fills and is cut again and
    again; ascending: nothing after the first k does"""
    W, lat, lon, d = stress
    order = np.argsort(d[1:], kind="stable") + 1
    order = order[::-1] if layout == "descending" else order
    perm = np.concatenate([[0], order])
    la, lo = np.ascontiguousarray(lat[perm]), np.ascontiguousarray(lon[perm])
    eng, flags = stress_engine(la, lo)
    compat, gof = all_ok(W)
    for k in KS:
        check_call(eng, [(0, 0)], E.NEAR_IDLE, k, compat, flags, gof, la, lo, True, layout)
    eng.close()


def test_stress_identical_coordinates_give_index_order(stress):
    W = stress[0]
    lat, lon = np.full(W, 35.6762), np.full(W, 139.6503)
    flags = np.full(W, LOC, dtype=np.uint32)
    flags[5::7] = BASE                                 # unlocated rows: behind all the located ones, in index order too
    eng, _ = stress_engine(lat, lon, flags)
    compat, gof = all_ok(W)
    for k in KS:
        for o in (1500, 5):                            # a located and an unlocated origin
            _, workers, km = check_call(eng, [(o, 0)], E.NEAR_IDLE, k, compat, flags, gof, lat, lon, True, "identical")
            assert np.all(np.diff(workers[0].astype(np.int64)) > 0) or k > 2500
            assert np.all(km[0] == (0.0 if o == 1500 else NM.F64_MAX))
    rows, workers, km = check_call(eng, [(1500, 0)], E.NEAR_ELIGIBLE, 256, compat, flags, gof, lat, lon, True)
    eng.close()


@pytest.mark.parametrize("k", [1, 64, 65, 256])
def test_stress_exactly_k_and_2k_candidates(stress, k):
    W, lat, lon, d = stress
    rng = np.random.default_rng(k)
    compat, gof = all_ok(W)
    for n_cand in (k, 2 * k, 2 * k + 1, k + 64, k + 65):
        flags = np.full(W, LOC & ~E.W_HEALTHY, dtype=np.uint32)
        flags[0] = LOC
        flags[rng.choice(np.arange(1, W), n_cand, replace=False)] = LOC
        eng, _ = stress_engine(lat, lon, flags)
        rows, _, _ = check_call(eng, [(0, 0), (SEED, 0)], E.NEAR_IDLE, k, compat, flags, gof, lat, lon, True, f"{n_cand} candidates")
        assert int(rows[0]["candidates"]) == n_cand
        eng.close()


def test_stress_tie_clusters_straddle_every_k(stress):
    """40 sites, 75 rows each in round-robin: every k of the sweep ends inside a cluster of exact ties, whose members are
    spread over all four waves"""
    W, lat, lon, d = stress
    site = np.arange(W) % 40
    site[0] = 0
    la, lo = np.ascontiguousarray(lat[1 + site]), np.ascontiguousarray(lon[1 + site])
    la[0], lo[0] = lat[0], lon[0]
    assert NM.is_separated([0], la, lo)
    eng, flags = stress_engine(la, lo)
    compat, gof = all_ok(W)
    for k in KS:
        check_call(eng, [(0, 0)], E.NEAR_IDLE, k, compat, flags, gof, la, lo, True, "clusters")
    eng.close()


def test_non_finite_coordinates_terminate_with_distinct_candidates():
    W = 600
    rng = np.random.default_rng(3)
    lat, lon = rng.uniform(-50, 60, W), rng.uniform(-100, 50, W)
    lat[::5], lon[1::7] = np.nan, np.inf
    eng, flags = stress_engine(lat, lon)
    rows, workers, _ = eng.nearest_workers([(1, 0), (0, 0)], E.NEAR_IDLE, 256)
    for i in range(2):
        assert int(rows[i]["n"]) == 256 and int(rows[i]["candidates"]) == W - 1 and len(set(workers[i].tolist())) == 256
        assert workers[i].max() < W and (1, 0)[i] not in workers[i]
    eng.close()


# ------------------------------------------------------------------ origins

def test_origins():
    rng = np.random.default_rng(77)
    W = 300
    flags = np.full(W, LOC, dtype=np.uint32)
    flags[[0, 3, 40, 41]] = BASE                         # unlocated candidates; worker 0 is one: the seed is a later row
    flags[7] = LOC & ~E.W_HEALTHY                        # an unhealthy origin
    flags[9] = E.W_HEALTHY | E.W_HAS_LOC                 # ... and one without a p2p id
    lat, lon = NM.separated_coordinates(rng, W, origins=[1, 7, 9, 20, 21, 100], twins=10)
    configs = (("a", 1, 300, None), ("b", 1, 300, "gpu:count=1"))
    eng = make_engine(make_cols(flags, lat, lon), configs=configs)
    groups = [(11, 0, [20, 30, 31]), (12, 0, [50])]
    g = np.zeros(len(groups), dtype=E.group_dt)
    mem = []
    for i, (gid, cfg, m) in enumerate(groups):
        g[i]["id"], g[i]["config"], g[i]["n_members"], g[i]["member_begin"], g[i]["task"] = gid, cfg, len(m), len(mem), NONE
        mem += m
    eng.adopt_groups(g, np.array(mem, dtype=np.uint32), 999)
    gof = np.full(W, -1)
    gof[[20, 30, 31]], gof[50] = 0, 1
    compat = np.full(W, 1, dtype=np.uint64)              # (no worker has specs: only configuration 0 is met; an origin
    for pool in (E.NEAR_IDLE, E.NEAR_ELIGIBLE):          #  that meets nothing measures as well as any other)
        for k in (4, 64, 256):
            q = [(1, 0), (0, 0), (3, 0), (20, 0), (7, 0), (9, 0), (21, 1), (100, 1), (SEED, 0), (SEED, 1)]
            rows, workers, km = check_call(eng, q, pool, k, compat, flags, gof, lat, lon, True, "origins")
            assert rows["origin"].tolist() == [1, 0, 3, 20, 7, 9, 21, 100, 1, NONE]
            assert np.all(km[1] == NM.F64_MAX) and workers[1][:3].tolist() == [1, 2, 3]   # unlocated origin: index order
            assert rows["candidates"][6:8].tolist() == [0, 0]
    eng.close()
    # no located candidate: the seed is the lowest-index candidate; no candidate at all: PM_NONE
    flags2 = np.full(W, BASE, dtype=np.uint32)
    flags2[0] = E.W_HAS_P2P
    eng = make_engine(make_cols(flags2, lat, lon))
    rows, workers, km = check_call(eng, [(SEED, 0)], E.NEAR_IDLE, 8, compat, flags2, np.full(W, -1), lat, lon, True)
    assert int(rows[0]["origin"]) == 1 and workers[0].tolist() == list(range(2, 10)) and int(rows[0]["located"]) == 0
    eng.close()
    flags3 = np.full(W, LOC & ~E.W_HEALTHY, dtype=np.uint32)
    eng = make_engine(make_cols(flags3, lat, lon))
    rows, workers, km = check_call(eng, [(SEED, 0), (5, 0)], E.NEAR_ELIGIBLE, 8, compat, flags3, np.full(W, -1), lat, lon, True)
    assert rows["origin"].tolist() == [NONE, 5] and rows["n"].tolist() == [0, 0]
    eng.close()


# ------------------------------------------------------------------ pools, configurations, batches

@pytest.fixture(scope="module")
def swarm():
    """a generated swarm (requirements, GPU alternatives, a configuration without requirements) with coordinates inside
    the tolerance's range, after one tick: standing groups"""
    sw = make_swarm(1, 300, 1500)
    rng = np.random.default_rng(5)
    sw.lat = np.ascontiguousarray(rng.uniform(-50.0, 60.0, sw.W))
    sw.lon = np.ascontiguousarray(rng.uniform(-100.0, 50.0, sw.W))
    sw.lat[100:140], sw.lon[100:140] = sw.lat[100], sw.lon[100]      # a few exact ties
    nodes, cfgs, tasks, enabled = orc.from_swarm(sw)
    compat = orc.compat_masks(nodes, cfgs)
    return sw, compat, host.worker_flags(sw)


def swarm_engine(sw, enabled=None):
    eng = E.Engine(group_id_seed=3)
    host.load_swarm(eng, sw, enabled=enabled)
    return eng


def test_pools_configurations_and_batches(swarm):
    sw, compat, flags = swarm
    C = len(sw.configs)
    reqs = [r for (_n, _a, _b, r) in sw.configs]
    assert any(r is None for r in reqs) and any(r and r.count("gpu:count") >= 2 for r in reqs)   # (GPU alternatives)
    disabled = 1                                         # configuration 1 and all from 6 on are switched off (so that a
    eng = swarm_engine(sw, enabled=0x3D)                 # third of the swarm is grouped, the rest idle): still answered
    eng.tick()
    gof = eng.get_groups()[0].astype(np.int64)
    assert (gof >= 0).sum() > 100 and (gof < 0).sum() > 100
    assert np.array_equal(eng.explain_workers()[0] == 0, ((compat[:, None] >> np.arange(C, dtype=np.uint64)) & np.uint64(1)) != 0)
    rng = np.random.default_rng(9)
    grouped, free = np.flatnonzero(gof >= 0), np.flatnonzero(gof < 0)
    for pool in (E.NEAR_IDLE, E.NEAR_ELIGIBLE):
        q1 = [(int(grouped[0]), disabled)]
        q2 = [(SEED, 0), (int(free[0]), C - 1)]
        q300 = [(SEED if i % 10 == 0 else int(rng.integers(0, sw.W)), i % C) for i in range(300)]
        for q, k in ((q1, 16), (q2, 256), (q300, 7)):
            rows, _, _ = check_call(eng, q, pool, k, compat, flags, gof, sw.lat, sw.lon, False, "swarm")
        assert len(set(rows["candidates"].tolist())) > 3
    eng.close()


# ------------------------------------------------------------------ state

def test_pending_changes_are_seen_and_the_next_tick_is_untouched(swarm):
    sw, compat, flags = swarm
    flags = flags.copy()
    a, b = swarm_engine(sw, enabled=0x3D), swarm_engine(sw, enabled=0x3D)   # b never makes the call
    for e in (a, b):
        e.tick()
    gof, groups, members = a.get_groups()
    b.get_groups()
    gof = gof.astype(np.int64)
    # a status change and a dissolution that have not gone up yet
    slot = int(np.argmax(groups["n_members"]))
    mem = members[int(groups[slot]["member_begin"]):int(groups[slot]["member_begin"]) + int(groups[slot]["n_members"])]
    victim = int(np.flatnonzero(gof < 0)[3])
    flags[victim] &= ~np.uint32(E.W_HEALTHY)
    for e in (a, b):
        e.on_worker_status(victim, int(flags[victim]), False)
        e.dissolve_group(slot)
    gof[mem] = -1
    c = int(groups[slot]["config"])
    q = [(int(mem[0]), c), (SEED, c), (victim, 0), (int(mem[-1]), 0)]
    for pool in (E.NEAR_IDLE, E.NEAR_ELIGIBLE):
        rows, workers, _ = check_call(a, q, pool, 64, compat, flags, gof, sw.lat, sw.lon, False, "pending")
        assert victim not in workers
    # the freed members are candidates of their configuration again
    w_all = a.nearest_workers([(int(mem[0]), c)], E.NEAR_IDLE, 256)[1][0].tolist()
    n_idle = a.nearest_workers([(int(mem[0]), c)], E.NEAR_IDLE, 1)[0][0]["candidates"]
    assert n_idle > 256 or all(int(m) in w_all for m in mem[1:])
    sa, sb = a.tick(), b.tick()
    for key in ("n_groups", "n_formed", "n_merged", "n_dissolved"):
        assert sa.get(key) == sb.get(key), key
    ga, gb = a.get_groups(), b.get_groups()
    assert all(np.array_equal(x, y) for x, y in zip(ga, gb))
    ta = [(x.task, x.group_slot, x.group_index, x.group_size, x.next_worker, x.group_id) for x in map(a.lookup, range(sw.W))]
    tb = [(x.task, x.group_slot, x.group_index, x.group_size, x.next_worker, x.group_id) for x in map(b.lookup, range(sw.W))]
    assert ta == tb
    a.close()
    b.close()


def test_calls_between_the_ticks_of_the_churn_stream():
    """the oracle's digests through the pinned churn stream with the call made between every two engine calls"""
    gold = GOLD["churn"]
    eng = E.Engine(group_id_seed=1)
    cs = ChurnStream(CHURN_SEED, CHURN_TICKS_PLANNED)
    sw = cs.sw_all
    packed = host.pack_workers(sw)
    rows_of = lambda idx: {k: np.ascontiguousarray(v[idx]) for k, v in packed.items()}
    cfg_rows, alt_rows, req_models = host.pack_configs(sw.configs)
    eng.set_configs(cfg_rows, alt_rows)
    eng.set_model_table(host.build_model_table(req_models, sw.model_names), len(req_models), len(sw.model_names))
    eng.upload_workers(rows_of(np.arange(cs.W0)))
    eng.upload_tasks(cs.masks, cs.created, cs.uid)
    eng.set_enabled_mask(sw.enabled_mask())
    eng.enable_group_events()
    flags = packed["flags"].astype(np.int64).copy()
    C = len(sw.configs)

    def call():
        q = [(SEED, c) for c in range(C)] + [(0, 0), (eng.W - 1, C - 1)]
        rows, workers, km = eng.nearest_workers(q, E.NEAR_IDLE, 16)
        rep = eng.config_report()
        for c in range(C):                                # the seed's list and the seed are the idle workers that meet c
            n = int(rep[c]["idle_meets"])
            assert int(rows[c]["candidates"]) == max(n - 1, 0) and (int(rows[c]["origin"]) == NONE) == (n == 0)
            assert int(rows[c]["n"]) == min(16, max(n - 1, 0))
        live = workers[workers != NONE]
        assert live.size == 0 or live.max() < eng.W

    def check(W, g, stats, tag):
        assert stats["n_formed"] == g["n_formed"] and stats["n_groups"] == g["n_groups"], (tag, stats)
        col = np.array([eng.lookup(w).task for w in range(W)], dtype=np.uint32)
        assert sha(col) == g["task_sha256"], f"{tag}: per-worker tasks differ from the oracle"
        ev = eng.drain_group_events()
        assert len(ev) == g["n_events"] and events_digest(ev) == g["events_sha256"], f"{tag}: life-cycle feed"

    call()
    check(cs.W0, gold["cold"], eng.tick(), "cold")
    call()
    for k in range(CHURN_TICKS_PINNED):
        leave, idx_new, new_tasks = cs.step()
        flags[leave] &= ~E.W_HEALTHY
        eng.on_worker_status_many(leave, flags[leave], np.ones(len(leave), dtype=np.uint32))
        call()
        eng.append_workers(rows_of(idx_new))
        call()
        eng.tasks_insert_front(*new_tasks[:3])
        check(cs.W, gold["ticks"][k], eng.tick(), f"tick {k}")
        call()
    eng.close()


# ------------------------------------------------------------------ against the carve itself

@pytest.mark.parametrize("m", [2, 5, 64, 65])
def test_the_list_is_the_group_the_carve_forms(m):
    """one configuration with min = max = m: {seed} + the k = m - 1 nearest of the IDLE pool are the members of the next
    group pm_form_groups makes — for the first group on a fresh engine, and for the second and third with the earlier
    ones installed through pm_adopt_groups.  Separated coordinates from every row: no tolerance."""
    rng = np.random.default_rng(m)
    W = 3 * m + 17
    flags = np.full(W, LOC, dtype=np.uint32)
    flags[0] = BASE                                       # an unlocated candidate in front: never the seed
    flags[rng.choice(np.arange(1, W), 6, replace=False)] = BASE
    flags[rng.choice(np.arange(1, W), 4, replace=False)] &= ~np.uint32(E.W_HEALTHY)
    lat, lon = NM.separated_coordinates(rng, W, twins=6)
    cols = make_cols(flags, lat, lon)
    configs = (("only", m, m, None),)
    eng = make_engine(cols, configs=configs)
    rows, workers, _ = eng.nearest_workers([(SEED, 0)], E.NEAR_IDLE, m - 1)
    formed = eng.form_groups()
    assert formed >= 3
    _, groups, members = eng.get_groups()
    id_state = eng.group_id_state()
    eng.close()
    mem = [sorted(members[int(g["member_begin"]):int(g["member_begin"]) + int(g["n_members"])].tolist()) for g in groups]
    assert all(len(x) == m for x in mem[:3])
    assert int(rows[0]["n"]) == m - 1 and sorted([int(rows[0]["origin"])] + workers[0].tolist()) == mem[0]
    compat = np.full(W, 1, dtype=np.uint64)
    for j in (1, 2):
        eng = make_engine(cols, configs=configs)
        eng.adopt_groups(groups[:j], members[:int(groups[j]["member_begin"])], id_state)
        rows, workers, km = eng.nearest_workers([(SEED, 0)], E.NEAR_IDLE, m - 1)
        assert sorted([int(rows[0]["origin"])] + workers[0].tolist()) == mem[j], (m, j)
        gof = np.full(W, -1)
        for i in range(j):
            gof[mem[i]] = i
        NM.check_query(rows[0], workers[0], km[0], NM.nearest(SEED, 0, E.NEAR_IDLE, m - 1, compat, flags, gof, lat, lon), True)
        eng.close()


# ------------------------------------------------------------------ refusals

def test_refusals():
    L = E.lib()
    W = 10
    flags = np.full(W, LOC, dtype=np.uint32)
    cols = make_cols(flags, np.arange(W, dtype=float), np.zeros(W))
    k = 4
    q = np.zeros(2, dtype=E.near_query_dt)
    rows = np.full(2 * 16, 0xAB, dtype=np.uint8).view(E.near_row_dt)
    workers = np.full(2 * k, 0xABABABAB, dtype=np.uint32)
    km = np.full(2 * k, -1.0)
    keep = (rows.tobytes(), workers.tobytes(), km.tobytes())

    def call(eng, qq=q, n_q=2, pool=0, kk=k, r=rows, w=workers, d=km):
        rc = L.pm_nearest_workers(eng._h, qq.ctypes.data if qq is not None else None, n_q, pool, kk,
                                  r.ctypes.data if r is not None else None, w.ctypes.data if w is not None else None,
                                  d.ctypes.data if d is not None else None)
        assert (rows.tobytes(), workers.tobytes(), km.tobytes()) == keep or rc == 0, "an error wrote to the output"
        return rc

    eng = E.Engine()
    assert call(eng) == E.PM_ESTATE                                   # nothing uploaded
    cfg_rows, alt_rows, _ = host.pack_configs([("a", 1, 4, None), ("b", 1, 4, None)])
    eng.set_configs(cfg_rows, alt_rows)
    assert call(eng) == E.PM_ESTATE                                   # no workers yet
    eng.close()
    eng = make_engine(cols, configs=(("a", 1, 4, None), ("b", 1, 4, None)))
    assert call(eng, kk=0) == E.PM_EINVAL
    assert call(eng, kk=E.NEAR_MAX_K + 1) == E.PM_EINVAL
    assert call(eng, n_q=E.NEAR_MAX_QUERIES + 1) == E.PM_EINVAL
    assert call(eng, pool=2) == E.PM_EINVAL
    assert call(eng, r=None) == E.PM_EINVAL
    assert call(eng, w=None) == E.PM_EINVAL
    assert call(eng, qq=None) == E.PM_EINVAL
    for bad in ((W, 0), (NONE, 0), (0, 2), (SEED, 2)):
        q[1] = bad                                                    # (the first query is fine: still nothing is written)
        assert call(eng) == E.PM_ERANGE, bad
    q[1] = (3, 1)
    eng.dist_configure(0, 1)
    eng.dist_tick_begin()
    assert call(eng) == E.PM_ESTATE
    eng.dist_carve_wait()
    eng.dist_match_begin()
    eng.dist_tick_end()
    assert call(eng, n_q=0, qq=None, r=None, w=None, d=None) == 0     # no query: nothing to do
    assert call(eng, pool=1, d=None) == 0 and km.tobytes() == keep[2]  # km may be NULL
    assert rows["n"].tolist() == [4, 4] and rows["origin"].tolist() == [0, 3] and rows["candidates"].tolist() == [9, 9]
    assert call(eng, pool=1) == 0 and np.all(km >= 0.0)
    eng.close()
