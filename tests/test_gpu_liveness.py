"""The liveness sweep on the GPU (pm_liveness_* of include/pm_engine.h, kernels in pm_liveness.inc) against the model of
tests/liveness_model.py, which tests/test_liveness_model.py holds to the reference (status_update/mod.rs:144-372): the
transition list, the census and every row's status and counter; an applying sweep against the same list handed to
pm_on_worker_status_many by hand, and against the oracle; what a sweep leaves alone; re-initialisation and every error."""
import numpy as np
import pytest

from oracle import oracle_ffi as orc
from protocol_amd import engine as E
from protocol_amd import host
from protocol_amd.swarm import make_swarm
from helpers import engine_groups, oracle_groups

import liveness_cases as LC
import liveness_model as M

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
NOW = LC.NOW_MS


def _cols(flags):
    """worker rows that differ in their flags only (the ledger reads nothing else)"""
    n = len(flags)
    one = np.ones(n, dtype=np.uint32)
    return dict(flags=np.asarray(flags, dtype=np.uint32), gpu_count=one, gpu_mem_mb=one, gpu_model_class=0 * one, cpu_cores=one,
                ram_mb=one, storage_gb=one, lat=np.zeros(n), lon=np.zeros(n))


def _engine(flags, m):
    eng = E.Engine()
    eng.upload_workers(_cols(flags))
    eng.liveness_enable(True, m)
    return eng, M.Ledger(flags, m)


def _rows_of(eng):
    r = eng.liveness_transitions()
    assert np.all(r["_pad"] == 0)
    return [(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(r["worker"], r["old_status"], r["new_status"], r["counter"])]


def _sweep_both(eng, led, now, beats, pool=None, tag=""):
    """one sweep on the engine and on the model; list, census and the whole ledger compared"""
    n, census = eng.liveness_sweep(now, beats, pool)
    rows, want_census = led.sweep(now, beats, pool)
    assert n == len(rows), tag
    assert census.tolist() == want_census, tag
    assert _rows_of(eng) == rows, tag
    s, c = eng.liveness_get()
    assert s.tolist() == led.status and c.tolist() == led.counter, tag
    return rows


def _flags(rng, W):
    return np.where(rng.random(W) < 0.5, E.W_HEALTHY, 0).astype(np.uint32) | np.uint32(1)   # (some other bit: only HEALTHY counts)


@pytest.mark.parametrize("m", LC.THRESHOLDS)
def test_every_named_case_in_one_sweep(m):
    """W = 8 x the number of cases: case k in the rows k, k + n, ... — 43 cases against words of 64 rows, so every case meets
    wave and word edges.  Under the threshold a case is named for, its hand-written outcome is asserted as well."""
    nc = len(LC.CASES)
    W = 8 * nc
    eng, led = _engine(np.zeros(W, dtype=np.uint32), m)
    which = np.arange(W) % nc
    status = np.array([LC.CASES[k]["status"] for k in which], dtype=np.uint8)
    counter = np.array([LC.CASES[k]["counter"] for k in which], dtype=np.uint32)
    beats = np.array([LC.beat_ms(LC.CASES[k]) for k in which], dtype=np.uint64)
    pool = M.pack_bits([LC.CASES[k]["in_pool"] for k in which])
    eng.liveness_set(np.arange(W), status, counter)
    led.set(np.arange(W), status, counter)
    rows = _sweep_both(eng, led, NOW, beats, pool)
    listed = {r[0] for r in rows}
    s, c = eng.liveness_get()
    for w in range(W):
        case = LC.CASES[which[w]]
        if case["m"] == m:
            assert (int(s[w]), int(c[w]), w in listed) == case["want"], case["name"]
    eng.close()


@pytest.mark.parametrize("with_pool", [False, True], ids=["pool-null", "pool-bits"])
@pytest.mark.parametrize("W", [1, 63, 64, 65, 255, 256, 257, 1025, 65537])
def test_list_order_and_census(W, with_pool):
    """seeded random states with about half the rows listed, then an all-listed and a none-listed sweep; 65,537 rows take the
    scan's second pass (65,536 rows a pass)"""
    rng = np.random.default_rng(1000 + W)
    eng, led = _engine(_flags(rng, W), 3)
    pool = M.pack_bits(rng.random(W) < 0.5) if with_pool else None
    status = rng.integers(0, M.N_STATUS, size=W).astype(np.uint8)
    counter = rng.choice([0, 1, 2, 3, 359, 360, 361, M.U32_MAX], size=W).astype(np.uint32)
    eng.liveness_set(np.arange(W), status, counter)
    led.set(np.arange(W), status, counter)
    beats = np.where(rng.random(W) < 0.5, NOW - rng.integers(0, 90_000, size=W), 0).astype(np.uint64)
    rows = _sweep_both(eng, led, NOW, beats, pool, "random")
    if W >= 255:
        assert 0.3 * W < len(rows) < 0.8 * W
    healthy = np.full(W, M.HEALTHY, dtype=np.uint8)
    eng.liveness_set(np.arange(W), healthy)
    led.set(np.arange(W), healthy)
    rows = _sweep_both(eng, led, NOW + 15_000, np.zeros(W, dtype=np.uint64), pool, "all listed")
    assert [r[0] for r in rows] == list(range(W))
    eng.liveness_set(np.arange(W), healthy)
    led.set(np.arange(W), healthy)
    rows = _sweep_both(eng, led, NOW + 30_000, np.full(W, NOW + 29_000, dtype=np.uint64), pool, "none listed")
    assert rows == []
    eng.close()


def test_three_hundred_sweeps_with_beats_sets_and_appends():
    """W = 257 growing to about 400 by appends; between sweeps seeded beats, pm_liveness_set calls and pm_append_workers;
    everything compared after every sweep"""
    rng = np.random.default_rng(77)
    W = 257
    flags = _flags(rng, W)
    eng, led = _engine(flags, 3)
    beats = np.zeros(W, dtype=np.uint64)
    in_pool = rng.random(W) < 0.7
    now = NOW
    for k in range(300):
        now += 15_000
        if k % 2 == 0:                                                  # a new row (some healthy, some not; some never beat)
            f = _flags(rng, 1)
            assert eng.append_workers(_cols(f)) == W
            led.append(f)
            beats = np.append(beats, np.uint64(0))
            in_pool = np.append(in_pool, rng.random() < 0.7)
            W += 1
        if k % 3 == 0:                                                  # statuses written by someone else: the ban route, the invite ...
            idx = rng.choice(W, size=5, replace=True)
            st = rng.integers(0, M.N_STATUS, size=5).astype(np.uint8)
            if k % 2:
                eng.liveness_set(idx, st)
                led.set(idx, st)
            else:
                cnt = rng.choice([0, 1, 2, 358, 359, 360], size=5).astype(np.uint32)
                eng.liveness_set(idx, st, cnt)
                led.set(idx, st, cnt)
        chatty = rng.random(W) < 0.8                                    # four in five beat this interval, the others' beats age
        beats = np.where(chatty, now - rng.integers(0, 15_000, size=W), beats).astype(np.uint64)
        if k % 50 == 49:
            in_pool = rng.random(W) < 0.7
        _sweep_both(eng, led, now, beats, M.pack_bits(in_pool) if k % 4 else None, f"sweep {k}")
    assert W == 407 and eng.W == W
    eng.close()


# ------------------------------------------------------------------------------------------------ apply

def _swarm():
    """402 rows, quads and solos: 95 groups of four and 3 solo groups on the first tick"""
    sw = make_swarm(7, 120, 402)
    sw.configs = [("quad", 4, 4, None), ("solo", 1, 1, None)]
    sw.topo[:] = -2
    sw.topo[:, 0] = 0
    sw.topo[:, 1] = 1
    sw.restricted[:] = True
    sw.n_topo[:] = 2
    return sw


def _loaded(sw, feed=True):
    eng = E.Engine()
    host.load_swarm(eng, sw)
    eng.enable_group_events(True)
    if feed:
        eng.enable_assignment_changes(True)
    eng.tick()
    eng.drain_group_events()
    if feed:
        eng.drain_assignment_changes()
    return eng


def _lookups(eng, W):
    out = []
    for w in range(W):
        a = eng.lookup(w)
        out.append((a.task, a.group_index, a.group_size, a.next_worker, a.group_id))
    return out


def _by_hand(eng, flags, rows):
    """what an applying sweep does with its list, through the public call"""
    w = np.array([r[0] for r in rows], dtype=np.uint32)
    f = np.array([(int(flags[r[0]]) | E.W_HEALTHY) if r[2] == M.HEALTHY else (int(flags[r[0]]) & ~E.W_HEALTHY) for r in rows], dtype=np.uint32)
    d = np.array([r[2] == M.DEAD for r in rows], dtype=np.uint32)
    eng.on_worker_status_many(w, f, d)
    return w, f


def test_applying_sweep_equals_the_list_by_hand_and_the_oracle():
    """Engine A sweeps with apply = 1; engine B sweeps with apply = 0 and hands the list to pm_on_worker_status_many itself.
    m = 1: a silent Healthy row is Unhealthy after one sweep and Dead after two.  A member of a quad and a solo die (their
    groups dissolve), then beat again, revive and are carved again.  After every sweep: groups, life-cycle events and every
    published row equal; after the tick behind it the change feed too, and groups and tasks equal the oracle that was given
    the same flips."""
    sw = _swarm()
    W = 402
    a, b = _loaded(sw), _loaded(sw)
    nodes, cfgs, tasks, enabled = orc.from_swarm(sw)
    st = orc.State(nodes, cfgs, enabled=enabled, tasks=tasks)
    st.try_form_new_groups()
    st.try_merge_solo_groups()
    assert [st.get_task_for_node(w) for w in range(W)] == [(-1 if t[0] == NONE else t[0]) for t in _lookups(a, W)]
    groups = engine_groups(a)
    assert groups == engine_groups(b) and sorted(groups) == sorted(oracle_groups(st))
    quad = next(g for g in groups if len(g[2]) == 4)
    solo = next(g for g in groups if len(g[2]) == 1)
    victims = [quad[2][1], solo[2][0]]
    flags = host.pack_workers(sw)["flags"].astype(np.uint32).copy()
    led = M.Ledger(flags, 1)
    for eng in (a, b):
        eng.liveness_enable(True, 1)
    now = NOW
    beats = np.full(W, now, dtype=np.uint64)
    silent = [True, True, False, False]               # the victims: Healthy -> Unhealthy -> Dead -> (beat) Healthy -> Healthy
    saw = []
    for k, quiet in enumerate(silent):
        now += 15_000
        beats[:] = now - 1000
        if quiet:
            beats[victims] = NOW - 200_000
        rows, census = led.sweep(now, beats)
        na, ca = a.liveness_sweep(now, beats, None, apply=True)
        nb, cb = b.liveness_sweep(now, beats, None, apply=False)
        assert na == nb == len(rows) and ca.tolist() == cb.tolist() == census
        assert _rows_of(a) == _rows_of(b) == rows
        saw.append({r[0]: (r[1], r[2]) for r in rows})
        _, f = _by_hand(b, flags, rows)
        for (w, _, new, _), fl in zip(rows, f):
            flags[w] = fl
            st.set_node_status(int(w), int(new))
        assert engine_groups(a) == engine_groups(b), k
        assert a.drain_group_events() == b.drain_group_events(), k
        assert _lookups(a, W) == _lookups(b, W), k
        if k == 1:                                                        # the deaths: both groups are gone, at once
            left = {g[0] for g in engine_groups(a)}
            assert quad[0] not in left and solo[0] not in left
            assert all(a.lookup(int(w)).group_size == 0 for w in quad[2] + solo[2])
        sa, sb = a.tick(), b.tick()
        st.try_form_new_groups()
        st.try_merge_solo_groups()
        want = [st.get_task_for_node(w) for w in range(W)]
        la = _lookups(a, W)
        assert la == _lookups(b, W), k
        assert [(-1 if t[0] == NONE else t[0]) for t in la] == want, k
        assert sorted(engine_groups(a)) == sorted(engine_groups(b)) == sorted(oracle_groups(st)), k
        ca_, cb_ = a.drain_assignment_changes(), b.drain_assignment_changes()
        assert ca_[0].tolist() == cb_[0].tolist() and ca_[1].tolist() == cb_[1].tolist() and ca_[2] == cb_[2], k
        assert a.drain_group_events() == b.drain_group_events(), k
        assert sa["n_formed"] == sb["n_formed"]
    # sweep 0 also turned every Discovered row of the swarm Healthy (all beat, all in pool): many flips in one list
    assert len(saw[0]) > 2 and all(saw[0][v] == (M.HEALTHY, M.UNHEALTHY) for v in victims)
    assert all(saw[1][v] == (M.UNHEALTHY, M.DEAD) for v in victims)
    assert all(saw[2][v] == (M.DEAD, M.HEALTHY) for v in victims) and saw[3] == {}
    assert all(a.lookup(int(v)).group_size > 0 for v in victims)          # revived and carved again
    a.close(), b.close()


def test_a_reporting_sweep_leaves_the_tick_alone():
    """an engine that enabled liveness and swept with apply = 0 (set, get and transitions beside it) ticks to the same groups,
    tasks and counters as a twin that never enabled it — with status changes pending on both"""
    sw = make_swarm(9, 200, 600)
    W = 600
    flags = host.pack_workers(sw)["flags"].astype(np.uint32)
    a, b = _loaded(sw, feed=False), _loaded(sw, feed=False)
    healthy = np.nonzero(sw.status == 2)[0][:30]
    for eng in (a, b):                                                    # pending deltas the sweep must not consume
        eng.on_worker_status_many(healthy, flags[healthy] & ~np.uint32(E.W_HEALTHY), np.ones(len(healthy), dtype=np.uint32))
    pushes = a.debug_delta_pushes()
    a.liveness_enable(True, 3)
    now_flags = flags.copy()
    now_flags[healthy] &= ~np.uint32(E.W_HEALTHY)
    led = M.Ledger(now_flags, 3)                                          # (the host's CURRENT flags, pending or not)
    beats = np.where(np.arange(W) % 2 == 0, NOW - 5, 0).astype(np.uint64)
    rows, want_census = led.sweep(NOW, beats)
    n, census = a.liveness_sweep(NOW, beats, None, apply=False)
    assert n == len(rows) and census.tolist() == want_census and _rows_of(a) == rows
    a.liveness_set([0, 1], [M.BANNED, M.DEAD], [4, 5])
    a.liveness_get()
    a.liveness_transitions()
    assert a.debug_delta_pushes() == pushes
    assert engine_groups(a) == engine_groups(b)
    sa, sb = a.tick(), b.tick()
    assert (sa["n_formed"], sa["carve_steps"]) == (sb["n_formed"], sb["carve_steps"])
    assert engine_groups(a) == engine_groups(b) and _lookups(a, W) == _lookups(b, W)
    assert a.drain_group_events() == b.drain_group_events()
    a.close(), b.close()


# ------------------------------------------------------------------------------------------------ life cycle and errors

def test_reinitialisation_and_keeping():
    rng = np.random.default_rng(3)
    W = 130
    flags = _flags(rng, W)
    eng, led = _engine(flags, 3)
    _sweep_both(eng, led, NOW, np.zeros(W, dtype=np.uint64))
    before = eng.liveness_get()
    assert len(eng.liveness_transitions()) > 0
    # keep_groups = 1: the same rows in front keep their ledger, the rows behind them start fresh
    more = np.concatenate([flags, _flags(rng, 70)])
    eng.upload_workers(_cols(more), keep_groups=True)
    led.append(more[W:])
    s, c = eng.liveness_get()
    assert s[:W].tolist() == before[0].tolist() and c[:W].tolist() == before[1].tolist()
    assert s.tolist() == led.status and c.tolist() == led.counter
    assert _rows_of(eng) == led.rows                                      # the list names rows that are still there
    _sweep_both(eng, led, NOW + 15_000, np.zeros(200, dtype=np.uint64))
    # keep_groups = 0: every row starts over, from the new flags, and the list is empty
    fresh = _flags(rng, 90)
    eng.upload_workers(_cols(fresh))
    led = M.Ledger(fresh, 3)
    assert len(eng.liveness_transitions()) == 0
    s, c = eng.liveness_get()
    assert s.tolist() == led.status and not c.any()
    _sweep_both(eng, led, NOW + 30_000, np.zeros(90, dtype=np.uint64))
    # enabling again re-initialises (with the flags the host holds now) and takes the new threshold
    eng.on_worker_status(0, int(fresh[0]) ^ E.W_HEALTHY, False)
    fresh[0] ^= E.W_HEALTHY
    eng.liveness_enable(True, 1)
    led = M.Ledger(fresh, 1)
    assert len(eng.liveness_transitions()) == 0
    _sweep_both(eng, led, NOW + 45_000, np.zeros(90, dtype=np.uint64))
    _sweep_both(eng, led, NOW + 60_000, np.zeros(90, dtype=np.uint64))
    eng.liveness_enable(False)
    with pytest.raises(E.EngineError) as ei:
        eng.liveness_get()
    assert ei.value.code == -4
    eng.close()


def _code(call):
    with pytest.raises(E.EngineError) as ei:
        call()
    return ei.value.code


def test_inside_a_stepwise_tick_every_liveness_call_is_refused():
    """dist_phase != 0 is reachable on one GPU (pm_dist_tick_begin with world = 1): sweep, set, get, transitions and enable
    are PM_ESTATE between begin and end, and afterwards the ledger and the previous list are what they were"""
    ESTATE = -4
    sw = make_swarm(5, 40, 200)
    W = sw.W
    eng = E.Engine()
    host.load_swarm(eng, sw)
    flags = host.pack_workers(sw)["flags"].astype(np.uint32)
    eng.liveness_enable(True, 3)
    led = M.Ledger(flags, 3)
    beats = np.where(np.arange(W) % 3 == 0, 0, NOW - 10).astype(np.uint64)
    _sweep_both(eng, led, NOW, beats)
    rows = _rows_of(eng)
    assert rows
    eng.dist_configure(0, 1)
    eng.dist_tick_begin()
    assert _code(lambda: eng.liveness_sweep(NOW + 1, beats)) == ESTATE
    assert _code(lambda: eng.liveness_sweep(NOW + 1, beats, None, apply=True)) == ESTATE
    assert _code(lambda: eng.liveness_set([0], [M.BANNED], [9])) == ESTATE
    assert _code(lambda: eng.liveness_get([0])) == ESTATE
    assert _code(eng.liveness_transitions) == ESTATE
    assert _code(lambda: eng.liveness_enable(True, 1)) == ESTATE
    assert _code(lambda: eng.liveness_enable(False)) == ESTATE
    eng.dist_carve_wait()
    eng.dist_match_begin()
    eng.dist_tick_end()
    s, c = eng.liveness_get()
    assert s.tolist() == led.status and c.tolist() == led.counter and _rows_of(eng) == rows
    _sweep_both(eng, led, NOW + 15_000, beats)                            # (still on, with the threshold it had)
    eng.close()


def test_errors_leave_the_ledger_and_the_list_as_they_were():
    EINVAL, ESTATE, ERANGE = -1, -4, -5
    rng = np.random.default_rng(4)
    W = 100
    flags = _flags(rng, W)
    eng = E.Engine()
    beats = np.zeros(W, dtype=np.uint64)
    # off
    assert _code(lambda: eng.liveness_sweep(NOW, None)) == ESTATE
    assert _code(lambda: eng.liveness_set([0], [0])) == ESTATE
    assert _code(lambda: eng.liveness_get([0])) == ESTATE
    assert _code(eng.liveness_transitions) == ESTATE
    # on, before workers are uploaded
    eng.liveness_enable(True, 3)
    assert _code(lambda: eng.liveness_sweep(NOW, None)) == ESTATE
    assert _code(lambda: eng.liveness_get([])) == ESTATE
    eng.upload_workers(_cols(flags))
    led = M.Ledger(flags, 3)
    _sweep_both(eng, led, NOW, beats)
    rows = _rows_of(eng)
    assert rows and _rows_of(eng) == rows                                 # reading twice: the same list

    def unchanged():
        s, c = eng.liveness_get()
        assert s.tolist() == led.status and c.tolist() == led.counter and _rows_of(eng) == rows

    assert _code(lambda: eng.liveness_set([3, W], [M.BANNED, M.BANNED])) == ERANGE
    unchanged()
    assert _code(lambda: eng.liveness_set([3, 4], [M.BANNED, M.N_STATUS])) == EINVAL
    unchanged()
    assert _code(lambda: eng.liveness_get([0, W])) == ERANGE
    assert _code(lambda: eng.liveness_sweep(NOW + 1, None)) == EINVAL       # (a NULL beat column with W > 0)
    unchanged()
    n = E.C.c_uint32(0)
    small = np.zeros(max(len(rows) - 1, 1), dtype=E.live_row_dt)
    assert E.lib().pm_liveness_transitions(eng._h, small.ctypes.data, len(rows) - 1, E.C.byref(n)) == ERANGE
    assert n.value == len(rows) and not small["worker"].any() and not small["new_status"].any()
    assert E.lib().pm_liveness_transitions(eng._h, None, 1 << 20, E.C.byref(n)) == ERANGE and n.value == len(rows)
    unchanged()
    # multi-GPU engines are out of scope, both ways round
    assert _code(lambda: eng.dist_configure(0, 2, np.zeros(W, dtype=np.uint8))) == ESTATE
    unchanged()
    eng.liveness_enable(False)
    eng.dist_configure(0, 2, np.zeros(W, dtype=np.uint8))
    assert _code(lambda: eng.liveness_enable(True, 3)) == ESTATE
    eng.close()
