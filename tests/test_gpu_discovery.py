"""The discovery sync on the GPU (pm_discovery_sync of include/pm_engine.h, kernels in pm_discovery.inc) against the literal
sequential pass of tests/discovery_model.py, which tests/test_discovery_model.py holds to the reference
(discovery/monitor.rs:218-435).  Integers only, exact: every result row, every ledger byte; lane, wave and workgroup edges;
segments on both sides of the cooperative walk's threshold (DISC_WALK_ALONE = 64 events); order; the threshold; retired rows;
the 400 seeded cases; an applying call against the same updates by hand and the oracle; the ledger; every error."""
import numpy as np
import pytest

from oracle import oracle_ffi as orc
from protocol_amd import engine as E
from protocol_amd import host
from protocol_amd.swarm import make_swarm
from helpers import engine_groups, oracle_groups

import discovery_cases as DC
import discovery_model as M
import liveness_model as LM

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
NOW = DC.NOW_MS
EINVAL, ESTATE, ERANGE = -1, -4, -5
WALK_ALONE = 64
FILLER = M.node("filler", M.DISCOVERED, None)                             # (an engine has no empty table)


def _cols(flags):
    """worker rows that differ in their flags only (the ledger reads nothing else)"""
    n = len(flags)
    one = np.ones(n, dtype=np.uint32)
    return dict(flags=np.asarray(flags, dtype=np.uint32), gpu_count=one, gpu_mem_mb=one, gpu_model_class=0 * one, cpu_cores=one,
                ram_mb=one, storage_gb=one, lat=np.zeros(n), lon=np.zeros(n))


def _flags_of(status):
    return np.where(np.asarray(status) == M.HEALTHY, E.W_HEALTHY, 0).astype(np.uint32) | np.uint32(1)


def _load(eng, status):
    """a fresh table whose ledger holds `status` (counters 5, 6, 7, ... so that a touched counter shows)"""
    W = len(status)
    eng.upload_workers(_cols(_flags_of(status)))
    eng.liveness_set(np.arange(W), np.asarray(status, dtype=np.uint8), 5 + np.arange(W, dtype=np.uint32))


def _rows(abi):
    return np.array(abi["rows"], dtype=E.disc_row_dt)


def _as_dicts(out):
    res = []
    for o in out:
        n = int(o["n_updates"])
        assert n <= 3 and int(o["_pad"]) == 0
        assert all(int(o["upd_old"][k]) == M.N_STATUS and int(o["upd_new"][k]) == M.N_STATUS for k in range(n, 3))
        res.append(dict(cnt=int(o["healthy_same_endpoint"]), old_status=int(o["old_status"]), final_status=int(o["final_status"]),
                        updates=[(int(o["upd_old"][k]), int(o["upd_new"][k])) for k in range(n)], ops=int(o["ops"])))
    return res


def _sync_both(eng, store, discovery, now, max_same, tag=""):
    """one pass on the engine and in the model; every result row and the whole ledger compared -> (results, abi)"""
    if not store:
        store = M.make_store([FILLER])
    want, want_status, _, _, abi, _ = M.run_sequential(store, discovery, now, max_same)
    _load(eng, abi["status"])
    out, total = eng.discovery_sync(now, abi["row_endpoint"], abi["n_endpoints"], max_same, _rows(abi))
    got = _as_dicts(out)
    assert got == want, tag
    assert total == sum(len(r["updates"]) for r in want), tag
    s, c = eng.liveness_get()
    assert s.tolist() == want_status, tag
    assert c.tolist() == list(range(5, 5 + len(s))), tag                  # the counter column is not touched
    return got, abi


@pytest.fixture(scope="module")
def eng():
    e = E.Engine()
    e.upload_workers(_cols([1]))
    e.liveness_enable(True, 3)
    yield e
    e.close()


@pytest.mark.parametrize("case", DC.CASES, ids=lambda c: c["name"])
def test_named_case(eng, case):
    got, _ = _sync_both(eng, M.make_store(case["store"]), case["discovery"], case["now"], case["max"], case["name"])
    for res, (final, updates, _) in zip(got, case["want"]):
        if final in ("skip", "admit"):
            assert res["ops"] == (M.DO_SKIP if final == "skip" else M.DO_ADMIT)
        else:
            assert (res["final_status"], res["updates"]) == (final, updates)


@pytest.mark.parametrize("D", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("W", [1, 63, 64, 65, 255, 256, 257])
def test_lane_wave_and_workgroup_edges(eng, W, D):
    for n_ep in (1, 4, 16):
        store, discovery, now, max_same = M.seeded_case(7000 + 300 * n_ep + W + D, W=W, D=D, n_ep=n_ep)
        _sync_both(eng, store, discovery, now, max_same, "W %d D %d E %d" % (W, D, n_ep))


def test_all_endpoints_distinct(eng):
    W = 300
    nodes = [M.node("a%03d" % w, M.HEALTHY if w % 2 else M.UNHEALTHY, "10.1.%d.%d" % (w // 200, w % 200), stamp=NOW - 10**7) for w in range(W)]
    discovery = [M.sighting(n["address"], n["ip_address"], active=bool(k % 3)) for k, n in enumerate(nodes)]
    discovery += [M.sighting("n%03d" % k, "10.1.%d.%d" % (k // 200, k % 200)) for k in range(0, W, 7)]
    got, abi = _sync_both(eng, M.make_store(nodes), discovery[::-1], NOW, 1)
    _, _, _, seg = M.parallel_pass(abi["status"], abi["row_endpoint"], abi["rows"], NOW, 1)
    assert set(seg.values()) <= {1, 2} and any(r["ops"] == M.DO_SKIP for r in got) and any(r["ops"] == M.DO_ADMIT for r in got)


@pytest.mark.parametrize("keep,demoted", [(0, 0), (0, 1), (31, 1), (32, 0), (32, 1), (100, 1), (300, 5)],
                         ids=lambda v: str(v))
def test_one_endpoint_for_everybody(eng, keep, demoted):
    """E = 1: `keep` listed Healthy rows that stay (two events each) and `demoted` ones that do not (one event): segments of
    0, 1, 63, 64, 65, 201 and 605 events around the cooperative walk's threshold of 64; new rows and unhealthy table rows ask at
    every third position"""
    nodes = [M.node("k%03d" % k, M.HEALTHY, stamp=NOW - 10**7) for k in range(keep)]
    nodes += [M.node("d%03d" % k, M.HEALTHY, stamp=NOW - 10**7) for k in range(demoted)]
    nodes += [M.node("u%03d" % k, M.UNHEALTHY) for k in range(5)] + [M.node("h-unlisted", M.HEALTHY)]
    discovery = [M.sighting("k%03d" % k) for k in range(keep)] + [M.sighting("d%03d" % k, active=False) for k in range(demoted)]
    rng = np.random.default_rng(keep + demoted)
    rng.shuffle(discovery)
    asks = [M.sighting("u%03d" % k) for k in range(5)] + [M.sighting("n%03d" % k) for k in range(max(3, (keep + demoted) // 3))]
    for k, a in enumerate(asks):
        discovery.insert(min(3 * k, len(discovery)), a)
    for max_same in (1, keep + demoted):
        got, abi = _sync_both(eng, M.make_store(nodes), discovery, NOW, max_same)
        _, _, _, seg = M.parallel_pass(abi["status"], abi["row_endpoint"], abi["rows"], NOW, max_same)
        assert sum(seg.values()) == 2 * keep + demoted and len(seg) <= 1
    assert (2 * keep + demoted > WALK_ALONE) == ((keep, demoted) in [(32, 1), (100, 1), (300, 5)])


def test_order_the_reversed_list_gives_the_reversed_lists_answer(eng):
    case = next(c for c in DC.CASES if c["name"].startswith("an ip move"))
    fwd, _ = _sync_both(eng, M.make_store(case["store"]), case["discovery"], NOW, 1)
    rev, _ = _sync_both(eng, M.make_store(case["store"]), case["discovery"][::-1], NOW, 1)
    assert [r["ops"] for r in rev[::-1]] != [r["ops"] for r in fwd]
    assert [r["cnt"] for r in rev[::-1]] != [r["cnt"] for r in fwd]


@pytest.mark.parametrize("max_same", [0, 1, 2, 3])
def test_threshold_counts_on_below_and_above(eng, max_same):
    """endpoint k holds k Healthy nodes, k = 0..4: a new node there is admitted iff k < max"""
    nodes = [M.node("h%d-%d" % (k, i), M.HEALTHY, "10.2.0.%d" % k) for k in range(5) for i in range(k)]
    discovery = [M.sighting("n%d" % k, "10.2.0.%d" % k) for k in range(5)]
    got, _ = _sync_both(eng, M.make_store(nodes), discovery, NOW, max_same)
    assert [r["cnt"] for r in got] == [0, 1, 2, 3, 4]
    assert [r["ops"] for r in got] == [M.DO_ADMIT if k < max_same else M.DO_SKIP for k in range(5)]


def test_retired_rows_listed_and_unlisted(eng):
    """PM_EP_NONE: an unlisted Healthy one is in no count, a listed one counts nowhere before its step and on its new endpoint
    behind it; a listed one that keeps no endpoint (Dead, specs put-back) stays out"""
    nodes = [M.node("r-unlisted", M.HEALTHY, None), M.node("r-gains", M.HEALTHY, None, stamp=NOW - 10**7),
             M.node("r-dead", M.DEAD, None, stamp=NOW - 1000, specs="specs-a")]
    discovery = [M.sighting("n0"), M.sighting("r-gains"), M.sighting("n1"),
                 M.sighting("r-dead", "10.0.0.9", specs="specs-b", last_updated=NOW - 10), M.sighting("n2")]
    got, abi = _sync_both(eng, M.make_store(nodes), discovery, NOW, 1)
    assert abi["row_endpoint"] == [M.EP_NONE] * 3
    assert [r["cnt"] for r in got] == [0, 0, 1, 0, 1] and [r["ops"] & 3 for r in got] == [M.DO_ADMIT, 0, M.DO_SKIP, 0, M.DO_SKIP]
    assert got[1]["ops"] == M.DO_IP_REWRITE and got[1]["final_status"] == M.HEALTHY
    assert got[3]["ops"] == M.DO_IP_REWRITE | M.DO_SPECS_REWRITE | M.DO_STAMP_NOW and got[3]["final_status"] == M.DISCOVERED


@pytest.mark.parametrize("chunk", range(8))
def test_seeded_cases(eng, chunk):
    for seed in range(chunk * M.N_SEEDED // 8, (chunk + 1) * M.N_SEEDED // 8):
        store, discovery, now, max_same = M.seeded_case(seed)
        _sync_both(eng, store, discovery, now, max_same, "seed %d" % seed)


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


def _loaded(sw):
    eng = E.Engine()
    host.load_swarm(eng, sw)
    eng.enable_group_events(True)
    eng.enable_assignment_changes(True)
    eng.tick()
    eng.drain_group_events()
    eng.drain_assignment_changes()
    eng.liveness_enable(True, 3)
    return eng


def _lookups(eng, W):
    out = []
    for w in range(W):
        a = eng.lookup(w)
        out.append((a.task, a.group_index, a.group_size, a.next_worker, a.group_id))
    return out


def test_apply_equals_the_updates_by_hand_and_the_oracle():
    """Engine A syncs with apply = 1; engine B with apply = 0 and sends the same updates through pm_on_worker_status_many itself.
    A LowBalance and a Dead update each dissolve a whole quad; an Ejected one dissolves nothing; a not whitelisted Healthy solo
    whose ip changed is Ejected and put back: it ends Healthy, keeps its flag and is used at the next tick (the oracle)."""
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
    quads = [g for g in groups if len(g[2]) == 4]
    solo = next(g for g in groups if len(g[2]) == 1)
    low, dead, ejected, back = quads[0][2][1], quads[1][2][2], quads[2][2][0], solo[2][0]
    flags = host.pack_workers(sw)["flags"].astype(np.uint32).copy()
    status = a.liveness_get()[0].tolist()
    assert all(status[w] == M.HEALTHY for w in (low, dead, ejected, back))
    all_ok = M.DF_VALIDATED | M.DF_WHITELISTED | M.DF_ACTIVE
    row_endpoint = list(range(W))
    rows = [(back, W, W, M.DF_VALIDATED | M.DF_ACTIVE, 0, 0),         # moved to endpoint W, not whitelisted
            (low, low, low, all_ok | M.DF_BALANCE_ZERO, 0, 0),
            (M.DISC_NEW, W + 1, 0, all_ok, 0, 0),
            (dead, dead, dead, M.DF_VALIDATED | M.DF_WHITELISTED, 0, 0),  # inactive, no stamp
            (ejected, ejected, ejected, M.DF_VALIDATED | M.DF_ACTIVE, 0, 0)]
    want, want_status, _, _ = M.parallel_pass(status, row_endpoint, rows, NOW, 1)
    assert [r["updates"] for r in want] == [[(M.HEALTHY, M.EJECTED)], [(M.HEALTHY, M.LOWBALANCE)], [],
                                            [(M.HEALTHY, M.DEAD)], [(M.HEALTHY, M.EJECTED)]]
    assert want[0]["final_status"] == M.HEALTHY and want[2]["ops"] == M.DO_ADMIT
    np_rows = np.array(rows, dtype=E.disc_row_dt)
    oa, ta = a.discovery_sync(NOW, row_endpoint, W + 2, 1, np_rows, apply=True)
    ob, tb = b.discovery_sync(NOW, row_endpoint, W + 2, 1, np_rows, apply=False)
    assert _as_dicts(oa) == _as_dicts(ob) == want and ta == tb == 4
    assert a.liveness_get()[0].tolist() == b.liveness_get()[0].tolist() == want_status
    # by hand: every update in discovery order, then the put-back's entry
    hw, hf, hd = [], [], []
    for r, res in zip(rows, want):
        for _, new in res["updates"]:
            hw.append(r[0]); hf.append(int(flags[r[0]]) & ~E.W_HEALTHY); hd.append(int(new in (M.DEAD, M.LOWBALANCE)))
            st.set_node_status(int(r[0]), int(new))
        if res["updates"] and res["final_status"] == M.HEALTHY:
            hw.append(r[0]); hf.append(int(flags[r[0]]) | E.W_HEALTHY); hd.append(0)
            st.set_node_status(int(r[0]), M.HEALTHY)
    assert hw == [back, back, low, dead, ejected]
    b.on_worker_status_many(np.array(hw, dtype=np.uint32), np.array(hf, dtype=np.uint32), np.array(hd, dtype=np.uint32))
    left = {g[0] for g in engine_groups(a)}
    assert quads[0][0] not in left and quads[1][0] not in left and quads[2][0] in left and solo[0] in left
    assert all(a.lookup(int(w)).group_size == 0 for w in quads[0][2] + quads[1][2])
    assert engine_groups(a) == engine_groups(b)
    assert a.drain_group_events() == b.drain_group_events()
    assert _lookups(a, W) == _lookups(b, W)
    sa, sb = a.tick(), b.tick()
    st.try_form_new_groups()
    st.try_merge_solo_groups()
    la = _lookups(a, W)
    assert la == _lookups(b, W)
    assert [(-1 if t[0] == NONE else t[0]) for t in la] == [st.get_task_for_node(w) for w in range(W)]
    assert sorted(engine_groups(a)) == sorted(engine_groups(b)) == sorted(oracle_groups(st))
    ca, cb = a.drain_assignment_changes(), b.drain_assignment_changes()
    assert ca[0].tolist() == cb[0].tolist() and ca[1].tolist() == cb[1].tolist() and ca[2] == cb[2]
    assert a.drain_group_events() == b.drain_group_events()
    assert sa["n_formed"] == sb["n_formed"]
    assert a.lookup(int(back)).group_size > 0                             # put back to Healthy: still eligible, still used
    assert a.lookup(int(low)).group_size == 0 and a.lookup(int(dead)).group_size == 0
    a.close(), b.close()


# ------------------------------------------------------------------------------------------------ ledger, interplay, errors

def test_a_sweep_after_a_sync_starts_from_the_synced_statuses(eng):
    store, discovery, now, max_same = M.seeded_case(12345, W=130, D=100, n_ep=4)
    _, abi = _sync_both(eng, store, discovery, now, max_same)
    s, c = eng.liveness_get()
    W = len(s)
    led = LM.Ledger(_flags_of(abi["status"]), 3)
    led.set(np.arange(W), s, c)
    beats = np.where(np.arange(W) % 2 == 0, now - 5, 0).astype(np.uint64)
    rows, census = led.sweep(now + 1, beats, None)
    n, got_census = eng.liveness_sweep(now + 1, beats, None)
    assert n == len(rows) and got_census.tolist() == census
    s, c = eng.liveness_get()
    assert s.tolist() == led.status and c.tolist() == led.counter


def _code(call):
    with pytest.raises(E.EngineError) as ei:
        call()
    return ei.value.code


def test_errors_leave_the_ledger_byte_identical():
    e = E.Engine()
    good = np.array([(0, 0, 0, 7, 0, 0)], dtype=E.disc_row_dt)
    assert _code(lambda: e.discovery_sync(NOW, None, 1, 1, good)) == ESTATE              # liveness off
    e.liveness_enable(True, 3)
    assert _code(lambda: e.discovery_sync(NOW, None, 1, 1, good)) == ESTATE              # no workers yet
    W = 70
    status = [M.HEALTHY, M.DEAD, M.UNHEALTHY, M.EJECTED, M.DISCOVERED] * 14
    _load(e, status)
    ep = np.arange(W, dtype=np.uint32) % 5
    before = [x.tolist() for x in e.liveness_get()]

    def refused(code, rows, row_endpoint=ep, n_endpoints=5):
        r = np.array(rows, dtype=E.disc_row_dt)
        for apply in (False, True):
            assert _code(lambda: e.discovery_sync(NOW, row_endpoint, n_endpoints, 1, r, apply=apply)) == code
        assert [x.tolist() for x in e.liveness_get()] == before

    demote = (0, 0, 0, M.DF_VALIDATED | M.DF_ACTIVE, 0, 0)                                           # (would eject row 0 if it ran)
    refused(EINVAL, [demote, (1, 1, 1, 64, 0, 0)])                                       # an unknown flag bit
    refused(EINVAL, [demote, (5, 0, 0, 7, 0, 0), (0, 0, 0, 7, 0, 0)])                    # a table row twice
    refused(EINVAL, [demote], n_endpoints=W + 2 + 1)                                     # more ids than anyone can name
    refused(EINVAL, [demote], row_endpoint=None)                                         # a NULL column
    refused(ERANGE, [demote, (W, 0, 0, 7, 0, 0)])                                        # a row behind the table
    refused(ERANGE, [demote, (1, 5, 1, 7, 0, 0)])                                        # the key
    refused(ERANGE, [demote, (1, 1, 5, 7, 0, 0)])                                        # endpoint_after of a table row
    refused(ERANGE, [demote, (M.DISC_NEW, 5, 0, 7, 0, 0)])                               # the key of a new row
    bad = ep.copy()
    bad[W - 1] = 5
    refused(ERANGE, [demote], row_endpoint=bad)
    assert E.lib().pm_discovery_sync(e._h, NOW, ep.ctypes.data, 5, 1, None, 3, 0, None, None) == EINVAL  # NULL rows
    # what is not an error: endpoint_after of a new row is ignored; PM_EP_NONE in the column; no rows at all
    out, total = e.discovery_sync(NOW, ep, 5, 1, np.zeros(0, dtype=E.disc_row_dt), apply=True)
    assert len(out) == 0 and total == 0 and [x.tolist() for x in e.liveness_get()] == before
    none = ep.copy()
    none[1] = M.EP_NONE
    out, total = e.discovery_sync(NOW, none, 5, 1, np.array([(M.DISC_NEW, 4, 99, 7, 0, 0)], dtype=E.disc_row_dt))
    assert total == 0 and [x.tolist() for x in e.liveness_get()] == before
    out, total = e.discovery_sync(NOW, ep, 5, 1, np.array([demote], dtype=E.disc_row_dt))  # and the demotion, when it runs
    assert total == 1 and e.liveness_get()[0][0] == M.EJECTED
    e.close()


def test_inside_a_stepwise_tick_the_call_is_refused():
    sw = make_swarm(5, 40, 200)
    e = E.Engine()
    host.load_swarm(e, sw)
    e.liveness_enable(True, 3)
    before = [x.tolist() for x in e.liveness_get()]
    rows = np.array([(0, 0, 0, 7 | M.DF_BALANCE_ZERO, 0, 0)], dtype=E.disc_row_dt)
    ep = np.arange(sw.W, dtype=np.uint32)
    e.dist_configure(0, 1)
    e.dist_tick_begin()
    assert _code(lambda: e.discovery_sync(NOW, ep, sw.W, 1, rows)) == ESTATE
    assert _code(lambda: e.discovery_sync(NOW, ep, sw.W, 1, rows, apply=True)) == ESTATE
    e.dist_carve_wait()
    e.dist_match_begin()
    e.dist_tick_end()
    assert [x.tolist() for x in e.liveness_get()] == before
    out, total = e.discovery_sync(NOW, ep, sw.W, 1, rows)
    assert total == 1 and e.liveness_get()[0][0] == M.LOWBALANCE
    e.close()
