"""The group geography reports on the GPU (pm_group_spread, pm_config_spread) and pm_force_regroup against the model of
tests/spread_model.py (the oracle's calculate_distance, the BTreeSet ring, the "{:x}" order).  Groups are installed with
pm_adopt_groups, so their shapes are chosen exactly: every size at which the kernels change path (the wave path up to 64
members, the workgroup path and its tiles of 256 above), every located share, five coordinate mixes.

Tolerances: diameter_km, longest_hop_km within relative 1e-12 of the oracle (hav_a's error ~2e-15 reaches d multiplied by at
most 1 / (2 sqrt(1 - a)) ~ 16 for a <= 0.999, plus a few ulp of sqrt / atan2; tests/test_spread_model.py checks a tenth of it
on the CPU), ring_km within 1e-11 (up to 300 terms summed in another order)."""
import json
import os
import sys

import numpy as np
import pytest

from oracle import oracle_ffi as orc
from protocol_amd import engine as E
from protocol_amd import host
from protocol_amd.churn import ChurnStream
from protocol_amd.swarm import baseline_config

import spread_model as SM

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from make_golden_churn import CHURN_SEED, CHURN_TICKS_PINNED, CHURN_TICKS_PLANNED, events_digest, sha  # noqa: E402

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "churn_digests.json")))
TOL, TOL_RING, KM_AT_A_0_999 = SM.TOL, SM.TOL_RING, SM.KM_AT_A_0_999
BASE = E.W_HEALTHY | E.W_HAS_P2P
BERLIN, NEW_YORK = (52.52, 13.405), (40.7128, -74.006)

# (members, located share, coordinate mix): the first ten alternate between the wave path and the workgroup path in slot
# order; the rest are small groups for the shares and mixes the large ones leave out
SPECS = [(1, "all", "world"), (65, "all", "city"), (2, "all", "two"), (255, "two", "world"), (3, "all", "far"),
         (256, "all", "ulp"), (63, "all", "world"), (257, "one", "world"), (64, "all", "two"), (300, "all", "far"),
         (1, "none", "world"), (2, "one", "world"), (2, "none", "city"), (3, "two", "world"), (3, "all", "ulp"),
         (2, "all", "same"), (3, "none", "two"), (64, "two", "city"), (63, "none", "world"), (65, "none", "world"),
         (3, "all", "city"), (2, "all", "far"), (3, "all", "world"), (2, "all", "city"), (3, "all", "same")]
N_FREE = 150      # workers in no group, for the tick that forms more
EXACT_TIES = ("two", "same")


def coordinates(rng, n, mix):
    if mix == "world":
        return rng.uniform(-50.0, 60.0, n), rng.uniform(-100.0, 50.0, n)
    if mix == "city":       # within 1 km of one centre
        return 48.8566 + rng.uniform(-0.003, 0.003, n), 2.3522 + rng.uniform(-0.004, 0.004, n)
    if mix == "two":        # two sites only: every pair across ties
        k = np.arange(n) % 2
        return np.where(k == 0, BERLIN[0], NEW_YORK[0]).astype(float), np.where(k == 0, BERLIN[1], NEW_YORK[1]).astype(float)
    if mix == "same":       # bit-identical coordinates
        return np.full(n, 35.6762), np.full(n, 139.6503)
    if mix == "ulp":        # a few ulp apart
        lat, lon = np.full(n, 35.6762), np.full(n, 139.6503)
        for _ in range(3):
            step = rng.integers(0, 2, n).astype(bool)
            lat = np.where(step, np.nextafter(lat, 90.0), lat)
            step = rng.integers(0, 2, n).astype(bool)
            lon = np.where(step, np.nextafter(lon, 180.0), lon)
        return lat, lon
    assert mix == "far"     # a cluster, and one member about 19,000 km from it
    lat, lon = 10.0 + rng.uniform(-0.5, 0.5, n), 10.0 + rng.uniform(-0.5, 0.5, n)
    lat[n - 1], lon[n - 1] = -10.0, -160.87
    return lat, lon


class Fixture:
    def __init__(self):
        rng = np.random.default_rng(977)
        W = sum(s[0] for s in SPECS) + N_FREE
        self.W = W
        flags = np.full(W, BASE, dtype=np.uint32)
        lat, lon = np.zeros(W), np.zeros(W)
        self.groups = []   # (id, config, members in carve order)
        perm = rng.permutation(W)  # which rows a group's members are: anywhere in the table
        at = 0
        ids = rng.integers(1, 1 << 62, len(SPECS), dtype=np.uint64)
        ids[4], ids[2] = 0x10, 0x9                              # "10" < "9" among the ids of configuration 0
        for k, (n, share, mix) in enumerate(SPECS):
            ws = perm[at:at + n]
            at += n
            la, lo = coordinates(rng, n, mix)
            lat[ws], lon[ws] = la, lo
            nloc = {"none": 0, "one": 1, "two": 2, "all": n}[share]
            flags[ws[rng.permutation(n)[:nloc]]] |= E.W_HAS_LOC
            self.groups.append((int(ids[k]), k % 2, [int(w) for w in ws]))
        free = perm[at:]
        lat[free], lon[free] = coordinates(rng, len(free), "world")
        flags[free] |= E.W_HAS_LOC
        self.free = free
        z = np.zeros(W, dtype=np.uint32)
        self.cols = dict(flags=flags, gpu_count=z, gpu_mem_mb=z, gpu_model_class=z, cpu_cores=z, ram_mb=z, storage_gb=z,
                         price=z, addr_rank=rng.permutation(W).astype(np.uint32), lat=lat, lon=lon)
        self.cfg_rows, self.alt_rows, _ = host.pack_configs([("a", 1, 300, None), ("b", 1, 300, None)])
        self.rows = model_rows(self.groups, flags, lat, lon, self.cols["addr_rank"])
        # no pair the kernels look at has a > 0.999 (the tolerance's derivation stops there)
        assert max(r["diameter_km"] for r in self.rows) <= KM_AT_A_0_999
        assert max(r["diameter_km"] for r in self.rows) > 18_900.0
        assert [(r["located"]) for r in self.rows[:10]] == [1, 65, 2, 2, 3, 256, 63, 1, 64, 300]

    def engine(self, adopt=True, **kw):
        eng = E.Engine(group_id_seed=5, **kw)
        eng.set_configs(self.cfg_rows, self.alt_rows)
        eng.upload_workers(self.cols)
        eng.upload_tasks(np.array([3, 1, 2], dtype=np.uint64), np.array([30, 20, 10], dtype=np.int64),
                         np.array([7, 8, 9], dtype=np.uint64))
        eng.set_enabled_mask(3)
        if adopt:
            adopt_groups(eng, self.groups)
        return eng


def adopt_groups(eng, groups, id_state=12345):
    g = np.zeros(len(groups), dtype=E.group_dt)
    members = []
    for k, (gid, cfg, mem) in enumerate(groups):
        g[k]["id"], g[k]["config"], g[k]["n_members"], g[k]["member_begin"], g[k]["task"] = gid, cfg, len(mem), len(members), NONE
        members += mem
    eng.adopt_groups(g, np.array(members, dtype=np.uint32), id_state)


def model_rows(groups, flags, lat, lon, rank):
    return [SM.group_spread(g[2], flags, lat, lon, rank) for g in groups]


@pytest.fixture(scope="module")
def fx():
    return Fixture()


close = SM.close


def check_rows(got, want, lat, lon, exact=None, tag=""):
    SM.check_rows(got, want, lat, lon, exact, tag)


def check_config_rows(eng, rows, cfg_of_row):
    got = eng.config_spread()
    want = SM.config_spread(rows, cfg_of_row, eng.C)
    assert np.array_equal(got, want), (got, want)
    assert np.array_equal(got["groups"], eng.config_report()["groups"])
    return got


def check_engine(eng, cols, tag, exact_for=None):
    """both reports of an engine in any state against the model built from what pm_get_groups says afterwards"""
    got = eng.group_spread()
    cs = eng.config_spread()
    groups = SM.engine_groups(eng)        # (compacts: the reports above ran on the list as it was)
    want = model_rows(groups, cols["flags"], cols["lat"], cols["lon"], cols["addr_rank"])
    check_rows(got, want, cols["lat"], cols["lon"], exact_for, tag)
    assert np.array_equal(cs, SM.config_spread(got, [g[1] for g in groups], eng.C)), tag
    again = eng.group_spread()            # the compacted list gives the same rows
    assert np.array_equal(again, got), tag
    return got, groups


# ------------------------------------------------------------------ sizes, shares, mixes

def test_every_size_share_and_mix_against_the_model(fx):
    eng = fx.engine()
    exact = [s[2] in EXACT_TIES for s in SPECS]
    got = eng.group_spread()               # the list has not gone up yet: offsets and members from scratch
    check_rows(got, fx.rows, fx.cols["lat"], fx.cols["lon"], exact, "scratch")
    same = [k for k, s in enumerate(SPECS) if s[2] == "same" and s[1] == "all"]
    assert same and all(got[k]["diameter_km"] == 0.0 and got[k]["ring_km"] == 0.0 and got[k]["ring_hops"] == SPECS[k][0]
                        for k in same)
    two = got[2]                            # two located members: there and back
    assert int(two["ring_hops"]) == 2 and close(float(two["ring_km"]), 2.0 * float(two["diameter_km"]), 1e-15)
    check_config_rows(eng, got, [g[1] for g in fx.groups])
    eng.match()                             # the device mirror holds the list now: read in place
    assert np.array_equal(eng.group_spread(), got)
    check_config_rows(eng, got, [g[1] for g in fx.groups])
    hist = eng.config_spread()["hist"].sum(axis=0)
    assert hist[0] > 0 and hist[4] > 0 and int(hist.sum()) == sum(1 for r in fx.rows if r["located"] >= 2)
    eng.close()


# ------------------------------------------------------------------ state

def test_tombstones_compaction_and_a_tick_on_top(fx):
    eng = fx.engine()
    eng.match()
    pushes = eng.debug_delta_pushes()
    # tombstones with the mirror in place: a member of every third group dies
    victims = [g[2][0] for g in fx.groups[::3]]
    flags = fx.cols["flags"].copy()
    flags[victims] &= ~np.uint32(E.W_HEALTHY)
    eng.on_worker_status_many(victims, flags[victims], np.ones(len(victims), dtype=np.uint32))
    cols = dict(fx.cols, flags=flags)
    left = [g for k, g in enumerate(fx.groups) if k % 3]
    got = eng.group_spread()
    want = model_rows(left, flags, cols["lat"], cols["lon"], cols["addr_rank"])
    check_rows(got, want, cols["lat"], cols["lon"], None, "tombstones")
    check_config_rows(eng, got, [g[1] for g in left])
    assert eng.debug_delta_pushes() == pushes
    # pm_dissolve_group of every third of what is left (it compacts), then pm_get_groups
    for slot in range(len(left) - 1, -1, -3):
        eng.dissolve_group(slot)
        left.pop(slot)
    got = eng.group_spread()
    check_rows(got, model_rows(left, flags, cols["lat"], cols["lon"], cols["addr_rank"]), cols["lat"], cols["lon"], None,
               "dissolved")
    assert [g[0] for g in SM.engine_groups(eng)] == [g[0] for g in left]
    assert np.array_equal(eng.group_spread(), got)
    # a tick forms more groups on top of the standing ones
    stats = eng.tick()
    assert stats["n_formed"] > 0
    got, groups = check_engine(eng, cols, "after a tick")
    assert {g[0] for g in groups} - {g[0] for g in left}          # (new ids; the merge pass may have taken solo groups)
    eng.close()


def test_moved_members_pending_flags_and_new_ranks(fx):
    eng = fx.engine()
    eng.match()
    cols = {k: v.copy() for k, v in fx.cols.items()}
    base = eng.group_spread()
    # pm_update_workers moves a member of the one-city group of 65 and one of the 300 far away: the report follows
    movers = np.array([fx.groups[1][2][7], fx.groups[9][2][11], fx.groups[6][2][5]], dtype=np.uint32)
    cols["lat"][movers] = [-33.8688, 61.2, 35.0]
    cols["lon"][movers] = [151.2093, -149.9, -5.0]
    eng.update_workers(movers, {k: np.ascontiguousarray(v[movers]) for k, v in cols.items()})
    got = eng.group_spread()
    want = model_rows(fx.groups, cols["flags"], cols["lat"], cols["lon"], cols["addr_rank"])
    assert max(r["diameter_km"] for r in want) <= KM_AT_A_0_999
    check_rows(got, want, cols["lat"], cols["lon"], None, "moved")
    assert float(got[1]["diameter_km"]) > 10_000.0 > float(base[1]["diameter_km"])
    assert int(got[1]["far_a"]) == int(movers[0]) or int(got[1]["far_b"]) == int(movers[0])
    # pm_on_worker_status without a tick in between: the flags column has not gone up
    lose = [fx.groups[1][2][7], fx.groups[2][2][0], fx.groups[8][2][3]]
    gain = [w for g in (fx.groups[10], fx.groups[16]) for w in g[2]]
    for w in lose:
        cols["flags"][w] &= ~np.uint32(E.W_HAS_LOC)
        eng.on_worker_status(w, int(cols["flags"][w]), False)
    for w in gain:
        cols["flags"][w] |= np.uint32(E.W_HAS_LOC)
        eng.on_worker_status(w, int(cols["flags"][w]), False)
    got = eng.group_spread()
    want = model_rows(fx.groups, cols["flags"], cols["lat"], cols["lon"], cols["addr_rank"])
    check_rows(got, want, cols["lat"], cols["lon"], None, "pending flags")
    assert int(got[2]["located"]) == 1 and int(got[2]["ring_hops"]) == 0 and int(got[10]["located"]) == 1
    assert int(got[16]["located"]) == 3 and float(got[1]["diameter_km"]) < 10.0
    check_config_rows(eng, got, [g[1] for g in fx.groups])
    # other address ranks: the ring changes, the diameter does not
    cols["addr_rank"] = (np.uint32(fx.W - 1) - cols["addr_rank"]).astype(np.uint32)
    cols["addr_rank"][fx.groups[9][2]] = np.random.default_rng(4).permutation(300).astype(np.uint32)  # (ties across groups)
    cols["addr_rank"][fx.groups[6][2]] = 7                                                           # (ties within one)
    eng.set_addr_ranks(cols["addr_rank"])
    ranked = eng.group_spread()
    want = model_rows(fx.groups, cols["flags"], cols["lat"], cols["lon"], cols["addr_rank"])
    check_rows(ranked, want, cols["lat"], cols["lon"], None, "new ranks")
    for f in ("located", "far_a", "far_b", "diameter_km"):
        assert np.array_equal(ranked[f], got[f]), f
    assert float(ranked[9]["ring_km"]) != float(got[9]["ring_km"])
    eng.close()


def test_churn_stream_with_both_reports_between_every_call():
    """the reports change nothing: the oracle's digests through the churn stream, and as many delta pushes as without"""
    def run(with_reports):
        gold = GOLD["churn"]
        eng = E.Engine(group_id_seed=1)
        cs = ChurnStream(CHURN_SEED, CHURN_TICKS_PLANNED)
        sw = cs.sw_all
        packed = host.pack_workers(sw)
        rows = lambda idx: {k: np.ascontiguousarray(v[idx]) for k, v in packed.items()}
        cfg_rows, alt_rows, req_models = host.pack_configs(sw.configs)
        eng.set_configs(cfg_rows, alt_rows)
        eng.set_model_table(host.build_model_table(req_models, sw.model_names), len(req_models), len(sw.model_names))
        eng.upload_workers(rows(np.arange(cs.W0)))
        eng.upload_tasks(cs.masks, cs.created, cs.uid)
        eng.set_enabled_mask(sw.enabled_mask())
        eng.enable_group_events()
        flags = packed["flags"].astype(np.int64).copy()
        n = [0]

        def report():
            if not with_reports:
                return
            g, c = eng.group_spread(), eng.config_spread()          # (nothing here may compact the list: no pm_get_groups)
            assert np.array_equal(c["groups"], eng.config_report()["groups"]) and int(c["groups"].sum()) == len(g)
            m = g[g["located"] >= 2]
            assert int(c["measured"].sum()) == len(m) == int(c["hist"].sum())
            assert int(c["sum_diameter_m"].sum()) == int(np.rint(m["diameter_km"] * 1000.0).astype(np.int64).sum())
            assert int(c["sum_ring_m"].sum()) == int(np.rint(g["ring_km"][g["ring_hops"] >= 1] * 1000.0).astype(np.int64).sum())
            assert float(c["max_diameter_km"].max()) == (float(m["diameter_km"].max()) if len(m) else 0.0)
            n[0] += 1

        def check(W, g, stats, tag):
            assert stats["n_formed"] == g["n_formed"] and stats["n_groups"] == g["n_groups"], (tag, stats)
            col = np.array([eng.lookup(w).task for w in range(W)], dtype=np.uint32)
            assert sha(col) == g["task_sha256"], f"{tag}: per-worker tasks differ from the oracle"
            ev = eng.drain_group_events()
            assert len(ev) == g["n_events"] and events_digest(ev) == g["events_sha256"], f"{tag}: life-cycle feed"

        report()
        check(cs.W0, gold["cold"], eng.tick(), "cold")
        report()
        for k in range(CHURN_TICKS_PINNED):
            leave, idx_new, new_tasks = cs.step()
            flags[leave] &= ~E.W_HEALTHY
            eng.on_worker_status_many(leave, flags[leave], np.ones(len(leave), dtype=np.uint32))
            report()
            eng.append_workers(rows(idx_new))
            report()
            eng.tasks_insert_front(*new_tasks[:3])
            report()
            check(cs.W, gold["ticks"][k], eng.tick(), f"tick {k}")
            report()
        pushes = eng.debug_delta_pushes()
        eng.close()
        return pushes, n[0]

    pushes, n = run(True)
    assert n == 2 + 4 * CHURN_TICKS_PINNED
    assert pushes == run(False)[0]


# ------------------------------------------------------------------ pm_force_regroup

def destroyed(eng):
    ev = eng.drain_group_events()
    assert all(e[0] == E.GROUP_DESTROYED for e in ev), ev
    return [e[1] for e in ev]


def test_force_regroup_all_is_the_route(fx):
    a, b = fx.engine(), fx.engine()
    for e in (a, b):
        e.tick()                                                  # groups on top of the adopted ones, a table published
        e.enable_group_events()
    groups = SM.engine_groups(a)
    assert SM.engine_groups(b) == groups
    want = SM.regroup_selection(groups, [None] * len(groups), 0, E.REGROUP_ALL, 0.0)
    texts = [SM.id_text(g[0]) for g in want]
    assert texts == sorted(texts) and texts.index("10") < texts.index("9")
    assert [int(t, 16) for t in texts] != sorted(int(t, 16) for t in texts)
    n_g, n_w = a.force_regroup(0, E.REGROUP_ALL, float("nan"))    # (the threshold is ignored)
    assert n_g == len(want) and n_w == sum(len(g[2]) for g in want)
    assert destroyed(a) == [g[0] for g in want]
    for g in want:
        for w in g[2][:3]:
            r = a.lookup(w)
            assert r.group_slot == NONE and r.task == NONE, (g[0], w)
        assert b.dissolve_group_by_id(g[0])                       # the same groups one by one, in that order
    assert destroyed(b) == [g[0] for g in want]
    rest = [g for g in groups if g[1] != 0]
    assert SM.engine_groups(a) == rest == SM.engine_groups(b)     # the other configuration's groups are untouched
    assert a.config_spread()["groups"].tolist() == [0, len(rest)]
    sa, sb = a.tick(), b.tick()
    assert sa["n_formed"] == sb["n_formed"] > 0
    assert SM.engine_groups(a) == SM.engine_groups(b)
    assert a.drain_group_events() == b.drain_group_events()
    assert [a.lookup(w).task for w in range(fx.W)] == [b.lookup(w).task for w in range(fx.W)]
    a.close(), b.close()


def gaps(values):
    """thresholds in the middle of the gaps between consecutive distinct values; every gap is at least 1e-6 relative"""
    v = sorted(set(values))
    for lo, hi in zip(v, v[1:]):
        assert hi - lo >= 1e-6 * hi, (lo, hi)
    return [(lo + hi) / 2.0 for lo, hi in zip(v, v[1:])]


@pytest.mark.parametrize("metric", [E.REGROUP_DIAMETER, E.REGROUP_LONGEST_HOP])
def test_force_regroup_by_metric(fx, metric):
    field, need = ("diameter_km", lambda r: r["located"] >= 2) if metric == E.REGROUP_DIAMETER else \
        ("longest_hop_km", lambda r: r["ring_hops"] >= 1)
    for cfg in (0, 1):
        mine = [k for k, g in enumerate(fx.groups) if g[1] == cfg]
        measured = [fx.rows[k][field] for k in mine if need(fx.rows[k])]
        unmeasured = [fx.groups[k][0] for k in mine if not need(fx.rows[k])]
        assert unmeasured and len(set(measured)) >= 4
        cuts = gaps(measured)
        for thr in (cuts[0], cuts[len(cuts) // 2], cuts[-1], 0.0):
            eng = fx.engine()
            eng.enable_group_events()
            want = SM.regroup_selection(fx.groups, fx.rows, cfg, metric, thr)
            assert (thr == 0.0) == (len(want) == len(measured))
            n_g, n_w = eng.force_regroup(cfg, metric, thr)
            assert (n_g, n_w) == (len(want), sum(len(g[2]) for g in want)), (cfg, thr)
            assert destroyed(eng) == [g[0] for g in want]
            gone = {g[0] for g in want}
            assert [g[0] for g in SM.engine_groups(eng)] == [g[0] for g in fx.groups if g[0] not in gone]
            if thr == 0.0:                                          # located < 2 survives a metric and falls to ALL
                assert eng.force_regroup(cfg, metric, 0.0) == (0, 0)
                assert eng.force_regroup(cfg, E.REGROUP_ALL)[0] == len(unmeasured)
                assert sorted(destroyed(eng)) == sorted(unmeasured)
            eng.close()
        eng = fx.engine()                                           # above every value: nothing
        eng.enable_group_events()
        assert eng.force_regroup(cfg, metric, max(measured) * (1.0 + 1e-6)) == (0, 0)
        assert destroyed(eng) == [] and len(eng.group_spread()) == len(fx.groups)
        eng.close()


# ------------------------------------------------------------------ refusals

def test_refusals(fx):
    L = E.lib()
    u32 = E.C.c_uint32
    eng = E.Engine()
    n = u32(77)
    assert L.pm_group_spread(eng._h, None, 0, E.C.byref(n)) == E.PM_ESTATE
    assert L.pm_config_spread(eng._h, None, 0, E.C.byref(n)) == E.PM_ESTATE
    assert L.pm_force_regroup(eng._h, 0, 0, 0.0, None, None) == E.PM_ESTATE
    eng.set_configs(fx.cfg_rows, fx.alt_rows)
    assert L.pm_group_spread(eng._h, None, 0, E.C.byref(n)) == E.PM_ESTATE    # no workers yet
    eng.close()
    eng = fx.engine(adopt=False)
    assert L.pm_group_spread(eng._h, None, 0, E.C.byref(n)) == 0 and n.value == 0
    assert len(eng.group_spread()) == 0 and eng.config_spread()["groups"].tolist() == [0, 0]
    assert eng.force_regroup(1) == (0, 0)
    adopt_groups(eng, fx.groups)
    G = len(fx.groups)
    out = np.full(G, 0xAB, dtype=np.uint8).repeat(48).view(E.group_spread_dt)
    keep = out.copy()
    assert L.pm_group_spread(eng._h, out.ctypes.data, G - 1, E.C.byref(n)) == E.PM_ERANGE and n.value == G
    assert out.tobytes() == keep.tobytes()
    assert L.pm_group_spread(eng._h, None, 0, None) == E.PM_ERANGE
    cout = np.full(2 * 64, 0xAB, dtype=np.uint8).view(E.config_spread_dt)
    ckeep = cout.copy()
    assert L.pm_config_spread(eng._h, cout.ctypes.data, 1, E.C.byref(n)) == E.PM_ERANGE and n.value == 2
    assert cout.tobytes() == ckeep.tobytes()
    g, w = u32(5), u32(5)
    assert L.pm_force_regroup(eng._h, 2, 0, 0.0, E.C.byref(g), E.C.byref(w)) == E.PM_ERANGE
    assert L.pm_force_regroup(eng._h, 0, 3, 0.0, E.C.byref(g), E.C.byref(w)) == E.PM_EINVAL
    assert L.pm_force_regroup(eng._h, 0, E.REGROUP_DIAMETER, float("nan"), None, None) == E.PM_EINVAL
    assert L.pm_force_regroup(eng._h, 0, E.REGROUP_LONGEST_HOP, -1.0, None, None) == E.PM_EINVAL
    assert len(eng.group_spread()) == G                                         # nothing was dissolved
    eng.dist_configure(0, 1)
    eng.dist_tick_begin()
    assert L.pm_group_spread(eng._h, out.ctypes.data, G, E.C.byref(n)) == E.PM_ESTATE
    assert L.pm_config_spread(eng._h, cout.ctypes.data, 2, E.C.byref(n)) == E.PM_ESTATE
    assert L.pm_force_regroup(eng._h, 0, 0, 0.0, None, None) == E.PM_ESTATE
    eng.dist_carve_wait()
    eng.dist_match_begin()
    eng.dist_tick_end()
    check_engine(eng, fx.cols, "after a stepwise tick")
    eng.close()


# ------------------------------------------------------------------ one run at size

def test_baseline_config_1_at_full_size():
    sw = baseline_config(1, seed=1)
    eng = E.Engine()
    host.load_swarm(eng, sw)
    eng.tick()
    cols = host.pack_workers(sw)
    got, groups = check_engine(eng, cols, "baseline 1")
    measured = got["located"] >= 2
    assert measured.sum() > 1000
    # the inputs: a proximity-formed swarm is tighter than the same workers in random groups of the same sizes (the oracle's
    # numbers, on a sample of the groups)
    rng = np.random.default_rng(8)
    members = np.concatenate([g[2] for g in groups])
    shuffled = rng.permutation(members)
    cut = np.cumsum([0] + [len(g[2]) for g in groups])
    random_groups = [(g[0], g[1], shuffled[cut[k]:cut[k + 1]].tolist()) for k, g in enumerate(groups)]
    other = E.Engine()
    host.load_swarm(other, sw)
    adopt_groups(other, random_groups)
    rnd = other.group_spread()
    pick = rng.choice(len(groups), 300, replace=False)
    want = model_rows([random_groups[k] for k in pick], cols["flags"], cols["lat"], cols["lon"], cols["addr_rank"])
    check_rows(rnd[pick], want, cols["lat"], cols["lon"], None, "random groups")
    formed = model_rows([groups[k] for k in pick], cols["flags"], cols["lat"], cols["lon"], cols["addr_rank"])
    med = lambda rows: float(np.median([r["diameter_km"] for r in rows if r["located"] >= 2]))
    print(f"\nmedian diameter of {len(pick)} groups: formed by proximity {med(formed):.1f} km, random {med(want):.1f} km")
    assert med(formed) < med(want)
    eng.close(), other.close()
