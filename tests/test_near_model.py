"""The model of pm_nearest_workers (tests/near_model.py) against hand-built cases of the reference's rules, and the
guarantee of its fixture generator.  CPU only."""
import numpy as np
import pytest

from oracle import oracle_ffi as orc
from protocol_amd import engine as E

import near_model as NM

BASE = E.W_HEALTHY | E.W_HAS_P2P
LOC = BASE | E.W_HAS_LOC
NONE = NM.NONE


def table(flags, lat=None, lon=None, group_of=None, compat=None):
    n = len(flags)
    return dict(compat=np.full(n, 1, dtype=np.uint64) if compat is None else np.asarray(compat, dtype=np.uint64),
                flags=np.asarray(flags, dtype=np.uint32), group_of=np.full(n, -1) if group_of is None else np.asarray(group_of),
                lat=np.zeros(n) if lat is None else np.asarray(lat, dtype=float),
                lon=np.zeros(n) if lon is None else np.asarray(lon, dtype=float))


def test_seed_prefers_a_located_candidate_over_an_earlier_unlocated_one():
    t = table([BASE, BASE, LOC, LOC])
    assert NM.seed(0, t["compat"], t["flags"], t["group_of"]) == 2
    t = table([BASE, LOC, LOC], group_of=[-1, 0, -1])            # (the located one in front is grouped: not in the pool)
    assert NM.seed(0, t["compat"], t["flags"], t["group_of"]) == 2
    t = table([E.W_HAS_P2P, BASE, BASE])                          # no located candidate: the first candidate
    assert NM.seed(0, t["compat"], t["flags"], t["group_of"]) == 1
    t = table([LOC, LOC], compat=[2, 2])                          # nobody meets configuration 0
    assert NM.seed(0, t["compat"], t["flags"], t["group_of"]) == NONE
    r = NM.nearest(E.NEAR_SEED, 0, E.NEAR_ELIGIBLE, 3, **t)
    assert (r["origin"], r["n"], r["candidates"], r["workers"], r["km"]) == (NONE, 0, 0, [NONE] * 3, [NM.F64_MAX] * 3)


def test_the_seed_comes_from_the_idle_pool_whatever_pool_is_asked_for():
    t = table([LOC, LOC, LOC], lat=[0.0, 1.0, 2.0], group_of=[3, -1, -1])
    r = NM.nearest(E.NEAR_SEED, 0, E.NEAR_ELIGIBLE, 4, **t)
    assert r["origin"] == 1 and r["workers"][:2] == [0, 2] and r["candidates"] == 2
    r = NM.nearest(E.NEAR_SEED, 0, E.NEAR_IDLE, 4, **t)
    assert r["origin"] == 1 and r["workers"] == [2, NONE, NONE, NONE] and r["candidates"] == 1


def test_an_unlocated_origin_keeps_index_order():
    t = table([BASE, LOC, LOC, BASE, LOC], lat=[0.0, 50.0, 1.0, 0.0, 20.0])
    r = NM.nearest(0, 0, E.NEAR_IDLE, 8, **t)
    assert r["workers"][:4] == [1, 2, 3, 4] and r["km"] == [NM.F64_MAX] * 8 and (r["n"], r["located"]) == (4, 3)


def test_order_ties_and_the_unlocated_tail():
    # from worker 0: 5 and 2 at bit-identical coordinates (a tie: index order), 4 and 1 mirrored in longitude (a tie too),
    # 3 unlocated and 6 unlocated behind every located one, in index order
    lat = [10.0, 10.0, 12.0, 0.0, 10.0, 12.0, 0.0]
    lon = [20.0, 25.0, 20.0, 0.0, 15.0, 20.0, 0.0]
    t = table([LOC, LOC, LOC, BASE, LOC, LOC, BASE], lat=lat, lon=lon)
    r = NM.nearest(0, 0, E.NEAR_IDLE, 6, **t)
    assert r["workers"] == [2, 5, 1, 4, 3, 6]
    assert r["key"][0] == r["key"][1] and r["key"][2] == r["key"][3] and r["key"][4:] == [NM.F64_MAX] * 2
    assert r["km"][0] == orc.calculate_distance(10.0, 20.0, 12.0, 20.0)
    # the origin is a point to measure from, whatever its own state; it is never in its list
    t["flags"][0] = E.W_HAS_LOC
    t["group_of"][0] = 7
    t["compat"][0] = 0
    assert NM.nearest(0, 0, E.NEAR_IDLE, 6, **t)["workers"] == [2, 5, 1, 4, 3, 6]


def test_k_above_and_below_the_candidate_count():
    t = table([LOC] * 5, lat=[0.0, 4.0, 3.0, 2.0, 1.0])
    r = NM.nearest(0, 0, E.NEAR_IDLE, 7, **t)
    assert (r["n"], r["candidates"]) == (4, 4) and r["workers"] == [4, 3, 2, 1, NONE, NONE, NONE]
    assert r["km"][4:] == [NM.F64_MAX] * 3 and r["km"][:4] == sorted(r["km"][:4])
    r = NM.nearest(0, 0, E.NEAR_IDLE, 2, **t)
    assert (r["n"], r["candidates"]) == (2, 4) and r["workers"] == [4, 3]


def test_pools_and_compat_filter():
    t = table([LOC] * 6, lat=[0, 1, 2, 3, 4, 5], group_of=[-1, 2, -1, -1, -1, -1], compat=[3, 3, 1, 2, 3, 3])
    t["flags"][4] = E.W_HAS_P2P | E.W_HAS_LOC        # unhealthy
    t["flags"][5] = E.W_HEALTHY | E.W_HAS_LOC        # no p2p id
    assert NM.nearest(0, 1, E.NEAR_IDLE, 4, **t)["workers"] == [3, NONE, NONE, NONE]
    assert NM.nearest(0, 1, E.NEAR_ELIGIBLE, 4, **t)["workers"] == [1, 3, NONE, NONE]
    assert NM.nearest(0, 0, E.NEAR_ELIGIBLE, 4, **t)["workers"] == [1, 2, NONE, NONE]


@pytest.mark.parametrize("seed", [1, 2])
def test_separated_fixture_guarantee(seed):
    rng = np.random.default_rng(seed)
    n = 220
    lat, lon = NM.separated_coordinates(rng, n, twins=6, mirrors=4)
    assert NM.is_separated(range(n), lat, lon)
    # the exact ties are there: twins of an earlier row, and pairs mirrored about row 0's longitude
    d0 = orc.distance_column(float(lat[0]), float(lon[0]), np.ascontiguousarray(lat), np.ascontiguousarray(lon))
    pairs = [(n - 1 - 2 * j, n - 2 - 2 * j) for j in range(4)]
    assert all(d0[a] == d0[b] and lon[a] != lon[b] and lat[a] == lat[b] == lat[0] for a, b in pairs)
    coords = list(zip(lat.tolist(), lon.tolist()))
    assert sum(1 for t in range(n - 8 - 6, n - 8) if coords.count(coords[t]) >= 2) == 6
    # and the check is not vacuous: two rows whose distances differ by about 1e-12 relatively fail it
    lat2, lon2 = lat.copy(), lon.copy()
    lat2[5], lon2[5] = lat[6], lon[6] + 1e-9
    assert d0[6] > 100.0 and orc.calculate_distance(lat[0], lon[0], lat2[5], lon2[5]) != d0[6]
    assert not NM.is_separated([0], lat2, lon2)
