"""tests/spread_model.py (the model the GPU tests of the group geography reports compare against) against brute force on
hand cases, and the CPU check of the GPU tests' distance tolerance: the device's Haversine term, emulated operation by
operation, pushed through sqrt / atan2, against the oracle's calculate_distance."""
import itertools

import numpy as np

from oracle import oracle_ffi as orc
from protocol_amd import engine as E

import distance_key_model as DK
import spread_model as SM

LOC = E.W_HAS_LOC
NONE = SM.NONE
# a handful of places (lat, lon)
P = [(52.52, 13.405), (48.8566, 2.3522), (40.7128, -74.006), (-33.8688, 151.2093), (35.6762, 139.6503), (52.52, 13.405)]


def brute(members, flags, lat, lon, rank):
    """the definitions, spelled out with calculate_distance alone"""
    d = lambda a, b: orc.calculate_distance(float(lat[a]), float(lon[a]), float(lat[b]), float(lon[b]))
    loc = [w for w in members if flags[w] & LOC]
    pairs = [(min(a, b), max(a, b)) for a, b in itertools.combinations(loc, 2)]
    diam = max((d(a, b) for a, b in pairs), default=0.0)
    far = min(((a, b) for a, b in pairs if d(a, b) == diam), default=(NONE, NONE))
    ring = sorted(members, key=lambda w: (rank[w], w))
    hops = []
    for i, w in enumerate(ring):
        nx = ring[(i + 1) % len(ring)]
        if nx != w and flags[w] & LOC and flags[nx] & LOC:
            hops.append((w, d(w, nx)))
    longest = max((h[1] for h in hops), default=0.0)
    return dict(located=len(loc), ring_hops=len(hops), far_a=far[0], far_b=far[1], diameter_km=diam,
                ring_km=sum(h[1] for h in hops), longest_hop_km=longest,
                hop_from=min((h[0] for h in hops if h[1] == longest), default=NONE))


def columns(n, located="all"):
    lat = np.array([P[i % len(P)][0] for i in range(n)])
    lon = np.array([P[i % len(P)][1] for i in range(n)])
    flags = np.zeros(n, dtype=np.uint32)
    if located == "all":
        flags[:] = LOC
    elif located == "one":
        flags[n // 2] = LOC
    return flags, lat, lon


def same(got, want):
    for k, v in want.items():
        if isinstance(v, float):
            assert abs(got[k] - v) <= 1e-12 * max(abs(v), 1.0), (k, got[k], v)
        else:
            assert got[k] == v, (k, got[k], v)


def test_sizes_one_two_three_and_located_shares():
    for n in (1, 2, 3):
        for located in ("none", "one", "all"):
            flags, lat, lon = columns(n, located)
            rank = np.arange(n)
            got = SM.group_spread(list(range(n)), flags, lat, lon, rank)
            same(got, brute(list(range(n)), flags, lat, lon, rank))
            if located != "all" or n == 1:
                assert got["ring_hops"] == 0 and got["far_a"] == NONE and got["hop_from"] == NONE and got["diameter_km"] == 0.0
    flags, lat, lon = columns(2)
    got = SM.group_spread([0, 1], flags, lat, lon)
    d = orc.calculate_distance(*P[0], *P[1])
    assert got["ring_hops"] == 2 and got["ring_km"] == 2 * d and got["diameter_km"] == d    # there and back
    assert (got["far_a"], got["far_b"], got["hop_from"]) == (0, 1, 0)


def test_two_sites_only_every_pair_ties():
    n = 7
    lat = np.array([P[0][0] if i % 2 == 0 else P[2][0] for i in range(n)])
    lon = np.array([P[0][1] if i % 2 == 0 else P[2][1] for i in range(n)])
    flags = np.full(n, LOC, dtype=np.uint32)
    members = [6, 5, 4, 3, 2, 1, 0]
    got = SM.group_spread(members, flags, lat, lon, np.arange(n))
    same(got, brute(members, flags, lat, lon, np.arange(n)))
    assert (got["far_a"], got["far_b"]) == (0, 1) and got["hop_from"] == 0
    assert len(got["pairs_at_max"]) == 4 * 3
    # members at one spot: located, measured, at exactly zero
    lat[:] = P[0][0]
    lon[:] = P[0][1]
    got = SM.group_spread(members, flags, lat, lon, np.arange(n))
    assert got["diameter_km"] == 0.0 and got["ring_km"] == 0.0 and got["ring_hops"] == n
    assert (got["far_a"], got["far_b"], got["hop_from"]) == (0, 1, 0)


def test_addr_rank_reversed_changes_the_ring_not_the_diameter():
    n = 5
    flags, lat, lon = columns(n)
    fwd = SM.group_spread(list(range(n)), flags, lat, lon, np.arange(n))
    shuf = np.array([2, 0, 4, 1, 3])
    mixed = SM.group_spread(list(range(n)), flags, lat, lon, shuf)
    rev = SM.group_spread(list(range(n)), flags, lat, lon, np.arange(n)[::-1].copy())
    same(mixed, brute(list(range(n)), flags, lat, lon, shuf))
    assert fwd["diameter_km"] == mixed["diameter_km"] == rev["diameter_km"]
    assert (fwd["far_a"], fwd["far_b"]) == (mixed["far_a"], mixed["far_b"])
    assert [h[0] for h in rev["hops"]] == [4, 3, 2, 1, 0] and [h[1] for h in rev["hops"]] == [3, 2, 1, 0, 4]
    assert abs(rev["ring_km"] - fwd["ring_km"]) <= 1e-12 * fwd["ring_km"]    # the same cycle the other way round
    assert mixed["ring_km"] != fwd["ring_km"]
    # equal ranks: the worker index decides
    tie = SM.group_spread([3, 1, 2], flags, lat, lon, np.zeros(n, dtype=np.uint32))
    assert [h[0] for h in tie["hops"]] == [1, 2, 3]
    assert SM.ring_order([3, 1, 2]) == [1, 2, 3]


def test_regroup_selection_and_id_text_order():
    assert SM.id_text(16) == "10" and SM.id_text(9) == "9" and SM.id_text(0xABC) == "abc"
    groups = [(9, 0, [0, 1]), (16, 0, [2, 3]), (0xA, 0, [4]), (3, 1, [5, 6]), (0x100, 0, [7, 8])]
    rows = [dict(located=2, ring_hops=2, diameter_km=50.0, longest_hop_km=50.0, ring_km=100.0),
            dict(located=2, ring_hops=2, diameter_km=500.0, longest_hop_km=500.0, ring_km=1000.0),
            dict(located=1, ring_hops=0, diameter_km=0.0, longest_hop_km=0.0, ring_km=0.0),
            dict(located=2, ring_hops=2, diameter_km=5000.0, longest_hop_km=5000.0, ring_km=10000.0),
            dict(located=3, ring_hops=1, diameter_km=700.0, longest_hop_km=20.0, ring_km=20.0004)]
    ids = lambda *a: [g[0] for g in SM.regroup_selection(groups, rows, *a)]
    assert ids(0, E.REGROUP_ALL, 0.0) == [16, 0x100, 9, 0xA]             # "10" < "100" < "9" < "a"
    assert ids(1, E.REGROUP_ALL, 1e9) == [3]
    assert ids(0, E.REGROUP_DIAMETER, 0.0) == [16, 0x100, 9]            # the unlocated one survives a metric
    assert ids(0, E.REGROUP_DIAMETER, 500.0) == [16, 0x100]             # >=
    assert ids(0, E.REGROUP_LONGEST_HOP, 30.0) == [16, 9]
    assert ids(0, E.REGROUP_DIAMETER, 1e6) == []
    cs = SM.config_spread(rows, [g[1] for g in groups], 2)
    assert cs["groups"].tolist() == [4, 1] and cs["measured"].tolist() == [3, 1]
    assert cs["hist"].tolist() == [[0, 1, 2, 0, 0], [0, 0, 0, 0, 1]]
    assert cs["max_diameter_km"].tolist() == [700.0, 5000.0] and cs["max_hop_km"].tolist() == [500.0, 5000.0]
    assert cs["sum_diameter_m"].tolist() == [1_250_000, 5_000_000] and cs["sum_ring_m"].tolist() == [1_120_000, 10_000_000]
    assert SM.bucket(9.999) == 0 and SM.bucket(10.0) == 1 and SM.bucket(5000.0) == 4


def pairs_for_tolerance(n=100_000, seed=20260918):
    """seeded pairs, half world-wide, half clustered (both ends within a degree or so of one centre)"""
    rng = np.random.default_rng(seed)
    h = n // 2
    lat1 = np.concatenate([rng.uniform(-89.0, 89.0, h), rng.uniform(-60.0, 60.0, n - h)])
    lon1 = np.concatenate([rng.uniform(-180.0, 180.0, h), rng.uniform(-179.0, 179.0, n - h)])
    scale = 10.0 ** rng.uniform(-4.0, 0.0, n - h)
    lat2 = np.concatenate([rng.uniform(-89.0, 89.0, h), lat1[h:] + rng.normal(0.0, 1.0, n - h) * scale])
    lon2 = np.concatenate([rng.uniform(-180.0, 180.0, h), lon1[h:] + rng.normal(0.0, 1.0, n - h) * scale])
    return lat1, lon1, lat2, lon2


def test_device_distance_is_within_a_tenth_of_the_gpu_tolerance():
    """The GPU tests allow relative 1e-12 between the device's distance and the oracle's.  Of that, the Haversine term
    (sin_band's polynomial, the cosine column, the last additions) may use a tenth: 100,000 seeded pairs with a <= 0.999,
    the term emulated operation by operation, sqrt / atan2 by numpy, against calculate_distance.  Measured: 4.5e-15 (see
    profiles/r09_spread.txt); the rest is left for OCML's sqrt / atan2 / cos."""
    src = DK.sin_band_source()
    lat1, lon1, lat2, lon2 = pairs_for_tolerance()
    a = np.array([SM.device_a(*p, src, DK.fma, DK.sin_band) for p in
                  zip(lat1.tolist(), lon1.tolist(), lat2.tolist(), lon2.tolist())], dtype=np.float64)
    keep = a <= 0.999
    assert keep.sum() >= 95_000
    want = np.array([orc.calculate_distance(*p) for p in zip(lat1[keep].tolist(), lon1[keep].tolist(), lat2[keep].tolist(),
                                                              lon2[keep].tolist())])
    got = SM.km_of_a(a[keep])
    assert (want > 0).all()
    rel = np.abs(got - want) / want
    print(f"\n{int(keep.sum())} pairs with a <= 0.999: largest relative difference {rel.max():.3e} "
          f"(at a = {a[keep][rel.argmax()]:.6f}, {want[rel.argmax()]:.3f} km)")
    assert rel.max() <= 1e-13
