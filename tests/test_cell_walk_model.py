"""CPU model of the proposer's walk over the spatial index (cell_walk / cell_bound_key in pm_propose.inc), statement by
statement: the enumeration of a ring's runs covers the shell of cells exactly once, the lower bounds are lower bounds,
and a walk that stops by the kernel's rule has seen every candidate below the row's window — so the 64 smallest keys it
holds are the 64 smallest keys of the whole list.  (The GPU tests compare the carves; this pins the geometry.)"""
import numpy as np
import pytest

from cell_walk_model import bound_a, cell_coord, cell_index, ring_runs, unit, walk_float  # noqa: F401  (the model itself)

G_SIZES = (32, 64)


@pytest.mark.parametrize("g", G_SIZES)
def test_rings_cover_every_shell_exactly_once(g):
    rng = np.random.default_rng(3)
    for _ in range(6):
        cx, cy, cz = (int(v) for v in rng.integers(0, g, 3))
        for r in range(0, 7):
            seen = {}
            for (y, z, x0, x1) in ring_runs(r, cx, cy, cz, g):
                for x in range(x0, x1 + 1):
                    seen[(x, y, z)] = seen.get((x, y, z), 0) + 1
            want = {(x, y, z)
                    for x in range(max(cx - r, 0), min(cx + r, g - 1) + 1)
                    for y in range(max(cy - r, 0), min(cy + r, g - 1) + 1)
                    for z in range(max(cz - r, 0), min(cz + r, g - 1) + 1)
                    if max(abs(x - cx), abs(y - cy), abs(z - cz)) == r}
            assert set(seen) == want and all(v == 1 for v in seen.values()), (cx, cy, cz, r)


def _swarm(rng, n):
    lat = np.round(25.0 + 35.0 * rng.random(n), 4)
    ul = rng.random(n) * 110.0
    lon = np.round(np.where(ul < 60.0, -125.0 + ul, -10.0 + (ul - 60.0)), 4)
    city = rng.integers(0, 32, n)
    clat, clon = np.round(25.0 + 35.0 * rng.random(32), 4), np.round(-125.0 + 60.0 * rng.random(32), 4)
    snap = rng.random(n) < 0.4
    return np.where(snap, clat[city], lat), np.where(snap, clon[city], lon)


@pytest.mark.parametrize("g,n", [(32, 9000), (64, 60000)])
def test_walk_sees_everything_below_the_window(g, n):
    rng = np.random.default_rng(g)
    lat, lon = _swarm(rng, n)
    x, y, z = unit(lat, lon)
    h = 2.0 / g
    cells, _, order, start = cell_index(x, y, z, g)
    alive = rng.random(n) < 0.6  # the candidates of the batch: part of what the index holds
    WINDOW = 1.0 + 2.0 ** -20   # (far wider than the kernel's 2^25 ulps)
    visited_total = 0
    for s in rng.choice(np.nonzero(alive)[0], 60, replace=False):
        a_all = 0.25 * ((x - x[s]) ** 2 + (y - y[s]) ** 2 + (z - z[s]) ** 2)
        cand = alive.copy()
        cand[s] = False
        brute = np.sort(a_all[cand])[:64]
        row, seen, _ = walk_float(s, g, x, y, z, cells, order, start, cand, a_all, WINDOW, 14)
        assert np.array_equal(row, brute), s
        # ... and everything within the window of the last entry was offered (the near-miss tracker's domain)
        visited_total += seen
    assert visited_total < 60 * int(cand.sum()) // 8, "the walk looks at a small part of the list"
