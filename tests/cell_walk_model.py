"""CPU model of the proposer's walk over the spatial index (cell_walk / cell_run / cell_bound_key in
protocol_amd/csrc/pm_propose.inc), statement by statement: the grid cell of a coordinate, the runs of a ring, the lower bound of
a run's keys, the walk of one seed over a float model of the keys (tests/test_cell_walk_model.py), and — for
tests/first_batch_cases.py — the ring in front of which the kernel's walk stops, from packed integer keys."""
import struct

import numpy as np

RMAX = 14                      # PM_CELL_RMAX: rings a seed walks before it falls back to the whole list
EMPTY = 0xFFFFFFFFFFFFFFFF
NOLOC = 0x7FEFFFFFFFFFFFFF     # PM_KEY_NOLOC
FLOOR = 0x03B8F2B061AEA073     # bits of 1e-290, rounded up (near_window)


def cell_coord(v, g):
    t = np.maximum((v + 1.0) * (g >> 1), 0.0)
    return np.minimum(t.astype(np.int64), g - 1)


def n_ring_runs(r):
    return 8 * r + 2 * (2 * r - 1) * (2 * r - 1) if r else 1


def ring_runs(r, cx, cy, cz, g):
    """the kernel's run q of ring r -> (y, z, x0, x1) or None when it leaves the grid (same arithmetic as cell_walk)"""
    side, n_full, inner = 2 * r, (8 * r if r else 1), (2 * r - 1 if r else 0)
    n_runs = n_full + 2 * inner * inner
    out = []
    for qi in range(n_runs):
        dy = dz = 0
        x0 = x1 = cx
        if r > 0:
            if qi < n_full:
                sd, t = divmod(qi, side)
                dy = (-r + t, r, r - t, -r)[sd]
                dz = (-r, -r + t, r, r - t)[sd]
                x0, x1 = cx - r, cx + r
            else:
                m = (qi - n_full) >> 1
                dy = m % inner - (r - 1)
                dz = m // inner - (r - 1)
                x0 = x1 = cx + r if (qi - n_full) & 1 else cx - r
        y, z = cy + dy, cz + dz
        if not (0 <= y < g and 0 <= z < g and x1 >= 0 and x0 < g):
            continue
        out.append((y, z, max(x0, 0), min(x1, g - 1)))
    return out


def bound_a(gx, gy, gz):
    gx, gy, gz = (max(v - 1e-9, 0.0) for v in (gx, gy, gz))
    return 0.25 * (gx * gx + gy * gy + gz * gz) * (1.0 - 1e-6)


def unit(lat, lon):
    la, lo = np.radians(lat), np.radians(lon)
    return np.cos(la) * np.cos(lo), np.cos(la) * np.sin(lo), np.sin(la)


def cell_index(x, y, z, g):
    """the counting sort of cell_count / cell_scan / cell_place by numpy: -> (cell coordinates per point, linear cell, the
    points in cell order, cell_start[g^3 + 1])"""
    cxs, cys, czs = cell_coord(x, g), cell_coord(y, g), cell_coord(z, g)
    lin = (czs * g + cys) * g + cxs
    order = np.argsort(lin, kind="stable")
    start = np.searchsorted(lin[order], np.arange(g * g * g + 1))
    return (cxs, cys, czs), lin, order, start


def walk_float(s, g, x, y, z, cells, order, start, cand, a_all, window, max_ring):
    """The walk of seed s over a float model of the keys (a_all: the chord term to every point; `window`: tau_hi = the 64th
    smallest * window + 1e-290): -> (the row's values, candidates offered, the ring it stopped in front of).  Asserts on its
    way that cell_bound_key is a lower bound of every key in a run, and that the rings do not run out before max_ring."""
    h = 2.0 / g
    cxs, cys, czs = cells
    row = np.empty(0)
    tau_hi = np.inf
    cx, cy, cz = int(cxs[s]), int(cys[s]), int(czs[s])
    r, seen = 0, 0
    while True:
        if r >= 2 and bound_a((r - 1) * h, 0.0, 0.0) > tau_hi:
            break
        assert r <= max_ring and r < g, "the walk of the model swarm never runs out of rings"
        for (yy, zz, x0, x1) in ring_runs(r, cx, cy, cz, g):
            xlo, xhi = x0 * h - 1.0, (x1 + 1) * h - 1.0
            ylo, zlo = yy * h - 1.0, zz * h - 1.0
            gx = max(xlo - x[s], x[s] - xhi, 0.0)
            gy = max(ylo - y[s], y[s] - (ylo + h), 0.0)
            gz = max(zlo - z[s], z[s] - (zlo + h), 0.0)
            row_lin = (zz * g + yy) * g
            ent = order[start[row_lin + x0]:start[row_lin + x1 + 1]]
            lb = bound_a(gx, gy, gz)
            if len(ent):
                assert a_all[ent].min() >= lb, "cell_bound_key is a lower bound of every key in the run"
            if lb > tau_hi:
                continue
            ent = ent[cand[ent]]
            seen += len(ent)
            row = np.sort(np.concatenate([row, a_all[ent]]))[:64]
            if len(row) == 64:
                tau_hi = row[63] * window + 1e-290
        r += 1
    return row, seen, r


# ---- the kernel's stop rule on packed integer keys
def _bits(a: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", a))[0]


def bound_key(d: float, sb: int) -> int:
    """cell_bound_key(d, 0, 0, SB): with two gaps zero the sum is one product, rounded the same with or without contraction"""
    return (_bits(bound_a(d, 0.0, 0.0)) >> sb) << sb


def near_window(tau: int, sb: int, ulps: int) -> int:
    if tau >= (NOLOC >> sb) << sb:
        return tau
    return max(tau + ulps, FLOOR) | ((1 << sb) - 1)


def stop_ring(keys, rings, g, sb, ulps, r_max=RMAX):
    """cell_walk's return value for one seed: keys = the packed keys of the candidates its walk counts (located ones), rings =
    the Chebyshev distance of each one's cell from the seed's.  The threshold behind ring r is the 64th smallest key of the
    rings up to r — the runs the walk skips inside a ring hold nothing below it, if their bounds are bounds — and the walk
    stops in front of the first ring whose bound lies beyond that threshold's window.  0 = the rings ran out.
    -> (stop ring, the last ring it offered)"""
    keys = np.asarray(keys, dtype=np.uint64)
    o = np.argsort(keys, kind="stable")
    ks, rs = keys[o], np.asarray(rings)[o]
    h = 2.0 / g

    def tau_hi(r):
        at = np.nonzero(np.cumsum(rs <= r) == 64)[0]
        return near_window(int(ks[at[0]]) if at.size else EMPTY, sb, ulps)

    if bound_key(h, sb) > tau_hi(1):
        return 2, 1
    if r_max < 2 or g <= 2:
        return 0, 1
    r = 3
    while True:
        if bound_key((r - 1) * h, sb) > tau_hi(r - 1):
            return r, r - 1
        if r > r_max or r >= g:
            return 0, r - 1
        r += 1
