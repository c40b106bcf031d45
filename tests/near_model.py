"""A plain model of pm_nearest_workers written from the reference: the candidate filter of try_form_new_groups
(node_groups/mod.rs:492-497, :511-515), its seed rule (:526-530), and sort_nodes_by_proximity (:234-255) — a stable sort of
the candidates in index order by the oracle's calculate_distance, unlocated nodes at f64::MAX, no sort at all from an
unlocated origin.  Compatibility comes in as the oracle's compat masks.  Nothing here looks at the kernels.

Also the generator of "separated" coordinates: from every origin it names, any two distances are bit-equal in the oracle or
more than 1e-9 apart relatively, so the order is the same in any arithmetic that is good to 1e-10."""
import numpy as np

from oracle import oracle_ffi as orc
from protocol_amd import engine as E

import spread_model as SM

NONE = 0xFFFFFFFF
F64_MAX = float(np.finfo(np.float64).max)
SEP = 1e-9
TOL = SM.TOL


def in_pool(pool, flags, group_of):
    f = np.asarray(flags).astype(np.uint32)
    ok = ((f & E.W_HEALTHY) != 0) & ((f & E.W_HAS_P2P) != 0)
    if pool == E.NEAR_IDLE:
        ok &= np.asarray(group_of) < 0
    return ok


def candidate_list(origin, config, pool, compat, flags, group_of):
    """workers of the pool that meet the configuration, the origin excluded, in index order"""
    ok = in_pool(pool, flags, group_of) & (((np.asarray(compat, dtype=np.uint64) >> np.uint64(config)) & np.uint64(1)) != 0)
    return [int(w) for w in np.flatnonzero(ok) if int(w) != origin]


def seed(config, compat, flags, group_of):
    """compatible_nodes.iter().find(|n| n.location.is_some()).or(compatible_nodes.first()) over the IDLE pool"""
    cand = candidate_list(NONE, config, E.NEAR_IDLE, compat, flags, group_of)
    for w in cand:
        if int(flags[w]) & E.W_HAS_LOC:
            return w
    return cand[0] if cand else NONE


def distances(origin, ws, flags, lat, lon):
    """the sort key of every worker of ws from the origin: the oracle's distance, F64_MAX for an unlocated one"""
    ws = np.asarray(ws, dtype=np.int64)
    d = np.full(len(ws), F64_MAX)
    if len(ws) and (int(flags[origin]) & E.W_HAS_LOC):
        loc = (np.asarray(flags)[ws].astype(np.uint32) & E.W_HAS_LOC) != 0
        la, lo = np.asarray(lat, dtype=np.float64)[ws[loc]], np.asarray(lon, dtype=np.float64)[ws[loc]]
        d[loc] = orc.distance_column(float(lat[origin]), float(lon[origin]), np.ascontiguousarray(la), np.ascontiguousarray(lo))
    return d


def nearest(origin, config, pool, k, compat, flags, group_of, lat, lon) -> dict:
    """one query: the fields of pm_near_row, the k slots of workers / km, and the whole sorted list with its keys"""
    if origin == E.NEAR_SEED:
        origin = seed(config, compat, flags, group_of)
    if origin == NONE:
        return dict(origin=NONE, n=0, candidates=0, located=0, workers=[NONE] * k, km=[F64_MAX] * k, order=[], key=[])
    cand = candidate_list(origin, config, pool, compat, flags, group_of)
    d = distances(origin, cand, flags, lat, lon)
    if int(flags[origin]) & E.W_HAS_LOC:
        idx = sorted(range(len(cand)), key=lambda i: d[i])   # (stable, as slice::sort_by)
    else:
        idx = list(range(len(cand)))
    order, key = [cand[i] for i in idx], [float(d[i]) for i in idx]
    n = min(k, len(cand))
    return dict(origin=origin, n=n, candidates=len(cand),
                located=sum(1 for w in cand if int(flags[w]) & E.W_HAS_LOC),
                workers=order[:n] + [NONE] * (k - n), km=key[:n] + [F64_MAX] * (k - n), order=order, key=key)


def close(a, b, tol=TOL):
    return a == b or abs(a - b) <= tol * max(abs(a), abs(b))


def check_query(got_row, got_w, got_km, want, exact, tag=""):
    """one query's output against the model's.  exact: no position may differ.  Otherwise a position may hold another
    worker than the model's only where the oracle keys of the two agree within TOL, and it must be a candidate that is
    returned nowhere else; km within TOL of the oracle's; nothing left out is nearer than the last one returned."""
    row = tuple(int(got_row[f]) for f in ("origin", "n", "candidates", "located"))
    assert row == (want["origin"], want["n"], want["candidates"], want["located"]), (tag, row, want["origin"], want["n"],
                                                                                      want["candidates"], want["located"])
    n, k = want["n"], len(want["workers"])
    got_w = [int(x) for x in got_w]
    assert len(got_w) == k and got_w[n:] == [NONE] * (k - n), (tag, "tail", got_w[n:])
    if got_km is not None:
        assert all(float(x) == F64_MAX for x in got_km[n:]), (tag, "km tail")
    if exact:
        assert got_w == want["workers"], (tag, [(i, a, b) for i, (a, b) in enumerate(zip(got_w, want["workers"])) if a != b][:5])
    key_of = dict(zip(want["order"], want["key"]))
    assert len(set(got_w[:n])) == n, (tag, "a worker twice")
    for i in range(n):
        w = got_w[i]
        assert w in key_of, (tag, i, w, "not a candidate")
        assert close(key_of[w], want["key"][i]), (tag, i, w, key_of[w], want["workers"][i], want["key"][i])
        if got_km is not None:
            assert close(float(got_km[i]), key_of[w]), (tag, i, w, float(got_km[i]), key_of[w])
    if n and n < len(want["order"]):
        last = key_of[got_w[n - 1]]
        ret = set(got_w[:n])
        rest = min(key_of[w] for w in want["order"] if w not in ret)
        assert rest >= last * (1.0 - TOL), (tag, "a nearer candidate was left out", rest, last)


# ---- separated coordinates

def is_separated(origins, lat, lon, located=None):
    """from every origin: sorted oracle distances to all (located) rows are pairwise bit-equal or > SEP apart, relatively"""
    lat, lon = np.ascontiguousarray(lat, dtype=np.float64), np.ascontiguousarray(lon, dtype=np.float64)
    sel = np.arange(len(lat)) if located is None else np.flatnonzero(located)
    for o in origins:
        d = np.sort(orc.distance_column(float(lat[o]), float(lon[o]), np.ascontiguousarray(lat[sel]), np.ascontiguousarray(lon[sel])))
        gap = d[1:] - d[:-1]
        if not np.all((gap == 0.0) | (gap > SEP * d[1:])):
            return False
        if d.size and d[-1] > SM.KM_AT_A_0_999:
            return False
    return True


def separated_coordinates(rng, n, origins=None, twins=0, mirrors=0, tries=50):
    """n coordinates on a grid of 2^-12 degrees (differences of two of them are exact) such that is_separated holds from
    every row of `origins` (default: every row).  `twins` rows repeat an earlier row bit for bit; `mirrors` pairs of rows sit
    at the latitude of origins[0], the same longitude offset either side of it: the two kinds of exact ties."""
    grid = 4096.0
    draw = lambda m: (np.round(rng.uniform(-50.0, 60.0, m) * grid) / grid, np.round(rng.uniform(-100.0, 50.0, m) * grid) / grid)
    lat, lon = draw(n)
    origins = list(range(n)) if origins is None else [int(o) for o in origins]
    free = np.ones(n, dtype=bool)        # rows the repair loop may redraw
    free[origins[:1]] = False
    at = n - 1
    for _ in range(mirrors):
        o = origins[0]
        off = np.round(rng.uniform(1.0, 40.0) * grid) / grid
        for s in (1.0, -1.0):
            while at == origins[0]:
                at -= 1
            lat[at], lon[at], free[at] = lat[o], lon[o] + s * off, False
            at -= 1
    twin_rows = []
    for _ in range(twins):
        while at == origins[0]:
            at -= 1
        twin_rows.append(at)
        free[at] = False
        at -= 1
    assert at >= 0
    for _ in range(tries):
        src = np.flatnonzero(free)
        for t in twin_rows:
            s = int(src[rng.integers(0, len(src))])
            lat[t], lon[t] = lat[s], lon[s]
        bad = set()
        for o in origins:
            d = orc.distance_column(float(lat[o]), float(lon[o]), np.ascontiguousarray(lat), np.ascontiguousarray(lon))
            order = np.argsort(d, kind="stable")
            ds = d[order]
            gap = ds[1:] - ds[:-1]
            for i in np.flatnonzero(~((gap == 0.0) | (gap > SEP * ds[1:])) | (ds[1:] > SM.KM_AT_A_0_999)):
                a, b = int(order[i]), int(order[i + 1])
                bad.add(b if free[b] else a)
        bad = [w for w in bad if free[w]]
        if not bad:
            break
        lat[bad], lon[bad] = draw(len(bad))
    assert is_separated(origins, lat, lon), "the generator could not separate the distances"
    return lat, lon
