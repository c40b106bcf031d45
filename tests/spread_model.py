"""A plain numpy model of the group geography reports (pm_group_spread, pm_config_spread) and of pm_force_regroup's
selection, written from the reference: distances are the oracle's calculate_distance (node_groups/mod.rs:218-231), the ring
is the BTreeSet<String> order a worker's NEXT_P2P_ADDRESS follows (scheduler_impl.rs:115-116, mod.rs:424-434) given as
addr_rank, the regroup order is get_all_groups' ascending "{:x}" text of the id (mod.rs:1040).  Nothing here looks at the
kernels."""
import numpy as np

from oracle import oracle_ffi as orc
from protocol_amd import engine as E

NONE = 0xFFFFFFFF
EDGES_KM = (10.0, 100.0, 1000.0, 5000.0)


def ring_order(members, addr_rank=None):
    """members in BTreeSet<String> order: ascending address rank (the worker index without the column), ties by index"""
    key = (lambda w: (int(w), int(w))) if addr_rank is None else (lambda w: (int(addr_rank[w]), int(w)))
    return sorted((int(w) for w in members), key=key)


def pair_matrix(ws, lat, lon):
    """the oracle's distance of every ordered pair of the workers ws: D[i, j] = calculate_distance(ws[i], ws[j])"""
    la, lo = np.asarray(lat, dtype=np.float64)[ws], np.asarray(lon, dtype=np.float64)[ws]
    return np.stack([orc.distance_column(float(la[i]), float(lo[i]), la, lo) for i in range(len(ws))]) if len(ws) else \
        np.zeros((0, 0))


def group_spread(members, flags, lat, lon, addr_rank=None) -> dict:
    """one group: the fields of pm_group_spread_row, plus `hops` [(from, to, km)] in ring order and `pairs_at_max`"""
    f = np.asarray(flags).astype(np.uint32)
    ring = ring_order(members, addr_rank)
    loc = sorted(w for w in ring if f[w] & E.W_HAS_LOC)
    out = dict(located=len(loc), ring_hops=0, far_a=NONE, far_b=NONE, hop_from=NONE, diameter_km=0.0, ring_km=0.0,
               longest_hop_km=0.0, hops=[], pairs_at_max=[])
    if len(loc) >= 2:
        ws = np.array(loc, dtype=np.int64)
        D = pair_matrix(ws, lat, lon)
        iu = np.triu_indices(len(ws), 1)
        d = D[iu]
        mx = float(d.max())
        at = [(int(ws[i]), int(ws[j])) for i, j, v in zip(iu[0], iu[1], d) if v == mx]  # (ws ascends: lexicographic order)
        out.update(diameter_km=mx, far_a=at[0][0], far_b=at[0][1], pairs_at_max=at)
    n = len(ring)
    for i, w in enumerate(ring):
        nx = ring[(i + 1) % n]
        if nx != w and (f[w] & E.W_HAS_LOC) and (f[nx] & E.W_HAS_LOC):
            out["hops"].append((w, nx, orc.calculate_distance(float(lat[w]), float(lon[w]), float(lat[nx]), float(lon[nx]))))
    if out["hops"]:
        km = [h[2] for h in out["hops"]]
        out["ring_hops"] = len(km)
        out["ring_km"] = float(np.sum(np.array(km, dtype=np.float64)))
        out["longest_hop_km"] = max(km)
        out["hop_from"] = min(h[0] for h in out["hops"] if h[2] == out["longest_hop_km"])
    return out


def bucket(km: float) -> int:
    return sum(1 for e in EDGES_KM if km >= e)


def config_spread(rows, cfg_of_row, n_cfgs: int) -> np.ndarray:
    """pm_config_spread as an exact function of per-group rows (group_spread_dt records or the model's dicts)"""
    out = np.zeros(n_cfgs, dtype=E.config_spread_dt)
    for r, c in zip(rows, cfg_of_row):
        o = out[int(c)]
        o["groups"] += 1
        if int(r["located"]) >= 2:
            o["measured"] += 1
            o["hist"][bucket(float(r["diameter_km"]))] += 1
            o["max_diameter_km"] = max(float(o["max_diameter_km"]), float(r["diameter_km"]))
            o["sum_diameter_m"] += int(np.rint(np.float64(r["diameter_km"]) * 1000.0))
        if int(r["ring_hops"]) >= 1:
            o["max_hop_km"] = max(float(o["max_hop_km"]), float(r["longest_hop_km"]))
            o["sum_ring_m"] += int(np.rint(np.float64(r["ring_km"]) * 1000.0))
    return out


def id_text(group_id: int) -> str:
    return format(int(group_id), "x")


def regroup_selection(groups, rows, config: int, metric: int, threshold_km: float):
    """groups: [(id, config, members)] of the live groups, rows: their spread rows in the same order -> the groups the call
    dissolves, in the order it dissolves them (ascending "{:x}" text, compared as a string)"""
    sel = []
    for g, r in zip(groups, rows):
        if int(g[1]) != config:
            continue
        if metric == E.REGROUP_DIAMETER and not (int(r["located"]) >= 2 and float(r["diameter_km"]) >= threshold_km):
            continue
        if metric == E.REGROUP_LONGEST_HOP and not (int(r["ring_hops"]) >= 1 and float(r["longest_hop_km"]) >= threshold_km):
            continue
        sel.append(g)
    return sorted(sel, key=lambda g: id_text(g[0]))


def engine_groups(eng):
    """[(id, config, members in BTreeSet order)] of the live groups in slot order (pm_get_groups: compacts the list)"""
    _, groups, members = eng.get_groups()
    return [(int(g["id"]), int(g["config"]),
             members[int(g["member_begin"]):int(g["member_begin"]) + int(g["n_members"])].tolist()) for g in groups]


def device_a(lat1, lon1, lat2, lon2, src, fma, sin_band):
    """the device's Haversine term of one pair, operation by operation (hav_a in pm_validate.inc: the sine form, with the
    cosines of the latitude column); None where sin_band would call OCML's sin"""
    rad = 3.14159265358979323846 / 180.0
    s1 = sin_band(((lat2 - lat1) * rad) * 0.5, src)
    s2 = sin_band(((lon2 - lon1) * rad) * 0.5, src)
    if s1 is None or s2 is None:
        return None
    c = float(np.cos(np.float64(lat1 * rad))) * float(np.cos(np.float64(lat2 * rad)))
    return s1 * s1 + c * (s2 * s2)


def km_of_a(a):
    a = np.minimum(np.asarray(a, dtype=np.float64), 1.0)
    return 6371.0 * (2.0 * np.arctan2(np.sqrt(a), np.sqrt(1.0 - a)))


# ---- what the GPU tests allow between the device's rows and this model's (see tests/test_gpu_spread.py for the derivation)
TOL, TOL_RING = 1e-12, 1e-11
KM_AT_A_0_999 = 2.0 * 6371.0 * float(np.arcsin(np.sqrt(0.999)))  # a <= 0.999 <=> d <= this


def close(a, b, tol):
    return abs(a - b) <= tol * max(abs(a), abs(b))


def check_rows(got, want, lat, lon, exact=None, tag=""):
    """per-group rows against the model's; exact[k]: every maximal pair of group k ties exactly, so the indices must be the
    rule's"""
    assert len(got) == len(want), (tag, len(got), len(want))
    d = lambda a, b: orc.calculate_distance(float(lat[a]), float(lon[a]), float(lat[b]), float(lon[b]))
    for k, (g, w) in enumerate(zip(got, want)):
        t = f"{tag} group {k}"
        assert int(g["located"]) == w["located"] and int(g["ring_hops"]) == w["ring_hops"], (t, g, w)
        if w["diameter_km"] > KM_AT_A_0_999:   # (only a swarm that was not built for this test has such a pair: the
            continue                           # tolerance's derivation stops at a = 0.999, the counts above do not)
        assert close(float(g["diameter_km"]), w["diameter_km"], TOL), (t, g["diameter_km"], w["diameter_km"])
        assert close(float(g["longest_hop_km"]), w["longest_hop_km"], TOL), (t, g["longest_hop_km"], w["longest_hop_km"])
        assert close(float(g["ring_km"]), w["ring_km"], TOL_RING), (t, g["ring_km"], w["ring_km"])
        fa, fb, hf = int(g["far_a"]), int(g["far_b"]), int(g["hop_from"])
        if w["located"] < 2:
            assert (fa, fb) == (NONE, NONE) and float(g["diameter_km"]) == 0.0, t
        else:
            assert fa < fb and close(d(fa, fb), w["diameter_km"], TOL), (t, fa, fb)
            if exact is not None and exact[k]:
                assert (fa, fb) == (w["far_a"], w["far_b"]), (t, fa, fb, w["far_a"], w["far_b"])
        if w["ring_hops"] == 0:
            assert hf == NONE and float(g["ring_km"]) == 0.0 and float(g["longest_hop_km"]) == 0.0, t
        else:
            hop = {h[0]: h[2] for h in w["hops"]}
            assert hf in hop and close(hop[hf], w["longest_hop_km"], TOL), (t, hf)
            if exact is not None and exact[k]:
                assert hf == w["hop_from"], (t, hf, w["hop_from"])
