"""The first batch of a formation on the batch pipeline — eligible list, candidate list, seeds, spatial index, neighbour rows —
restated in numpy, and the swarm families tests/test_first_batch_model.py (CPU) and tests/test_gpu_first_batch.py (the kernels,
through pm_debug_first_batch_arm) hold it to.

References: the lists from the swarm's columns and the oracle's compatibility masks (node_groups/mod.rs:492-519 and the rules of
carve_prep_place_kernel / prop_limit_scan as their comments state them); the index from the snapshot's own unit vectors
(cell_walk_model.cell_index); a row from the SET of keys its path counts, through near_row_cases.Reference.  A key is the
device's own (Engine.debug_candidate_keys, held to a high-precision Haversine by tests/test_gpu_distance_key.py) or, for the
CPU's look at the families, the chord term in numpy.  Everything is compared as whole arrays of integers."""
from __future__ import annotations

import os
import re
from dataclasses import dataclass, field

import numpy as np

import cell_walk_model as M
import near_row_cases as N
from oracle import oracle_ffi as orc
from protocol_amd.swarm import ST_HEALTHY, ST_UNHEALTHY, make_swarm

U = np.uint64
_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "protocol_amd", "csrc")


def _const(name, file="pm_device.h"):
    """a constant of the sources, from its definition alone: `static constexpr uint32_t NAME = 123;` or `#define NAME 123u`"""
    src = open(os.path.join(_CSRC, file)).read()
    found = re.findall(r"^\s*(?:static constexpr \w+ %s = |#define %s )(\d+)u?\b" % (name, name), src, flags=re.M)
    assert len(found) == 1, (name, found)
    return int(found[0])


PROP_RESERVE, PROP_KMAX, PROP_MAX_SEEDS = _const("PM_PROP_RESERVE"), _const("PM_PROP_KMAX"), _const("PM_PROP_MAX_SEEDS")
CARVE_SLOTS, CARVE_BIG_SLOTS = _const("PM_CARVE_SLOTS"), _const("PM_CARVE_BIG_SLOTS")
CELL_MIN_N, CELL_BIG_N, CELL_G_MAX, CELL_RMAX = (_const("PM_CELL_MIN_N"), _const("PM_CELL_BIG_N"), _const("PM_CELL_G_MAX"),
                                                 _const("PM_CELL_RMAX"))
CAP_DIV, CAP_DIV_BIG, CAP_DIV_WALK = (_const("PM_PROP_CAP_DIV", "pm_propose.inc"), _const("PM_PROP_CAP_DIV_BIG", "pm_propose.inc"),
                                      _const("PM_PROP_CAP_DIV_WALK", "pm_propose.inc"))
CELL_BUF, PROP_TILE = _const("CELL_BUF", "pm_propose.inc"), _const("PROP_TILE", "pm_propose.inc")
assert M.RMAX == CELL_RMAX and N.NOLOC == M.NOLOC


# ------------------------------------------------------------------------------------------------------------------ swarms
def swarm(lat, lon, has_loc, configs, gpu8=None, eligible=None, seed=7):
    """W workers with every spec present, Healthy with a p2p id unless `eligible` says otherwise (those rows are Unhealthy),
    gpu_count 8 where gpu8 else 1 (what the two requirement strings of CFG_PAIR select), one task per configuration"""
    W, n = len(lat), len(configs)
    sw = make_swarm(seed, 2 * n, W)
    for k in ("has_specs", "has_gpu", "gpu_count_some", "gpu_mem_some", "gpu_model_some", "has_cpu", "cpu_cores_some", "ram_some",
              "storage_some", "has_p2p"):
        getattr(sw, k)[:] = True
    sw.status[:] = ST_HEALTHY
    if eligible is not None:
        sw.status[~np.asarray(eligible)] = ST_UNHEALTHY
    sw.gpu_count[:] = 1 if gpu8 is None else np.where(gpu8, 8, 1)
    sw.has_loc[:] = has_loc
    sw.lat[:] = lat
    sw.lon[:] = lon
    sw.configs = list(configs)
    sw.topo[:] = -2
    sw.topo[:, 0] = np.arange(sw.T) % n
    sw.n_topo[:] = 1
    sw.restricted[:] = True
    return sw


CFG_ONE = (("one", 2, 8, None),)
CFG_COUNT8 = (("eights", 2, 8, "gpu:count=8"),)
CFG_PAIR = (("eights", 2, 8, "gpu:count=8"), ("ones", 2, 8, "gpu:count=1"))


# ------------------------------------------------------------------------------------------------- lists, seeds: reference
@dataclass
class Lists:
    order: np.ndarray          # eligible rows in input order
    compat: np.ndarray         # the oracle's mask per eligible position
    loc: np.ndarray            # bool per position
    avail: list                # configurations in carve order
    ci: int                    # position in `avail` of the configuration the first preparation picks (len(avail): none)
    pos: np.ndarray            # slot -> position
    slot_loc: np.ndarray       # bool per slot
    prop_k: int
    index_g: int               # grid of the carve's index (0 = none)
    batch_g: int               # grid the batch's proposals walk (0 = they sweep)
    limit: int
    seed_slots: np.ndarray
    seed_map: np.ndarray       # u64 per bitmap word below the limit
    seed_prefix: np.ndarray
    max_size: int = 0

    @property
    def n_list(self):
        return len(self.pos)

    @property
    def n_seeds(self):
        return len(self.seed_slots)

    @property
    def slot_wid(self):
        return self.order[self.pos]


def bitmap(b):
    """bool[n] -> u64[ceil(n / 64)], bit i of word j = b[64 j + i]"""
    b = np.asarray(b, dtype=bool)
    pad = np.zeros((len(b) + 63) // 64 * 64, dtype=np.uint8)
    pad[:len(b)] = b
    return np.packbits(pad.reshape(-1, 8), axis=1, bitorder="little").reshape(-1).view("<u8").copy()


def cell_g_for(n):
    return CELL_G_MAX if n >= CELL_BIG_N else CELL_G_MAX // 2 if n >= CELL_MIN_N else 0


def lists(sw, prune_mode: int, walk_cap_div: int = 0) -> Lists:
    assert prune_mode in (0, 2, 3), "mode 1 weighs the list against the index: not restated here"
    nodes, cfgs, _tasks, enabled = orc.from_swarm(sw)
    masks = orc.compat_masks(nodes, cfgs)
    order = np.nonzero((sw.status == ST_HEALTHY) & sw.has_p2p)[0]                 # mod.rs:492-497 (no groups yet)
    code, corder = orc.sort_configs(cfgs)
    assert code == 0
    avail = [int(c) for c in corder if enabled[c]]
    n = len(order)
    compat, loc = masks[order], np.asarray(sw.has_loc)[order]
    ci, pos = len(avail), np.zeros(0, dtype=np.int64)
    for k, c in enumerate(avail):                                                  # mod.rs:505-519
        mn = sw.configs[c][1]
        if n < mn:
            continue
        cand = np.nonzero((compat >> U(c)) & U(1))[0]
        if len(cand) < mn or len(cand) == 0:
            continue
        ci, pos = k, cand
        break
    forced = prune_mode >= 2
    index_g = cell_g_for(CELL_MIN_N if forced and 64 <= n < CELL_MIN_N else n) if forced else 0   # cell_count_kernel
    n_list = len(pos)
    slot_loc = loc[pos]
    prop_k = limit = batch_g = 0
    seed_slots = np.zeros(0, dtype=np.int64)
    seed_map, seed_prefix = np.zeros(0, dtype=U), np.zeros(0, dtype=np.uint32)
    mx = sw.configs[avail[ci]][2] if ci < len(avail) else 0
    if ci < len(avail) and n_list <= CARVE_BIG_SLOTS and mx - 1 < PROP_KMAX:      # carve_prep_place_kernel: `props`
        batch_g = index_g
        prop_k = min(mx - 1 + PROP_RESERVE, PROP_KMAX)
        div = (walk_cap_div or CAP_DIV_WALK) if batch_g else CAP_DIV_BIG if n_list > CARVE_SLOTS else CAP_DIV   # prop_limit_scan
        cap = min(max(n_list // div, 512), PROP_MAX_SEEDS)
        words = bitmap(slot_loc)                                                   # (every slot of a fresh list is alive)
        cnt = np.array([bin(int(w)).count("1") for w in words], dtype=np.int64)
        cum = np.cumsum(cnt)
        over = np.nonzero(cum >= cap)[0]
        last = int(over[0]) if over.size else len(words) - 1
        limit = min((last + 1) * 64, n_list) if over.size else n_list
        seed_slots = np.nonzero(slot_loc[:limit])[0]
        assert len(seed_slots) == (int(cum[last]) if len(words) else 0)
        seed_map = words[:last + 1].copy()
        seed_prefix = (cum - cnt)[:last + 1].astype(np.uint32)
    return Lists(order, compat, loc, avail, ci, pos, slot_loc, prop_k, index_g, batch_g, limit, seed_slots, seed_map, seed_prefix, mx)


def seam_offsets(L: Lists):
    """carve_prep_place_kernel, per 64-position word of the eligible list: (off & 63 of the word's first slot, whether the word's
    located bits reach into a second word of the slot loc bitmap — the second atomicOr)"""
    n = len(L.order)
    is_c = np.zeros(n, dtype=bool)
    is_c[L.pos] = True
    out, off = [], 0
    for j in range(0, n, 64):
        c = is_c[j:j + 64]
        locm = L.loc[j:j + 64][c]
        sh = off & 63
        spill = bool(sh and locm[64 - sh:].any())
        if c.any():
            out.append((sh, spill, bool(locm.any())))
        off += int(c.sum())
    return out


# --------------------------------------------------------------------------------------------------------------- rows: sets
def geometry(n_list):
    return N.GEOMETRIES["big" if n_list > CARVE_SLOTS else "small"]


def counted_sweep(L: Lists, seeds):
    """tile_keys / list_sweep_solo (FORM): alive slots t != s, without located t < s -> bool[len(seeds), n_list]"""
    t = np.arange(L.n_list)[None, :]
    s = np.asarray(seeds)[:, None]
    return (t != s) & ~(L.slot_loc[None, :] & (t < s))


def counted_walk(L: Lists, seeds, cc_site):
    """cell_drain: located slots t != s, without the slots at the seed's own shared site in front of it"""
    t = np.arange(L.n_list)[None, :]
    s = np.asarray(seeds)[:, None]
    ssite = np.asarray(cc_site)[np.asarray(seeds)][:, None]
    shared = (ssite & 0x80000000) != 0
    return L.slot_loc[None, :] & (t != s) & ~(shared & (np.asarray(cc_site)[None, :] == ssite) & (t < s))


def pack(L: Lists, unpacked, counted, cc_site, seeds):
    """unpacked key bits u64[len(seeds), n_list] of located pairs at different sites -> packed keys: 0 at the seed's own site,
    PM_KEY_NOLOC without a location, EMPTY where the slot does not count (near_row_cases._pack's layout)"""
    g = geometry(L.n_list)
    v = np.asarray(unpacked, dtype=U).copy()
    same = np.asarray(cc_site)[None, :] == np.asarray(cc_site)[np.asarray(seeds)][:, None]
    v[same & L.slot_loc[None, :]] = U(0)
    v[:, ~L.slot_loc] = U(N.NOLOC)
    return N._pack(g, v >> U(g.sb), np.broadcast_to(np.arange(L.n_list, dtype=U)[None, :], v.shape), ~counted)


def expected_rows(L: Lists, keys, cc_site):
    """packed keys (EMPTY = not counted) of some seeds -> what carve_propose_kernel stores for each: u64[n, 96]"""
    g = geometry(L.n_list)
    sites = np.zeros(1 << g.sb, dtype=np.uint32)
    sites[:L.n_list] = cc_site
    word, mine, _ = N.Reference(keys, sites, g).flags()
    K = L.prop_k
    meta, ent = word[:, K - 1].astype(U), mine[:, K - 1, :63]
    row = np.zeros((len(keys), 96), dtype=U)
    row[:, 0] = meta
    row[:, 1:64] = ent
    half = np.zeros((len(keys), 64), dtype=np.uint32)
    half[:, 0] = meta.astype(np.uint32)
    half[:, 1:] = (ent & U(g.mask)).astype(np.uint32)
    row[:, 64:] = half.view("<u8")
    return row


def numpy_keys(ux, uy, uz, L: Lists, seeds):
    """the chord term of every (seed, slot) pair in numpy -> its bits (the CPU's stand-in for the device's key)"""
    px, py, pz = ux[L.pos], uy[L.pos], uz[L.pos]
    s = np.asarray(seeds)
    a = 0.25 * ((px[None, :] - px[s][:, None]) ** 2 + (py[None, :] - py[s][:, None]) ** 2 + (pz[None, :] - pz[s][:, None]) ** 2)
    return a.view(U)


# --------------------------------------------------------------------------------------------------------- the walk's model
@dataclass
class Walks:
    stop: np.ndarray           # per seed: the ring the walk stops in front of, 0 = the rings run out (the seed falls back)
    last: np.ndarray           # the last ring it offers
    near: np.ndarray           # list candidates in rings 0 and 1 (the seed among them): what the walk's first pass packs
    cell0: np.ndarray          # entries of the seed's own cell (one run)
    clipped: np.ndarray        # the seed's cell is the first or the last of an axis
    strangers: np.ndarray      # indexed positions that are not in the list, inside the rings the walk offers


def walks(L: Lists, ux, uy, uz, cc_site, keys_of, chunk=256) -> Walks:
    """the model walk of every seed.  ux, uy, uz: per position; keys_of(seeds) -> unpacked key bits u64[len(seeds), n_list]"""
    g = L.batch_g
    gm = geometry(L.n_list)
    cx, cy, cz = (M.cell_coord(v, g) for v in (ux, uy, uz))
    px, py, pz = cx[L.pos], cy[L.pos], cz[L.pos]
    in_list = np.zeros(len(L.order), dtype=bool)
    in_list[L.pos] = True
    stranger = L.loc & ~in_list
    sx, sy, sz = cx[stranger], cy[stranger], cz[stranger]
    out = {k: [] for k in ("stop", "last", "near", "cell0", "clipped", "strangers")}
    for c0 in range(0, L.n_seeds, chunk):
        seeds = L.seed_slots[c0:c0 + chunk]
        counted = counted_walk(L, seeds, cc_site)
        keys = pack(L, keys_of(seeds), counted, cc_site, seeds)
        for i, s in enumerate(seeds):
            ring = np.maximum(np.maximum(np.abs(px - px[s]), np.abs(py - py[s])), np.abs(pz - pz[s]))
            m = counted[i]
            stop, last = M.stop_ring(keys[i][m], ring[m], g, gm.sb, gm.ulps, CELL_RMAX)
            out["stop"].append(stop)
            out["last"].append(last)
            out["near"].append(int((L.slot_loc & (ring <= 1)).sum()))
            out["cell0"].append(int((L.loc & (cx == px[s]) & (cy == py[s]) & (cz == pz[s])).sum()))
            out["clipped"].append(bool(min(px[s], py[s], pz[s]) == 0 or max(px[s], py[s], pz[s]) == g - 1))
            sr = np.maximum(np.maximum(np.abs(sx - px[s]), np.abs(sy - py[s])), np.abs(sz - pz[s]))
            out["strangers"].append(int((sr <= last).sum()))
    return Walks(**{k: np.array(v) for k, v in out.items()})


SPARSE_ABOVE = 6_000_000     # seeds x slots from which the model walk asks only for the keys of the rings it looks at


def numpy_pair_keys(ux, uy, uz, L: Lists):
    px, py, pz = ux[L.pos], uy[L.pos], uz[L.pos]

    def keys_of(s, t):
        a = 0.25 * ((px[t] - px[s]) ** 2 + (py[t] - py[s]) ** 2 + (pz[t] - pz[s]) ** 2)
        return a.view(U)
    return keys_of


def walk_stops(L: Lists, ux, uy, uz, cc_site, pair_keys, chunk=128):
    """cell_walk's return value for every seed, from the keys of the rings it looks at alone: what stops a walk in front of
    ring r is the threshold behind ring r - 1, so the slots within R rings decide every stop up to R + 1; the seeds that are
    still open behind R = 2 are looked at again within 5 rings, then within all PM_CELL_RMAX.
    pair_keys(seed slots, slots) -> unpacked key bits per pair"""
    g, gm = L.batch_g, geometry(L.n_list)
    cx, cy, cz = (M.cell_coord(v, g)[L.pos].astype(np.int32) for v in (ux, uy, uz))
    site = np.asarray(cc_site)
    stop = np.full(L.n_seeds, -1, dtype=np.int64)
    slots_u = np.arange(L.n_list, dtype=U)
    for R in (2, 5, CELL_RMAX):
        todo = np.nonzero(stop < 0)[0]
        for c0 in range(0, len(todo), chunk):
            idx = todo[c0:c0 + chunk]
            seeds = L.seed_slots[idx]
            ring = np.maximum(np.maximum(np.abs(cx[None, :] - cx[seeds][:, None]), np.abs(cy[None, :] - cy[seeds][:, None])),
                              np.abs(cz[None, :] - cz[seeds][:, None]))
            m = counted_walk(L, seeds, site) & (ring <= R)
            i, t = np.nonzero(m)
            v = np.asarray(pair_keys(seeds[i], t), dtype=U).copy()
            v[site[t] == site[seeds[i]]] = U(0)
            keys = ((v >> U(gm.sb)) << U(gm.sb)) | slots_u[t]
            ends = np.searchsorted(i, np.arange(len(idx) + 1))
            for k in range(len(idx)):
                a, b = ends[k], ends[k + 1]
                st, _ = M.stop_ring(keys[a:b], ring[k, t[a:b]], g, gm.sb, gm.ulps, CELL_RMAX)
                if R == CELL_RMAX or 0 < st <= R + 1:
                    stop[idx[k]] = st
    return stop


# ---------------------------------------------------------------------------------------------------------------- families
@dataclass
class Family:
    name: str
    sw: object
    modes: tuple                       # prune modes the GPU test forms it in
    special: object = None             # (Lists) -> seed numbers the family was built for
    expect: dict = field(default_factory=dict)   # what test_first_batch_model.py asserts it reaches
    n_drawn: int = 32


def _scatter(rng, n, lat0=25.0, lat1=60.0, lon0=-125.0, lon1=40.0):
    return np.round(lat0 + (lat1 - lat0) * rng.random(n), 4), np.round(lon0 + (lon1 - lon0) * rng.random(n), 4)


SEAM_GAPS = {1: 63, 127: 2}            # non-candidates behind the k-th candidate: the words' first slots fall at off & 63 = 1, then 63


def _with_gaps(n_cand, gaps):
    """candidate flags of an eligible list with gaps[k] non-candidates behind its k-th candidate"""
    out = []
    for k in range(1, n_cand + 1):
        out.append(True)
        out += [False] * gaps.get(k, 0)
    return np.array(out, dtype=bool)


def lengths():
    """n_list at the edges of PROP_TILE, of the bitmaps' last word and of tile_fetch's clamp; located shares all / 70 % / none;
    from 192 candidates on, the list's 64-position words start at off & 63 = 0, 1 and 63 (SEAM_GAPS)"""
    out = []
    for n_list in (1, 63, 64, 65, 511, 512, 513, 1025):
        for share in (1.0, 0.7, 0.0):
            rng = np.random.default_rng(1000 + n_list + int(share * 10))
            cand = _with_gaps(n_list, SEAM_GAPS)
            W = len(cand)
            lat, lon = _scatter(rng, W)
            loc = rng.random(W) < share if 0.0 < share < 1.0 else np.full(W, share == 1.0)
            if share == 0.7 and n_list > 1:      # a location-less candidate in front of every seed but the first, a located last slot
                ci = np.nonzero(cand)[0]
                loc[ci[0]], loc[ci[1]], loc[ci[-1]] = True, False, True
            cfgs = CFG_COUNT8 if n_list > 1 else (("solo", 1, 1, "gpu:count=8"),)
            out.append(Family(f"len-{n_list}-loc{int(share * 100)}", swarm(lat, lon, loc, cfgs, gpu8=cand), (0, 3),
                              expect={"n_list": n_list, "seams": n_list >= 192 and share > 0}))
    return out


def caps():
    """the seed cap of a swept list (512) one below, met and one above, well above, and somewhere inside a 70 % word"""
    out = []
    for n_loc, extra in ((511, 0), (512, 0), (513, 0), (600, 0), (600, 300)):
        rng = np.random.default_rng(2000 + n_loc + extra)
        W = n_loc + extra
        lat, lon = _scatter(rng, W)
        loc = np.ones(W, dtype=bool)
        if extra:
            loc[rng.permutation(W)[:extra]] = False
        out.append(Family(f"cap-{n_loc}-of-{W}", swarm(lat, lon, loc, CFG_ONE), (0, 3),
                          expect={"n_seeds": min(n_loc, 512) if not extra else None, "capped": n_loc > 512}))
    return out


def _continent(rng, n):
    """a third in eight cities a few dozen km wide (walks that stop in front of ring 2), a third over a country (ring 3), the
    rest over a third of the globe (later rings)"""
    k = n // 3
    c_lat, c_lon = _scatter(rng, 8, 30.0, 55.0, -120.0, 30.0)
    city = rng.integers(0, 8, k)
    lat = [c_lat[city] + rng.normal(0, 0.2, k), 35.0 + 10.0 * rng.random(k), -40.0 + 110.0 * rng.random(n - 2 * k)]
    lon = [c_lon[city] + rng.normal(0, 0.2, k), 70.0 + 14.0 * rng.random(k), -170.0 + 200.0 * rng.random(n - 2 * k)]
    p = rng.permutation(n)
    return np.round(np.concatenate(lat), 4)[p], np.round(np.concatenate(lon), 4)[p]


def continent():
    rng = np.random.default_rng(3000)
    lat, lon = _continent(rng, 3000)
    loc = np.ones(3000, dtype=bool)
    return [Family("continent", swarm(lat, lon, loc, CFG_ONE), (0, 2, 3), expect={"g": 32, "stops": (2, 3, 4)}),
            # (a configuration of up to 64 has no proposals: max_group_size - 1 < PM_PROP_KMAX fails, the validator sweeps)
            Family("continent-64", swarm(lat, lon, loc, (("wide", 2, 64, None),)), (0, 2, 3), expect={"no_props": True})]


def walked_cap():
    """a walked list's cap is n_list / 10: 5,300 candidates, 530 seeds and what the cap's word holds beyond them"""
    rng = np.random.default_rng(3100)
    lat, lon = _continent(rng, 5300)
    return [Family("walked-cap", swarm(lat, lon, np.ones(5300, dtype=bool), CFG_ONE), (2,), expect={"g": 32, "cap": 530})]


def two_configs():
    """disjoint requirements interleaved in input order: the index holds both populations, the list one"""
    rng = np.random.default_rng(3200)
    n = 1600
    lat, lon = _continent(rng, n)
    loc = rng.random(n) < 0.9
    eligible = rng.random(n) < 0.95
    return [Family("two-configs", swarm(lat, lon, loc, CFG_PAIR, gpu8=rng.random(n) < 0.5, eligible=eligible), (0, 2, 3),
                   expect={"g": 32, "strangers": True})]


AXIS_HALVES = {"north-east": ((90.0, 0.0), (0.0, 0.0), (0.0, 90.0)), "south-west": ((-90.0, 0.0), (0.0, 180.0), (0.0, -90.0))}


def grid_edges():
    """crowds of 130 around a pole and two equatorial axis points (two halves of the globe: no antipodal pairs, which are outside
    the reference's domain), the first ten of each exactly on the point: unit coordinates of exactly +-1 and 0, seeds in the first
    or the last cell of an axis, runs clipped at the grid's faces"""
    out = []
    for hi, (half, points) in enumerate(AXIS_HALVES.items()):
        rng = np.random.default_rng(3300 + hi)
        lat, lon = [], []
        for (la, lo) in points:
            k = 130
            dla, dlo = rng.normal(0, 1.5, k), rng.normal(0, 1.5, k)
            dla[:10] = dlo[:10] = 0.0
            if abs(la) == 90.0:
                lat.append(la - np.sign(la) * np.abs(dla))
                lon.append(np.where(dla == 0.0, lo, rng.uniform(-179.0, 179.0, k)))
            else:
                lat.append(la + dla)
                lon.append(((lo + dlo + 180.0) % 360.0) - 180.0 if abs(lo) == 180.0 else lo + dlo)
        lat, lon = np.round(np.concatenate(lat), 4), np.round(np.concatenate(lon), 4)
        lon[(lon == -180.0)] = 180.0
        p = rng.permutation(len(lat))
        lat, lon = lat[p], lon[p]
        on = np.zeros(len(lat), dtype=bool)
        for (la, lo) in points:
            on |= (lat == la) & (lon == lo)
        assert on.sum() == 30

        def special(L, on=on):
            return np.nonzero(on[L.slot_wid[L.seed_slots]])[0]

        out.append(Family("grid-edges-" + half, swarm(lat, lon, np.ones(len(lat), dtype=bool), CFG_ONE), (0, 2, 3), special,
                          expect={"g": 32, "clipped": True}))
    return out


def city():
    """1,500 workers within a kilometre, two shared sites of 60 among them: more than CELL_BUF - 256 candidates in rings 0 - 1 (a
    drain in mid-run), a run of more than 256 entries, the sine form of the key, zero keys at the seed's own site"""
    rng = np.random.default_rng(3400)
    n = 1500
    lat = 48.8566 + rng.uniform(-0.004, 0.004, n)
    lon = 2.3522 + rng.uniform(-0.006, 0.006, n)
    p = rng.permutation(n)
    for k, (la, lo) in enumerate(((48.857, 2.352), (48.858, 2.354))):
        lat[p[60 * k:60 * (k + 1)]] = la
        lon[p[60 * k:60 * (k + 1)]] = lo
    lat, lon = np.round(lat, 6), np.round(lon, 6)

    def special(L):
        w = L.slot_wid[L.seed_slots]
        return np.nonzero(np.isin(w, p[:120]))[0]

    return [Family("city", swarm(lat, lon, np.ones(n, dtype=bool), CFG_ONE), (0, 2, 3), special,
                   expect={"g": 32, "drain": True, "long_run": True})]


def lonely():
    """(a) a crowd and five located workers more than PM_CELL_RMAX rings from it and from each other: their walks run out of
    rings; (b) a list with fewer than 64 located candidates among location-less ones: every seed falls back"""
    rng = np.random.default_rng(3500)
    lat, lon = _scatter(rng, 700, 40.0, 50.0, 0.0, 15.0)
    far = ((-75.0, -150.0), (-80.0, 100.0), (-60.0, 179.0), (-70.0, -60.0), (-85.0, 20.0))
    at = (0, 1, 130, 300, 511)            # (inside the first 512 located slots: the batch's seeds)
    for k, (la, lo) in zip(at, far):
        lat, lon = np.insert(lat, k, la), np.insert(lon, k, lo)
    n = len(lat)

    def special(L):
        return np.nonzero(np.isin(L.slot_wid[L.seed_slots], at))[0]

    a = Family("lonely-far", swarm(lat, lon, np.ones(n, dtype=bool), CFG_ONE), (0, 2, 3), special, expect={"g": 32, "run_outs": 5})
    lat2, lon2 = _scatter(rng, 300, 40.0, 50.0, 0.0, 15.0)
    loc2 = np.zeros(300, dtype=bool)
    loc2[rng.permutation(300)[:50]] = True
    b = Family("lonely-few", swarm(lat2, lon2, loc2, CFG_ONE), (0, 2, 3), expect={"g": 32, "run_outs": 50})
    return [a, b]


def wide():
    """n_list = 8192 and 8193: 13 and 18 slot bits, the other certificate band and window"""
    out = []
    for n in (8192, 8193):
        rng = np.random.default_rng(3600 + n)
        lat, lon = _continent(rng, n)
        loc = rng.random(n) < 0.9
        out.append(Family(f"wide-{n}", swarm(lat, lon, loc, CFG_ONE), (0, 3), expect={"sb": 13 if n == 8192 else 18}, n_drawn=16))
    return out


def big_grid():
    """the 64^3 grid: 40,000 eligible workers (PM_CELL_BIG_N), all located — three quarters in forty cities a cell or two wide,
    the rest over two continents.  A quarter of them are candidates of the one configuration (groups of up to 63, so that the
    oracle's carve of the swarm stays a matter of a second): a list of some 10,000 — 18 slot bits, a cap of n_list / 10
    either way — inside an index of 40,000, three entries in four strangers to the list"""
    rng = np.random.default_rng(3700)
    n = CELL_BIG_N
    k = 3 * n // 4
    c_lat, c_lon = _scatter(rng, 40, 28.0, 58.0, -120.0, 35.0)
    city = rng.integers(0, 40, k)
    r_lat, r_lon = _scatter(rng, n - k, 25.0, 60.0, -125.0, 40.0)
    lat = np.round(np.concatenate([c_lat[city] + rng.normal(0, 0.5, k), r_lat]), 4)
    lon = np.round(np.concatenate([c_lon[city] + rng.normal(0, 0.5, k), r_lon]), 4)
    p = rng.permutation(n)
    cfg = (("eights", 2, 63, "gpu:count=8"),)
    return [Family("grid-64", swarm(lat[p], lon[p], np.ones(n, dtype=bool), cfg, gpu8=rng.random(n) < 0.25), (0, 2, 3),
                   expect={"g": 64, "stops": (2, 3), "sb": 18}, n_drawn=16)]


FAMILIES = {"lengths": lengths, "caps": caps, "continent": continent, "walked_cap": walked_cap, "two_configs": two_configs,
            "grid_edges": grid_edges, "city": city, "lonely": lonely, "wide": wide, "big_grid": big_grid}
_made = {}


def family(group):
    """the members of a family, made once"""
    if group not in _made:
        _made[group] = FAMILIES[group]()
    return _made[group]


def all_members():
    return [(g, i) for g in FAMILIES for i in range(len(family(g)))]


def member_id(gi):
    return family(gi[0])[gi[1]].name


def sample(fam: Family, L: Lists):
    """seed numbers the brute-force comparison takes: the first, the last, the family's own, fam.n_drawn more; all of them where
    there are no more than 48"""
    ns = L.n_seeds
    if ns <= 48:
        return np.arange(ns)
    rng = np.random.default_rng(99)
    own = fam.special(L) if fam.special else np.zeros(0, dtype=np.int64)
    n_drawn = fam.n_drawn if fam.n_drawn < 32 else max(fam.n_drawn, 48)      # (at least 48 distinct ones, the large families aside)
    return np.unique(np.concatenate([[0, ns - 1], own, rng.choice(ns, n_drawn, replace=False)]).astype(np.int64))


# ------------------------------------------------------------------------------------- what a family exists for, by the model
def model_sites(sw):
    """the site word of every row as the engine interns it: equal (lat, lon) bit patterns <=> equal id; bit 31 = two or more
    located rows share it"""
    key = np.stack([np.asarray(sw.lat, dtype=np.float64).view(U), np.asarray(sw.lon, dtype=np.float64).view(U)], axis=1)
    _, ids = np.unique(key, axis=0, return_inverse=True)
    ids = ids.reshape(-1).astype(np.uint32)
    pop = np.bincount(ids[np.asarray(sw.has_loc)], minlength=int(ids.max()) + 1 if len(ids) else 0)
    return ids | np.where(pop[ids] >= 2, np.uint32(0x80000000), np.uint32(0))


def reaches(fam: Family):
    """assert that the family reaches what it was built for, by the references and the model walk alone (numpy's unit vectors
    and chord terms in place of the device's) -> {mode: Lists}"""
    sw, ex = fam.sw, fam.expect
    out = {}
    for mode in fam.modes:
        L = out[mode] = lists(sw, mode)
        assert L.ci < len(L.avail) and L.n_list > 0, "a list is prepared"
        if "n_list" in ex:
            assert L.n_list == ex["n_list"]
        if ex.get("seams"):
            seams = seam_offsets(L)
            assert {sh for sh, spill, _ in seams if spill} >= {1, 63} and any(sh == 0 and any_loc for sh, _, any_loc in seams), seams
        if ex.get("n_seeds") is not None:
            assert L.n_seeds == ex["n_seeds"]
        if "capped" in ex:
            assert (L.limit < L.n_list) == ex["capped"] or L.n_list == 512, (L.limit, L.n_list)
        if "sb" in ex:
            assert geometry(L.n_list).sb == ex["sb"]
        if ex.get("no_props"):
            assert L.prop_k == 0 and L.n_seeds == 0 and L.batch_g == 0
        if mode != 2 or not L.batch_g:
            continue
        assert L.index_g == ex["g"] == L.batch_g
        if "cap" in ex:
            assert L.n_list // CAP_DIV_WALK == ex["cap"] > 512 and ex["cap"] <= L.n_seeds < ex["cap"] + 64 and L.limit % 64 == 0
        ux, uy, uz = (np.asarray(v)[L.order] for v in M.unit(np.asarray(sw.lat), np.asarray(sw.lon)))
        site = model_sites(sw)[L.order][L.pos]
        if L.n_seeds * L.n_list > SPARSE_ABOVE:
            stop = walk_stops(L, ux, uy, uz, site, numpy_pair_keys(ux, uy, uz, L))
            assert set(ex["stops"]) <= set(stop.tolist()), np.unique(stop, return_counts=True)
            assert len(L.order) == CELL_BIG_N and L.n_list // CAP_DIV_WALK <= L.n_seeds and (stop == 0).sum() < L.n_seeds // 2
            continue
        w = walks(L, ux, uy, uz, site, lambda seeds: numpy_keys(ux, uy, uz, L, seeds))
        own = fam.special(L) if fam.special else np.arange(L.n_seeds)
        if "stops" in ex:
            assert set(ex["stops"]) <= set(w.stop.tolist()) and (w.stop >= 4).any(), np.unique(w.stop, return_counts=True)
        if ex.get("drain"):
            assert (w.near > CELL_BUF - 256).any() and (w.stop[w.near > CELL_BUF - 256] != 0).all()
        if ex.get("long_run"):
            assert (w.cell0 > 256).any()
        if ex.get("clipped"):
            assert len(own) >= 20 and w.clipped[own].all() and (w.stop[own] != 0).all(), (w.clipped[own], w.stop[own])
        if ex.get("strangers"):
            assert (w.strangers[w.stop != 0] > 0).any() and (~L.slot_loc).any()
        if "run_outs" in ex:
            assert int((w.stop == 0).sum()) == ex["run_outs"], np.unique(w.stop, return_counts=True)
            if fam.special:
                assert (w.stop[own] == 0).all() and len(own) == ex["run_outs"]
        else:
            assert (w.stop != 0).any()
    return out
