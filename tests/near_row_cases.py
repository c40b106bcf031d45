"""Key sets for neighbour rows and what a row of them has to be, for tests/test_near_row_cases.py (CPU) and
tests/test_gpu_row_certificates.py (the kernels).

The reference is a function of the SET of a wave's keys and the site table — no strides, no tracker, no insertion order:
the row is the 64 smallest keys, the window is near_window as its comment states it (protocol_amd/csrc/pm_propose.inc), the
tracker's answer is "the smallest unlisted key below the window's end that does not sit at site X", and the flags word is
every field of near_row_finish computed from the sorted keys, `tail_ok` over ALL unlisted keys (the tail_ok_brute of
tests/test_near_row_model.py).  numpy, vectorised over the waves of a call.

Every band expression of near_row_finish multiplies by a power of two (4 band, band) and adds 1e-300.  No family here has a
located value below 1e-296, so no such product is subnormal: each is exact, the sum is rounded once with or without FMA
contraction, and numpy's float64 gives the device's bits."""
from __future__ import annotations

import struct
from dataclasses import dataclass, field

import numpy as np

from protocol_amd import engine as E

U = np.uint64
EMPTY = 0xFFFFFFFFFFFFFFFF
NOLOC = 0x7FEFFFFFFFFFFFFF              # PM_KEY_NOLOC: a candidate without a location
FLOOR = 0x03B8F2B061AEA073              # bits of 1e-290, rounded up (near_window)
ABSENT = 0xFFFFFFFE                     # a site no key sits at
KS = np.arange(1, E.PROP_KMAX + 1)


@dataclass(frozen=True)
class Geometry:
    name: str
    sb: int
    ulps: int
    band: float

    @property
    def mask(self):
        return (1 << self.sb) - 1

    @property
    def noloc_kb(self):
        return (NOLOC >> self.sb) << self.sb


# the two geometries rows run at (carve_propose_kernel)
GEOMETRIES = {"small": Geometry("small", E.ROW_SLOT_BITS, E.WINDOW_ULPS, E.TIE_BAND),
              "big": Geometry("big", E.ROW_SLOT_BITS_BIG, E.WINDOW_ULPS_BIG, E.TIE_BAND_BIG)}


@dataclass
class Case:
    name: str
    geom: Geometry
    keys: np.ndarray                    # u64[n_waves, n_per_wave], EMPTY = no candidate
    sites: np.ndarray                   # u32[1 << sb]
    uptos: tuple = (1 << 30,)           # how much of a row goes through the networks (the hook's `upto`)
    meta: dict = field(default_factory=dict)


def bits(a: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", a))[0]


# ---------------------------------------------------------------------------------------------------------------- reference
class Reference:
    def __init__(self, keys, sites, g: Geometry):
        keys = np.ascontiguousarray(keys, dtype=U)
        self.g, self.sites = g, np.asarray(sites, dtype=np.uint32)
        W, N = keys.shape
        s = np.sort(keys, axis=1)
        if N < 65:
            s = np.concatenate([s, np.full((W, 65 - N), EMPTY, dtype=U)], axis=1)
        self.s = s                                                   # all keys ascending, ~0 behind them
        self.row = s[:, :64]
        self.tau = self.row[:, 63].copy()
        hi = np.maximum(self.tau + U(g.ulps), U(FLOOR)) | U(g.mask)    # (wraps where tau is ~0: not used there)
        self.tau_hi = np.where(self.tau >= U(g.noloc_kb), self.tau, hi)  # location-less, or not full: no window
        self.n_all = (s != U(EMPTY)).sum(axis=1)
        self.kb = (s >> U(g.sb)) << U(g.sb)
        self.loc = (s != U(EMPTY)) & (self.kb != U(g.noloc_kb))
        self.a = np.where(self.loc, self.kb, U(0)).view(np.float64)
        self.site = self.sites[(s & U(g.mask)).astype(np.int64)]
        self.in_window = (s[:, 64:] < self.tau_hi[:, None])          # unlisted and below the window's end (a prefix)

    def answer(self, X):
        """X: u32[n_waves, nx] -> u64[n_waves, nx]: the smallest unlisted key below tau_hi whose site is not X, else ~0"""
        X = np.asarray(X, dtype=np.uint32)
        n = max(1, int(self.in_window.sum(axis=1).max()))
        unl, inw, us = self.s[:, 64:64 + n], self.in_window[:, :n], self.site[:, 64:64 + n]
        ok = inw[:, None, :] & (us[:, None, :] != X[:, :, None])
        first = ok.argmax(axis=2)
        return np.where(ok.any(axis=2), np.take_along_axis(unl, first, axis=1), U(EMPTY))

    def probe_sites(self):
        """the X worth asking: the sites of the in-window unlisted keys (all of the table's when those are few, else of the
        first sixteen such keys), the site of tau's entry, and one no key sits at"""
        W = self.s.shape[0]
        cols = [np.full((W, 1), ABSENT, dtype=np.uint32), self.site[:, 63:64]]
        uniq = np.unique(self.sites)
        if uniq.size <= 16:
            cols.append(np.broadcast_to(uniq[None, :], (W, uniq.size)))
        n = min(16, self.in_window.shape[1])
        cols.append(np.where(self.in_window[:, :n], self.site[:, 64:64 + n], np.uint32(ABSENT)))
        return np.concatenate(cols, axis=1).astype(np.uint32)

    def flags(self):
        """-> (u32[n_waves, 63] the flags word at K = 1 .. 63, u64[n_waves, 63, 64] the lanes' entries, dict of the fields)"""
        g, s = self.g, self.s
        band = g.band
        W = s.shape[0]
        lanes = np.arange(64)
        K = KS[None, :]
        n_tot = np.minimum(self.n_all, 64)
        n_k = np.minimum(n_tot[:, None], K)                          # [W, 63]
        mine = np.where(lanes[None, None, :] < n_k[:, :, None], self.row[:, None, :], U(EMPTY))
        loc, a, site = self.loc[:, :64], self.a[:, :64], self.site[:, :64]
        with np.errstate(invalid="ignore", over="ignore"):
            # clean: no two neighbouring entries within the band of each other sit at different sites
            pair_bad = (loc[:, :-1] & loc[:, 1:] & (a[:, 1:] - a[:, :-1] <= a[:, 1:] * (4.0 * band) + 1e-300)
                        & (site[:, 1:] != site[:, :-1]))
            cum = np.concatenate([np.zeros((W, 2), dtype=np.int64), np.cumsum(pair_bad, axis=1)], axis=1)  # cum[j]: pairs (i, i + 1), i + 1 < j
            clean = np.take_along_axis(cum, n_k, axis=1) == 0
            # safe: no listed term beyond PM_A_MAX_SAFE
            unsafe = loc & (a > E.A_MAX_SAFE)
            cum_u = np.concatenate([np.zeros((W, 1), dtype=np.int64), np.cumsum(unsafe, axis=1)], axis=1)
            safe = np.take_along_axis(cum_u, n_k, axis=1) == 0
            # j_tail: from which entry on the row lies within the band of its last entry
            le = np.maximum(n_k - 1, 0)
            a_le, loc_le = np.take_along_axis(a, le, axis=1), np.take_along_axis(loc, le, axis=1)
            within = (loc[:, None, :] & (lanes[None, None, :] < n_k[:, :, None])
                      & ((a_le[:, :, None] - a[:, None, :]) <= a[:, None, :] * band + 1e-300))
            j_tail = np.where((n_k > 0) & loc_le & within.any(axis=2), within.argmax(axis=2), n_k)
            # the tail: only where the row has its K entries
            full = n_k == K
            kk = np.broadcast_to(K, n_k.shape)
            beyond = np.where(self.n_all[:, None] > K, np.take_along_axis(s, kk, axis=1), U(EMPTY))
            e_last = np.take_along_axis(s, kk - 1, axis=1)
            a_last, loc_last = np.take_along_axis(self.a, kk - 1, axis=1), np.take_along_axis(self.loc, kk - 1, axis=1)
            a_b, loc_b = np.take_along_axis(self.a, kk, axis=1), np.take_along_axis(self.loc, kk, axis=1)
            site_last = np.take_along_axis(self.site, kk - 1, axis=1)
            nothing = (beyond == U(EMPTY)) | ~loc_last | ~loc_b      # nothing unlisted, or location-less on either side
            tail_clear = full & (nothing | (a_b - a_last > a_b * (4.0 * band) + 1e-300))
            decided = full & ~tail_clear
            band2 = a_last * (4.0 * band) + 1e-300
            tail_ok = np.zeros_like(decided)
            for j, k in enumerate(KS):                               # over ALL unlisted keys, not the row's lanes and a tracker
                w = np.nonzero(decided[:, j])[0]
                if w.size:
                    bad = (self.loc[w, k:] & (self.a[w, k:] - a_last[w, j, None] <= band2[w, j, None])
                           & (self.site[w, k:] != site_last[w, j, None]))
                    tail_ok[w, j] = ~bad.any(axis=1)
        complete = n_k < K
        word = (n_k | (j_tail << 8) | np.where(safe, E.ROW_SAFE, 0) | np.where(complete, E.ROW_COMPLETE, 0)
                | np.where(tail_ok, E.ROW_TAIL_OK, 0) | np.where(clean, E.ROW_CLEAN, 0) | np.where(tail_clear, E.ROW_TAIL_CLEAR, 0))
        fields = {"n_k": n_k, "j_tail": j_tail, "safe": safe, "complete": complete, "tail_ok": tail_ok, "clean": clean,
                  "tail_clear": tail_clear, "decided": decided, "e_last": e_last}
        return word.astype(np.uint32), mine, fields

    def entrants_per_call(self, keys):
        """keys in input order -> i64[n_waves, calls]: the keys of each 256-key call below the 64th smallest of everything
        in front of the call (what near_row_bulk4_body counts as n_ent)"""
        keys = np.asarray(keys, dtype=U)
        W, N = keys.shape
        out = []
        for c0 in range(0, N, 256):
            before = np.sort(np.concatenate([keys[:, :c0], np.full((W, 64), EMPTY, dtype=U)], axis=1), axis=1)[:, 63]
            out.append((keys[:, c0:c0 + 256] < before[:, None]).sum(axis=1))
        return np.stack(out, axis=1)


# --------------------------------------------------------------------------------------------------------------- generators
def _table(g: Geometry, n_sites: int, only: int | None = None):
    """site of slot s = s mod n_sites (one_site: `only` everywhere)"""
    if only is not None:
        return np.full(1 << g.sb, only, dtype=np.uint32)
    return (np.arange(1 << g.sb) % n_sites).astype(np.uint32)


def _slots_at(rng, g: Geometry, want, n_sites: int):
    """distinct slots per wave such that slot mod n_sites = want[w, i]"""
    W, N = want.shape
    out = np.zeros((W, N), dtype=U)
    per = (1 << g.sb) // n_sites
    for w in range(W):
        for x in range(n_sites):
            at = np.nonzero(want[w] == x)[0]
            assert at.size <= per, "more keys at a site than it has slots"
            out[w, at] = x + n_sites * rng.choice(per, size=at.size, replace=False)
    return out


def _pack(g: Geometry, v, slots, holes=None):
    keys = (np.asarray(v, dtype=U) << U(g.sb)) | np.asarray(slots, dtype=U)
    if holes is not None:
        keys[holes] = U(EMPTY)
    return keys


def _v(g: Geometry, a: float) -> int:
    return bits(a) >> g.sb


def _spread_case(name, g, seed, W, N, base_v, spread, n_sites, holes=0.0, noloc=0.0, only=None, uptos=(1 << 30,), meta=None):
    """values over `spread` truncation steps from base_v, sites at random"""
    rng = np.random.default_rng(seed)
    want = rng.integers(0, n_sites, size=(W, N))
    slots = _slots_at(rng, g, want, n_sites)
    v = U(base_v) + rng.integers(0, spread, size=(W, N), dtype=U)
    if noloc:
        v[rng.random((W, N)) < noloc] = U(NOLOC >> g.sb)
    keys = _pack(g, v, slots, rng.random((W, N)) < holes if holes else None)
    return Case(name, g, keys, _table(g, n_sites, only), uptos, meta or {})


BUSY_V = 1.37e-3
EDGE_KS = (1, 7, 33, 55, 63)         # the K of tests/test_near_row_model.py
UPTOS3 = (256, 300, 1 << 30)


def busy(g, W=32):
    return [_spread_case("busy", g, 101, W, 1024, _v(g, BUSY_V), 300, 3, holes=0.5, uptos=UPTOS3)]


LEVEL_CENTRES = {"mid": 1.37e-3, "above_2^-20": 2.0 ** -20 * (1 + 2.0 ** -26), "below_2^-20": None, "top_of_binade": 2.0 ** -19 * (1 - 2.0 ** -30)}
LEVEL_SEEDS, LEVEL_N, LEVEL_HOLES = 40, 512, 0.95


def levels(g):
    """ten levels 2.5 band units apart upwards from the centre (a unit = relative 4 band: two of the centres have the levels
    cross a power of two, where the truncation step doubles), in a level the offsets 0, 0.45, 0.9 units; a key sits at
    site level mod 3 with probability 0.985, else at the next site.  One wave per seed."""
    unit = 4.0 * g.band
    out = []
    for ci, (cname, centre) in enumerate(LEVEL_CENTRES.items()):
        if centre is None:
            centre = 2.0 ** -20 * (1 - 14 * unit)
        rng = np.random.default_rng(700 + ci)
        W, N = LEVEL_SEEDS, LEVEL_N
        lev = rng.integers(0, 10, size=(W, N))
        for w in range(0, W, 4):                                     # every fourth wave: the lowest level holds exactly K keys for one
            k = EDGE_KS[(w // 4) % len(EDGE_KS)]                     # of the K below, so that row ends where a level ends (tail_clear)
            lev[w] = np.where(lev[w] == 0, 1, lev[w])
            lev[w, :k] = 0
        off = rng.choice([0.0, 0.45, 0.9], size=(W, N))
        a = centre * (1.0 + (2.5 * lev + off) * unit)
        v = (a.view(U) >> U(g.sb))
        want = np.where(rng.random((W, N)) < 0.985, lev % 3, (lev + 1) % 3)
        holes = rng.random((W, N)) < rng.uniform(0.0, LEVEL_HOLES, size=(W, 1))   # rows of different lengths: K lands anywhere in the levels
        for w in range(0, W, 4):
            holes[w, :EDGE_KS[-1]] = False
        out.append(Case("levels-" + cname, g, _pack(g, v, _slots_at(rng, g, want, 3), holes), _table(g, 3)))
    return out


def floor(g, W=32):
    """every value below 1e-290 (and above 1e-296): the window is everything below the floor.  A tenth to four tenths of a
    wave's keys form a cluster of 1,000 steps at the bottom — within 1e-300 of each other, so within the band, and wider than
    tau + ulps: a row that ends in the cluster has its tail decided by keys only the floor keeps in the window — nearly all of
    them at one site; the rest lie anywhere above"""
    rng = np.random.default_rng(202)
    N = 320
    v = rng.integers(_v(g, 3e-295), _v(g, 1e-290) - 1, size=(W, N), dtype=U)
    cl = rng.random((W, N)) < rng.uniform(0.1, 0.4, size=(W, 1))
    v[cl] = (U(_v(g, 1e-295)) + rng.integers(0, 1000, size=(W, N), dtype=U))[cl]
    want = np.where(cl & (rng.random((W, N)) < 0.99), 0, rng.integers(0, 3, size=(W, N)))
    return [Case("floor", g, _pack(g, v, _slots_at(rng, g, want, 3)), _table(g, 3))]


def straddle(g, W=32):
    return [_spread_case("straddle", g, 203, W, 512, (FLOOR >> g.sb) - 200, 400, 3)]


def noloc_tail(g, W=32):
    return [_spread_case("noloc_tail", g, 204, W, 300, _v(g, BUSY_V), 300, 3, noloc=0.85)]


def noloc_some(g, W=32):
    return [_spread_case("noloc_some", g, 205, W, 300, _v(g, BUSY_V), 300, 3, noloc=0.30)]


def one_site(g, W=32):
    return [_spread_case("one_site", g, 206, W, 512, _v(g, BUSY_V), 300, 1, only=5)]


def sparse(g, W=32):
    """tests/test_gpu_row_networks.py's first shape: keys over 2^40 steps just above the floor, 4096 sites"""
    rng = np.random.default_rng(207)
    N = 740
    slots = np.stack([rng.permutation(1 << g.sb)[:N] for _ in range(W)]).astype(U)
    v = U((FLOOR >> g.sb) + 2) + rng.integers(0, 1 << 40, size=(W, N), dtype=U)
    sites = rng.integers(0, 4096, size=1 << g.sb, dtype=np.uint32)
    return [Case("sparse", g, _pack(g, v, slots), sites)]


def antipode(g, W=32):
    """short rows whose one or two last values lie a truncation step either side of PM_A_MAX_SAFE (or on it)"""
    rng = np.random.default_rng(208)
    N = 48
    v = U(_v(g, 0.3)) + rng.integers(0, 1 << 20, size=(W, N), dtype=U)
    holes = rng.random((W, N)) < 0.4
    v0 = _v(g, E.A_MAX_SAFE)
    assert (v0 << g.sb) == bits(E.A_MAX_SAFE)                         # the bound survives the truncation
    for w in range(W):
        for i in rng.permutation(N)[:rng.integers(1, 3)]:
            v[w, i] = v0 + int(rng.integers(-1, 2))
            holes[w, i] = False
    want = rng.integers(0, 3, size=(W, N))
    return [Case("antipode", g, _pack(g, v, _slots_at(rng, g, want, 3), holes), _table(g, 3))]


def edge_of_band(g, W=60):
    """The two bounds of the tail exactly met, and a truncation step either side.  Wave w: K = EDGE_KS[...], d = -1 / 0 / +1.
    kind 0: the first unlisted key b with a_b - a_last = a_b * 4 band exactly (+ d steps): a_b's mantissa is a multiple of
    2^47, so a_b (1 - 4 band) is a double with no bits in the slot field.  kind 1: behind some unlisted keys at the last entry's
    site, a key at another site with a - a_last = a_last * 4 band exactly (+ d steps).  Values at or above 1e-270."""
    rng = np.random.default_rng(209)
    N = 192
    sh = int(round(-np.log2(4.0 * g.band)))                          # 4 band = 2^-sh
    assert 2.0 ** -sh == 4.0 * g.band and sh + g.sb == 47
    v = np.zeros((W, N), dtype=U)
    want = np.zeros((W, N), dtype=np.int64)
    holes = np.zeros((W, N), dtype=bool)
    plan = []
    for w in range(W):
        kind, d, K = w % 2, (w // 2) % 3 - 1, EDGE_KS[(w // 6) % 5]
        expo = int(rng.integers(bits(1e-270) >> 52, bits(0.25) >> 52))
        m = (1 << 52) + int(rng.integers(1, 32)) * (1 << 47)          # 53-bit significand, a multiple of 2^47, not 2^52 itself
        if kind == 0:
            mb, ml = m, m - (m >> sh)                                # a_last = a_b (1 - 2^-sh)
            fill = 0
        else:
            ml, mb = m, m + (m >> sh)                                # a = a_last (1 + 2^-sh)
            fill = int(rng.integers(1, 90))                          # the key is in the row's lanes, or beyond lane 63
        assert (1 << 52) <= min(ml, mb) and max(ml, mb) < (1 << 53)
        v_last = ((expo << 52) | (ml - (1 << 52))) >> g.sb
        v_crit = (((expo << 52) | (mb - (1 << 52))) >> g.sb) + d
        i = 0
        v[w, :K - 1] = U(v_last - 4000) - rng.integers(0, 1 << 16, size=K - 1, dtype=U)  # in front of the last entry, far from it
        want[w, :K - 1] = rng.integers(0, 3, size=K - 1)
        i = K - 1
        v[w, i], want[w, i] = v_last, 0
        i += 1
        v[w, i:i + fill] = U(v_last) + rng.integers(0, 3, size=fill, dtype=U)   # unlisted, at the last entry's site, next to it
        want[w, i:i + fill] = 0
        i += fill
        v[w, i], want[w, i] = v_crit, 1
        i += 1
        n_far = int(rng.integers(0, N - i + 1))
        v[w, i:i + n_far] = U(v_crit + 4000) + rng.integers(0, 1 << 16, size=n_far, dtype=U)
        want[w, i:i + n_far] = rng.integers(0, 3, size=n_far)
        holes[w, i + n_far:] = True
        p = rng.permutation(N)                                       # (the order the sweep meets them in is not the order of size)
        v[w], want[w], holes[w] = v[w, p], want[w, p], holes[w, p]
        plan.append((kind, d, K))
    return [Case("edge_of_band", g, _pack(g, v, _slots_at(rng, g, want, 3), holes), _table(g, 3), meta={"plan": plan})]


LENGTHS = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513)


def lengths(g, W=32):
    out = []
    for n in LENGTHS:
        for holes in (0.0, 0.5):
            out.append(_spread_case(f"length-{n}-holes{holes}", g, 3000 + 2 * n + (holes > 0), W, n, _v(g, BUSY_V), 300, 3,
                                    holes=holes, meta={"n": n, "holes": holes}))
    c = _spread_case("length-513-stride-of-holes", g, 3998, W, 513, _v(g, BUSY_V), 300, 3, meta={"n": 513, "holes": None})
    c.keys[:, 128:192] = U(EMPTY)
    out.append(c)
    c = _spread_case("length-769-call-of-holes", g, 3999, W, 769, _v(g, BUSY_V), 300, 3, meta={"n": 769, "holes": None})
    c.keys[:, 256:512] = U(EMPTY)
    out.append(c)
    return out


S_MAX, P_KEYS = E.NET_SERIAL_MAX, E.NET_PACK_KEYS
ENTRANTS = (0, 1, S_MAX - 1, S_MAX, S_MAX + 1, 63, 64, 65, P_KEYS - 1, P_KEYS, P_KEYS + 1, 255, 256)
LAYOUTS = ("front", "spread", "back")


def entrants(g, W=32):
    """Call 0: 256 keys with values in [V0, V0 + 64).  Call c = 1 ..: ENTRANTS[c - 1] keys of value V0 - c — below everything
    in front of them, so each is an entrant — and in the other slots holes (one in two) or near misses with values in
    [V0 + 64, V0 + 104): above every threshold the row ever has, inside every window."""
    out = []
    V0 = _v(g, BUSY_V)
    for li, layout in enumerate(LAYOUTS):
        rng = np.random.default_rng(400 + li)
        N = 256 * (1 + len(ENTRANTS))
        v = np.zeros((W, N), dtype=U)
        holes = np.zeros((W, N), dtype=bool)
        v[:, :256] = U(V0) + rng.integers(0, 64, size=(W, 256), dtype=U)
        for c, n_e in enumerate(ENTRANTS, start=1):
            blk = slice(256 * c, 256 * (c + 1))
            v[:, blk] = U(V0 + 64) + rng.integers(0, 40, size=(W, 256), dtype=U)
            holes[:, blk] = rng.random((W, 256)) < 0.5
            for w in range(W):
                at = {"front": np.arange(n_e), "back": np.arange(256 - n_e, 256), "spread": rng.permutation(256)[:n_e]}[layout]
                v[w, 256 * c + at] = V0 - c
                holes[w, 256 * c + at] = False
        want = rng.integers(0, 3, size=(W, N))
        out.append(Case("entrants-" + layout, g, _pack(g, v, _slots_at(rng, g, want, 3), holes), _table(g, 3), UPTOS3,
                        meta={"layout": layout}))
    return out


FAMILIES = {"busy": busy, "levels": levels, "floor": floor, "straddle": straddle, "noloc_tail": noloc_tail, "noloc_some": noloc_some,
            "one_site": one_site, "sparse": sparse, "antipode": antipode, "edge_of_band": edge_of_band, "lengths": lengths,
            "entrants": entrants}
