"""The carve's distance key on the device against the exact Haversine term (protocol_amd/csrc/pm_validate.inc: sin_band,
hav_a, prox_a, pack_key; pm_kernels.hip: geo_of; pm_propose.inc: candidate_key), through pm_debug_distance_keys, which
runs geo_kernel and those device functions themselves.  Why the key's error has to stay within band / 4, and the
form's within band / 8: tests/test_distance_key_model.py.  "Exact" is the Haversine term of the reference's own f64
intermediates evaluated in high precision (tests/distance_key_model.py): mpmath at 50 digits on the named edge cases,
np.longdouble (cross-checked against mpmath) on a random sweep of a million pairs.

Bounds asserted, and the maxima this test measured on an MI355X (the bounds of the sine form and of geo_of are estimates;
nothing below is left to a tolerance chosen after the fact):
- sin_band, |x| <= 3.2: bit for bit the CPU emulation of its operations (measured: no bit differs, also in a build with
  -ffp-contract=off: the fma are written out).  Above 3.2 (OCML's sin): within 1 ulp of mpmath (measured 0.67 ulp).
- geo_of: every unit-vector component within 2.5e-16 absolute (measured 1.69e-16), cos(lat) within 2 ulp (measured 0.76).
- hav_a (the sine form): within 1e-14 relative (measured 8.0e-16).
- prox_a: the chord form exactly where the chord value is >= PM_A_CHORD_MIN, there bit for bit 0.25 * fma(dx, dx,
  fma(dy, dy, dz * dz)) of the device's unit vectors; its error within 1e-15 / sqrt(a) for longitudes less than 180
  degrees apart (measured 5.8e-16 / sqrt(a)), within 2e-15 / sqrt(a) the long way round (measured 1.25e-15 / sqrt(a):
  the reference's own fl(fl(lon2 - lon1) * RAD) rounds there, and the chord never forms it), and within band / 8 of the
  narrowest band wherever it is taken (measured 7.6e-13 against 1.8e-12).
- packed keys at the library's three slot widths, with a random slot: within band / 4 of the exact term (measured 0.124,
  0.125 and 0.125 of the band at 13, 18 and 21 bits: the truncation, band / 8, is nearly all of it).
- the order of clouds of near-equidistant candidates: pairs ordered against the reference lie within the band of each
  other (measured: 2.1e7 such pairs, at most 0.015 of the band apart at 13 bits).
"""
import math

import mpmath
import numpy as np
import pytest

from distance_key_model import (chord_a, exact_a_ld, exact_a_mp, sin_band, sin_band_points, sin_band_source, unit_ld,
                                unit_mp)
from protocol_amd import engine as E

pytestmark = pytest.mark.gpu

# the maxima of this run, printed (pytest -s) for the figures in the docstring
MEASURED = {"ocml_ulps": 0.0, "unit_abs": 0.0, "cos_ulps": 0.0, "hav_rel": 0.0, "chord_sqrt": 0.0, "chord_sqrt_long": 0.0,
            "chord_rel": 0.0, "packed_13": 0.0, "packed_18": 0.0, "packed_21": 0.0}
UNIT_ABS, COS_ULPS, HAV_REL, CHORD_SQRT, CHORD_SQRT_LONG = 2.5e-16, 2.0, 1e-14, 1e-15, 2e-15
N_RANDOM = 1 << 20


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _report(name, value):
    print(f"MEASURED {name} {value:.4g}")


@pytest.fixture(scope="module")
def eng():
    e = E.Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def geom(eng):
    g = eng.debug_key_geometry()
    assert g["slot_bits"] == tuple(sorted(g["slot_bits"])) and len(set(g["bands"])) == 3
    return g


# ---- sin_band on raw arguments

def test_sin_band_bit_for_bit_where_the_polynomial_runs(eng):
    src = sin_band_source()
    x = np.array(sin_band_points(src))
    got = eng.debug_sin_band(x)
    want = np.array([sin_band(v, src) for v in x.tolist()])
    bad = np.nonzero(_bits(got) != _bits(want))[0]
    assert bad.size == 0, [(x[i], got[i], want[i]) for i in bad[:8]]


def test_sin_band_beyond_the_polynomial_is_ocml_within_one_ulp(eng):
    """|x| > 3.2: half a difference of longitudes outside [-180, 180] (what is no difference of two in-range longitudes)."""
    src = sin_band_source()
    rng = np.random.default_rng(5)
    t = src["ocml"]
    x = [math.nextafter(t, math.inf), 3.2000000000000006, 2 * math.pi, 3 * math.pi / 2, 4.0, 5.0, 6.283185307179586, 9.42477796076938,
         12.566370614359172, 100.0, 1e4]
    x += rng.uniform(t, 4 * math.pi, 2000).tolist()
    x += ((rng.uniform(-540, 540, 500) - rng.uniform(-540, 540, 500)) * (math.pi / 180) * 0.5).tolist()
    x = np.array([v for v in x if abs(v) > t])
    x = np.concatenate([x, -x])
    got = eng.debug_sin_band(x)
    worst = 0.0
    with mpmath.workdps(50):
        for v, g in zip(x.tolist(), got.tolist()):
            w = mpmath.sin(mpmath.mpf(v))
            ulps = float(abs(mpmath.mpf(g) - w)) / float(np.spacing(abs(float(w))))
            worst = max(worst, ulps)
            assert ulps <= 1.0, (v, g, w)
    MEASURED["ocml_ulps"] = worst
    _report("ocml_ulps", worst)


# ---- pairs: the named edge cases (mpmath) and a random sweep (long double)

def _dest(lat, lon, bearing, delta):
    """the point `delta` radians from (lat, lon) along `bearing` (f64 spherical trigonometry: only where the pair lies matters;
    its exact term is computed afterwards from the rounded coordinates)"""
    p1, l1 = np.radians(lat), np.radians(lon)
    p2 = np.arcsin(np.clip(np.sin(p1) * np.cos(delta) + np.cos(p1) * np.sin(delta) * np.cos(bearing), -1.0, 1.0))
    l2 = l1 + np.arctan2(np.sin(bearing) * np.sin(delta) * np.cos(p1), np.cos(delta) - np.sin(p1) * np.sin(p2))
    lon2 = (np.degrees(l2) + 180.0) % 360.0 - 180.0
    return np.degrees(p2), lon2


def _ulp_walk(x, ks):
    return np.asarray(x, np.float64) + np.asarray(ks, np.float64) * np.spacing(np.float64(x))


def _bisect(f, lo, hi, iters=200):
    """the t where f changes sign on [lo, hi] (f(lo) < 0 <= f(hi))"""
    for _ in range(iters):
        mid = 0.5 * (lo + hi)
        if mid in (lo, hi):
            break
        lo, hi = (mid, hi) if f(mid) < 0 else (lo, mid)
    return hi


# the pairs whose chord value straddles PM_A_CHORD_MIN: (name, lat1, lon1, which coordinate of point 2 moves, direction)
STRADDLES = [("ns_equator", 0.0, 10.0, (1.0, 0.0)), ("ew_equator", 0.0, 0.0, (0.0, 1.0)), ("ns_lat80", 80.0, -30.0, (1.0, 0.0)),
             ("ew_lat80", 80.0, 0.0, (0.0, 1.0)), ("diag_south", -45.0, 100.0, (-0.6, 0.8)), ("ew_antimeridian", 12.0, 179.95, (0.0, 1.0))]


def _straddle_seed(lat1, lon1, d, a_target):
    """point 2 = point 1 + t * d (degrees; longitude steps widened by 1 / cos(lat)) with the exact term at a_target"""
    sc = 1.0 / math.cos(math.radians(lat1)) if d[1] else 1.0

    def pt(t):
        return lat1 + t * d[0], lon1 + t * d[1] * sc

    def f(t):
        la, lo = pt(t)
        return float(exact_a_ld([lat1], [lon1], [la], [lo])[0]) - a_target

    la, lo = pt(_bisect(f, 0.0, 1.0))
    return la, (lo - 360.0 if lo > 180.0 else lo)  # (across the antimeridian: dlon near -360 degrees)


def edge_cases(geom):
    """name -> (lat1, lon1, lat2, lon2) of the named edge cases, before the straddles (which need a device call to place)"""
    rng = np.random.default_rng(7)
    C = {}
    n = 64
    la = rng.uniform(-89, 89, n)
    C["antimeridian"] = (la, np.full(n, 179.99999999), la + rng.normal(0, 1e-3, n), np.full(n, -179.99999999))
    C["antimeridian_full_turn"] = (la, np.full(n, 180.0), la, np.full(n, -180.0))
    C["antimeridian_near"] = (la, rng.uniform(179.9, 180.0, n), rng.uniform(-89, 89, n), rng.uniform(-180.0, -179.9, n))
    C["lon_beyond_180"] = (la, rng.uniform(-540, 540, n), rng.uniform(-89, 89, n), rng.uniform(-540, 540, n))
    poles = np.array([90.0, np.nextafter(90.0, 0.0), -90.0, np.nextafter(-90.0, 0.0)])
    p1 = np.repeat(poles, 16)
    C["poles"] = (p1, rng.uniform(-180, 180, 64), np.tile(poles, 16), rng.uniform(-180, 180, 64))
    C["pole_to_anywhere"] = (p1, rng.uniform(-180, 180, 64), rng.uniform(-90, 90, 64), rng.uniform(-180, 180, 64))
    C["equator"] = (np.zeros(n), rng.uniform(-180, 180, n), np.where(np.arange(n) % 2 == 0, 0.0, -0.0), rng.uniform(-180, 180, n))
    big = np.concatenate([np.array([89.9999, 89.5, -89.99, 45.0, -60.0, 0.5, 179.0 / 2]), rng.uniform(-89.9, 89.9, 25)])
    lon_any = rng.uniform(-180, 180, 32)
    C["ulp_apart_lat"] = (big, lon_any, np.nextafter(big, 90.0 * np.sign(big)), lon_any)
    lons = np.concatenate([np.array([179.99999, -179.999, 120.0, -90.5]), rng.uniform(-180, 180, 28)])
    C["ulp_apart_lon"] = (big, lons, big, np.nextafter(lons, 0.0))
    C["ulp_apart_both"] = (big, lons, np.nextafter(big, 0.0), np.nextafter(lons, 1000.0))
    # around PM_A_MAX_SAFE, never beyond it (antipodes lie outside the reference's domain: test_gpu_geography.py)
    m = 256
    s_lat, s_lon = rng.uniform(-80, 80, m), rng.uniform(-180, 180, m)
    eps = np.geomspace(1e-14, 1e-7, m)
    theta = 2.0 * np.arcsin(np.sqrt(geom["a_max_safe"] * (1.0 - eps)))
    t_lat, t_lon = _dest(s_lat, s_lon, rng.uniform(0, 2 * np.pi, m), theta)
    safe = exact_a_ld(s_lat, s_lon, t_lat, t_lon) <= geom["a_max_safe"]
    assert safe.sum() > m // 2
    C["max_safe"] = (s_lat[safe], s_lon[safe], t_lat[safe], t_lon[safe])
    # distances on a log scale, 1 mm to a quarter of the world, so every regime of the forms is met
    m = 512
    s_lat, s_lon = rng.uniform(-85, 85, m), rng.uniform(-180, 180, m)
    t_lat, t_lon = _dest(s_lat, s_lon, rng.uniform(0, 2 * np.pi, m), np.geomspace(1.6e-10, 1.6, m))
    C["log_distances"] = (s_lat, s_lon, t_lat, t_lon)
    return {k: tuple(np.asarray(v, np.float64) for v in c) for k, c in C.items()}


@pytest.fixture(scope="module")
def edges(eng, geom):
    """the edge cases, the straddles of PM_A_CHORD_MIN placed in two device calls (a coarse walk finds where the device's
    chord value crosses it, a dense walk of single ulps covers both sides), and the device's answers"""
    cm = geom["chord_min"]
    C = edge_cases(geom)
    coarse = {}
    for name, lat1, lon1, d in STRADDLES:
        lat2, lon2 = _straddle_seed(lat1, lon1, d, cm)
        ks = np.arange(-8192, 8193, 32)
        coarse[name] = (lat1, lon1, lat2, lon2, d, ks)
    cat = [(np.full(ks.size, la1), np.full(ks.size, lo1), _ulp_walk(la2, ks) if d[0] else np.full(ks.size, la2),
            _ulp_walk(lo2, ks) if d[1] else np.full(ks.size, lo2)) for la1, lo1, la2, lo2, d, ks in coarse.values()]
    out = eng.debug_distance_keys(*(np.concatenate([c[i] for c in cat]) for i in range(4)))
    off = 0
    for (name, (la1, lo1, la2, lo2, d, ks)) in zip(list(coarse), coarse.values()):
        chord = out["chord"][off:off + ks.size]
        off += ks.size
        flips = np.nonzero(chord[1:] != chord[:-1])[0]
        assert flips.size, f"{name}: the chord value does not cross PM_A_CHORD_MIN within +-8192 ulps"
        k0 = ks[flips[0]]
        kk = np.arange(k0 - 48, k0 + 80)
        C["straddle_" + name] = (np.full(kk.size, la1), np.full(kk.size, lo1), _ulp_walk(la2, kk) if d[0] else np.full(kk.size, la2),
                                 _ulp_walk(lo2, kk) if d[1] else np.full(kk.size, lo2))
    names = list(C)
    sizes = [C[k][0].size for k in names]
    lat1, lon1, lat2, lon2 = (np.concatenate([C[k][i] for k in names]) for i in range(4))
    rng = np.random.default_rng(3)
    slots = rng.integers(0, 1 << 21, lat1.size)
    dev = eng.debug_distance_keys(lat1, lon1, lat2, lon2, slots)
    exact_mp = exact_a_mp(lat1, lon1, lat2, lon2)
    exact = np.array([float(v) for v in exact_mp])
    case = np.repeat(np.arange(len(names)), sizes)
    return {"names": names, "case": case, "pts": (lat1, lon1, lat2, lon2), "slots": slots, "dev": dev, "exact": exact,
            "exact_mp": exact_mp}


@pytest.fixture(scope="module")
def sweep(eng, geom):
    """a million random pairs: half anywhere on the globe, half at distances on a log scale; exact terms in long double"""
    assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is not the x87 extended format here"
    rng = np.random.default_rng(2024)
    h = N_RANDOM // 2
    lat1 = np.degrees(np.arcsin(rng.uniform(-1, 1, N_RANDOM)))
    lon1 = rng.uniform(-180, 180, N_RANDOM)
    lat2 = np.degrees(np.arcsin(rng.uniform(-1, 1, h)))
    lon2 = rng.uniform(-180, 180, h)
    nlat, nlon = _dest(lat1[h:], lon1[h:], rng.uniform(0, 2 * np.pi, h), 10.0 ** rng.uniform(-9.5, 0.3, h))
    lat2, lon2 = np.concatenate([lat2, nlat]), np.concatenate([lon2, nlon])
    exact = exact_a_ld(lat1, lon1, lat2, lon2)
    keep = exact <= geom["a_max_safe"]
    lat1, lon1, lat2, lon2, exact = lat1[keep], lon1[keep], lat2[keep], lon2[keep], exact[keep]
    slots = rng.integers(0, 1 << 21, lat1.size)
    dev = eng.debug_distance_keys(lat1, lon1, lat2, lon2, slots)
    return {"pts": (lat1, lon1, lat2, lon2), "slots": slots, "dev": dev, "exact": exact}


def _ld_to_mp(v):
    """a long double as an mpf, exactly (its 64-bit significand is the sum of two f64)"""
    hi = float(v)
    return mpmath.mpf(hi) + mpmath.mpf(float(v - np.longdouble(hi)))


def test_long_double_reference_agrees_with_mpmath(sweep):
    rng = np.random.default_rng(1)
    idx = rng.choice(sweep["exact"].size, 2500, replace=False)
    pts = [p[idx] for p in sweep["pts"]]
    mp = exact_a_mp(*pts)
    ld = sweep["exact"][idx]
    with mpmath.workdps(50):
        rel = max(float(abs((_ld_to_mp(v) - m) / m)) for v, m in zip(ld, mp))
        assert rel < 1e-17, rel
        cu = unit_ld(pts[0], pts[1])
        for i in range(0, 2500, 5):
            want = unit_mp(pts[0][i], pts[1][i])
            for k in range(4):
                assert abs(_ld_to_mp(cu[k][i]) - want[k]) < 1e-18, (i, k)


def _cases(edges, name):
    return edges["case"] == edges["names"].index(name)


def _check_geo(dev, lat1, lon1, lat2, lon2, exact_units):
    """exact_units(lat, lon) -> (cos, ux, uy, uz) as f64 arrays of the exact value and of its residual"""
    worst_abs, worst_cos = 0.0, 0.0
    for side, (la, lo) in (("1", (lat1, lon1)), ("2", (lat2, lon2))):
        (c, cr), *units = exact_units(la, lo)
        got_u = dev["u" + side]
        for k, (w, wr) in enumerate(units):
            err = np.abs((got_u[:, k] - w) - wr)
            worst_abs = max(worst_abs, float(err.max()))
            assert err.max() <= UNIT_ABS, (side, k, int(err.argmax()), float(err.max()))
        ulps = np.abs((dev["cos" + side] - c) - cr) / np.spacing(np.abs(c))
        worst_cos = max(worst_cos, float(ulps.max()))
        assert ulps.max() <= COS_ULPS, (side, int(ulps.argmax()), float(ulps.max()))
    return worst_abs, worst_cos


def _units_mp(la, lo):
    vals = [unit_mp(a, b) for a, b in zip(la.tolist(), lo.tolist())]
    out = []
    for k in range(4):
        w = np.array([float(v[k]) for v in vals])
        r = np.array([float(v[k] - mpmath.mpf(float(v[k]))) for v in vals])
        out.append((w, r))
    return out


def _units_ld(la, lo):
    out = []
    for v in unit_ld(la, lo):
        w = v.astype(np.float64)
        out.append((w, (v - w.astype(np.longdouble)).astype(np.float64)))
    return out


def test_geo_of(edges, sweep):
    a1, c1 = _check_geo(edges["dev"], *edges["pts"], _units_mp)
    a2, c2 = _check_geo(sweep["dev"], *sweep["pts"], _units_ld)
    MEASURED["unit_abs"], MEASURED["cos_ulps"] = max(a1, a2), max(c1, c2)
    _report("unit_abs", max(a1, a2))
    _report("cos_ulps", max(c1, c2))


def _rel(got, exact):
    """|got - exact| / exact with exact in long double (or an f64 array of mpmath values plus residuals)"""
    return np.abs((np.asarray(got, np.longdouble) - exact) / exact).astype(np.float64)


def _exact_ld(edges):
    with mpmath.workdps(50):
        r = np.array([float(m - mpmath.mpf(float(m))) for m in edges["exact_mp"]])
    return edges["exact"].astype(np.longdouble) + r.astype(np.longdouble)


def _check_forms(dev, exact, cm, band0, where, lon1, lon2):
    nz = exact > 0
    hav = _rel(dev["hav_a"][nz], exact[nz])
    assert hav.max() <= HAV_REL, (where, float(hav.max()))
    ch = dev["chord"] & nz
    rel = _rel(dev["prox_a"][ch], exact[ch])
    # The 1 / sqrt(a) law: the chord form sees each point, the reference the rounded difference fl(fl(lon2 - lon1) * RAD).
    # Less than 180 degrees apart that rounding is small (1e-15 / sqrt(a)); the long way round it is up to ~9e-16 radians
    # (2e-15 / sqrt(a)); with longitudes beyond +-180 it has no bound worth the name and only band / 8 is asserted.
    in_range = ((np.abs(lon1) <= 180.0) & (np.abs(lon2) <= 180.0))[ch]
    long_way = (np.abs(np.asarray(lon2) - np.asarray(lon1)) > 180.0)[ch]
    scaled = rel * np.sqrt(exact[ch].astype(np.float64)) * in_range
    assert scaled[~long_way].max(initial=0.0) <= CHORD_SQRT, (where, float(scaled[~long_way].max(initial=0.0)))
    assert scaled[long_way].max(initial=0.0) <= CHORD_SQRT_LONG, (where, float(scaled[long_way].max(initial=0.0)))
    MEASURED["chord_sqrt_long"] = max(MEASURED["chord_sqrt_long"], float(scaled[long_way].max(initial=0.0)))
    scaled = scaled[~long_way]
    assert rel.max(initial=0.0) <= band0 / 8, (where, float(rel.max(initial=0.0)), band0 / 8)
    # the sine form below: prox_a is hav_a, bit for bit; candidate_key (the proposer's copy) is prox_a, bit for bit
    assert np.array_equal(_bits(dev["prox_a"][~dev["chord"]]), _bits(dev["hav_a"][~dev["chord"]])), where
    assert np.array_equal(_bits(dev["candidate_key"]), _bits(dev["prox_a"])), where
    # the chord form is taken exactly where the chord value reaches PM_A_CHORD_MIN (long double: clear of the threshold)
    d = (dev["u2"] - dev["u1"]).astype(np.longdouble)
    cv = 0.25 * (d * d).sum(axis=1)
    clear = np.abs(cv - cm) > 1e-12 * cm
    assert np.array_equal(dev["chord"][clear], (cv >= cm)[clear]), where
    return float(hav.max()), float(scaled.max(initial=0.0)), float(rel.max(initial=0.0))


def _check_packed(dev, exact, slots, geom, where):
    out = []
    nz = exact > 0
    for w, (sb, band) in enumerate(zip(geom["slot_bits"], geom["bands"])):
        mask = np.uint64((1 << sb) - 1)
        for form, src in (("packed_prox", "prox_a"), ("packed_hav", "hav_a")):
            key = dev[form][:, w]
            assert np.array_equal(key & mask, slots.astype(np.uint64) & mask), (where, form, sb)
            assert np.array_equal(key >> np.uint64(sb), _bits(dev[src]) >> np.uint64(sb)), (where, form, sb)
            rel = _rel(key[nz].view(np.float64), exact[nz])
            assert rel.max() <= band / 4, (where, form, sb, float(rel.max()), band / 4)
            out.append((sb, float(rel.max()) / band))
    return out


def test_edge_cases_forms_and_keys(edges, geom):
    """every named edge case: geo_of is checked in test_geo_of; here the forms and the packed keys, case by case"""
    exact = _exact_ld(edges)
    worst = {}
    for i, name in enumerate(edges["names"]):
        sel = edges["case"] == i
        dev = {k: v[sel] for k, v in edges["dev"].items()}
        h, s, r = _check_forms(dev, exact[sel], geom["chord_min"], geom["bands"][0], name, edges["pts"][1][sel], edges["pts"][3][sel])
        worst["hav_rel"] = max(worst.get("hav_rel", 0.0), h)
        worst["chord_sqrt"] = max(worst.get("chord_sqrt", 0.0), s)
        worst["chord_rel"] = max(worst.get("chord_rel", 0.0), r)
        for sb, f in _check_packed(dev, exact[sel], edges["slots"][sel], geom, name):
            worst[f"packed_{sb}"] = max(worst.get(f"packed_{sb}", 0.0), f)
    for k, v in worst.items():
        MEASURED[k] = max(MEASURED.get(k, 0.0), v)
        _report("edges_" + k, v)


def test_chord_min_is_straddled_and_the_chord_is_the_emulated_one(edges, geom):
    """On each straddle both forms occur a few ulps apart, the form follows the device's chord value exactly, and the
    chord form is 0.25 * fma(dx, dx, fma(dy, dy, dz * dz)) of the device's unit vectors, bit for bit (every straddle
    pair and every other edge pair)."""
    cm = geom["chord_min"]
    dev = edges["dev"]
    emu = np.array([chord_a(u1, u2) for u1, u2 in zip(dev["u1"], dev["u2"])])
    assert np.array_equal(dev["chord"], emu >= cm)
    took = dev["chord"]
    assert np.array_equal(_bits(dev["prox_a"][took]), _bits(emu[took]))
    for name, *_ in STRADDLES:
        sel = _cases(edges, "straddle_" + name)
        c = dev["chord"][sel]
        assert c.any() and (~c).any(), name
        if name.endswith("equator"):  # (coordinates near 0: one ulp of them moves a by about one ulp)
            v = emu[sel]
            below, above = v[v < cm].max(), v[v >= cm].min()
            assert (above - below) <= 8 * np.spacing(cm), (name, below, above)


def test_random_sweep_forms_and_keys(sweep, geom):
    dev, exact = sweep["dev"], sweep["exact"]
    assert exact.size > 0.99 * N_RANDOM
    assert dev["chord"].sum() > 0.5 * exact.size and (~dev["chord"]).sum() > 1000
    h, s, r = _check_forms(dev, exact, geom["chord_min"], geom["bands"][0], "random", sweep["pts"][1], sweep["pts"][3])
    MEASURED["hav_rel"] = max(MEASURED["hav_rel"], h)
    MEASURED["chord_sqrt"] = max(MEASURED["chord_sqrt"], s)
    MEASURED["chord_rel"] = max(MEASURED["chord_rel"], r)
    for sb, f in _check_packed(dev, exact, sweep["slots"], geom, "random"):
        MEASURED[f"packed_{sb}"] = max(MEASURED[f"packed_{sb}"], f)
    # a subset bit for bit against the emulated chord
    idx = np.random.default_rng(4).choice(exact.size, 20000, replace=False)
    emu = np.array([chord_a(dev["u1"][i], dev["u2"][i]) for i in idx])
    assert np.array_equal(dev["chord"][idx], emu >= geom["chord_min"])
    took = dev["chord"][idx]
    assert np.array_equal(_bits(dev["prox_a"][idx][took]), _bits(emu[took]))
    for k in ("hav_rel", "chord_sqrt", "chord_rel", "packed_13", "packed_18", "packed_21"):
        _report(k, MEASURED[k])


# ---- the order of whole clouds against the reference's d

def _cloud(rng, lat0, lon0, theta, n):
    """n candidates around (lat0, lon0) at nearly one distance theta (radians): the radius jittered by 2^-e, e in [20, 56],
    so gaps fall on both sides of every band; a tenth repeats earlier coordinates, some with a signed zero flipped"""
    e = rng.integers(20, 57, n)
    delta = theta * (1.0 + rng.choice([-1.0, 1.0], n) * rng.random(n) * np.ldexp(1.0, -e))
    lat, lon = _dest(np.full(n, lat0), np.full(n, lon0), rng.uniform(0, 2 * np.pi, n), delta)
    rep = rng.random(n) < 0.1
    src = rng.integers(0, n, n)
    lat = np.where(rep, lat[src], lat)
    lon = np.where(rep, lon[src], lon)
    lat[:4], lon[:4] = [0.0, -0.0, 0.0, 5.0], [lon0, lon0, -0.0, 0.0]
    return lat, lon


CLOUD_SEEDS = [(47.37, 8.54), (0.0, 0.0), (-89.9, 179.99), (12.0, 179.9999), (64.1, -21.9)]
CLOUD_THETAS = [1e-7, 1.5e-3, 1.6e-3, 0.05, 1.0, 2.5, 3.13]  # (radians; a stays below PM_A_MAX_SAFE)


def test_order_against_the_reference(eng, geom):
    """Clouds of candidates at nearly equal distances from a seed: every pair the packed keys order against the reference's
    d (glibc, stable by input order; the slot is the input position) lies within the band of each other — what the
    certificate then catches — at every width and for both forms."""
    from oracle import oracle_ffi as orc
    rng = np.random.default_rng(17)
    n = 1200
    inverted = 0
    widest = [0.0, 0.0, 0.0]
    for lat0, lon0 in CLOUD_SEEDS:
        for theta in CLOUD_THETAS:
            lat, lon = _cloud(rng, lat0, lon0, theta, n)
            dev = eng.debug_distance_keys(np.full(n, lat0), np.full(n, lon0), lat, lon, np.arange(n))
            d = orc.distance_column(lat0, lon0, lat, lon)
            if not np.all(np.isfinite(d)):
                continue
            rr = np.empty(n, np.int64)
            rr[np.argsort(d, kind="stable")] = np.arange(n)
            for form in ("packed_prox", "packed_hav"):
                for w, band in enumerate(geom["bands"]):
                    key = dev[form][:, w]
                    rk = np.empty(n, np.int64)
                    rk[np.argsort(key)] = np.arange(n)
                    inv = np.triu((rk[:, None] < rk[None, :]) != (rr[:, None] < rr[None, :]), 1)
                    i, j = np.nonzero(inv)
                    if i.size == 0:
                        continue
                    kv = key.view(np.float64)
                    gap = np.abs(kv[i] - kv[j]) / np.maximum(kv[i], kv[j])
                    assert gap.max() <= band, (lat0, lon0, theta, form, w, int(i[gap.argmax()]), int(j[gap.argmax()]), float(gap.max()))
                    inverted += i.size
                    widest[w] = max(widest[w], float(gap.max()) / band)
    assert inverted > 0, "no cloud came near enough to the band to order a pair differently"
    _report("inverted_pairs", inverted)
    for w, f in enumerate(widest):
        _report(f"inverted_gap_over_band_{geom['slot_bits'][w]}", f)


# ---- one site, one key

def test_one_site_one_key(eng):
    """Candidates the host interns as one site (identical bits, +-0 folded: pm_engine_workers.inc site_key) get bit-identical
    keys from hav_a and from prox_a against any seed, and identical coordinates give exactly 0."""
    rng = np.random.default_rng(23)
    seeds_lat = np.concatenate([[0.0, -0.0, 90.0, -90.0, 45.0, 0.0], rng.uniform(-90, 90, 58)])
    seeds_lon = np.concatenate([[0.0, -0.0, 0.0, 180.0, -0.0, 179.999], rng.uniform(-180, 180, 58)])
    lt = float(rng.uniform(-80, 80))
    ln = float(rng.uniform(-180, 180))
    variants = [[(0.0, ln), (-0.0, ln)], [(lt, 0.0), (lt, -0.0)], [(0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0)],
                [(0.0, 180.0), (-0.0, 180.0)], [(lt, ln), (lt, ln)]]
    s_lat, s_lon, c_lat, c_lon = [], [], [], []
    for vs in variants:
        for (la, lo) in vs:
            s_lat += seeds_lat.tolist()
            s_lon += seeds_lon.tolist()
            c_lat += [la] * seeds_lat.size
            c_lon += [lo] * seeds_lat.size
    dev = eng.debug_distance_keys(np.array(s_lat), np.array(s_lon), np.array(c_lat), np.array(c_lon))
    m = seeds_lat.size
    off = 0
    for vs in variants:
        first = slice(off, off + m)
        for v in range(1, len(vs)):
            other = slice(off + v * m, off + (v + 1) * m)
            for f in ("hav_a", "prox_a", "candidate_key"):
                assert np.array_equal(_bits(dev[f][first]), _bits(dev[f][other])), (vs, f)
        off += len(vs) * m
    # identical coordinates (and their +-0 twins): exactly 0
    pts_lat = np.concatenate([seeds_lat, [0.0, -0.0, lt, 90.0, -90.0]])
    pts_lon = np.concatenate([seeds_lon, [-0.0, 0.0, ln, 180.0, -180.0]])
    twin_lat = np.where(pts_lat == 0.0, -pts_lat, pts_lat)
    twin_lon = np.where(pts_lon == 0.0, -pts_lon, pts_lon)
    for la2, lo2 in ((pts_lat, pts_lon), (twin_lat, twin_lon)):
        dev = eng.debug_distance_keys(pts_lat, pts_lon, la2, lo2)
        for f in ("hav_a", "prox_a", "candidate_key"):
            assert np.all(dev[f] == 0.0), (f, np.nonzero(dev[f] != 0.0)[0][:5])


def test_measured_maxima_stay_below_their_bounds():
    """(the maxima above, gathered by the tests of this module when they ran first; printed for the docstring)"""
    for k, v in MEASURED.items():
        _report("final_" + k, v)
