"""The carve's distance key on the CPU, for tests/test_distance_key_model.py and tests/test_gpu_distance_key.py.

- `device_constants()` and `sin_band_source()` parse the key's constants and sin_band's coefficients out of
  protocol_amd/csrc/pm_device.h and pm_validate.inc, so the tests follow edits of the sources;
- `sin_band()` emulates the device's sin_band operation by operation (each fma, * and + rounded once, the fma through
  `fractions.Fraction`), `chord_a()` the chord form of prox_a the same way;
- `exact_a_mp()` / `exact_a_ld()` are the Haversine term of the reference's own f64 intermediates — fl(fl(lat2 - lat1) * RAD),
  fl(lat * RAD), RAD = fl(pi / 180) as Rust's to_radians has it — with sin, cos, the products and the sum in high precision
  (mpmath at 50 digits; np.longdouble for sweeps too large for mpmath).  `unit_mp()` is the same for geo_of's unit vector.
"""
import math
import os
import re
from fractions import Fraction

import mpmath
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "protocol_amd", "csrc")
RAD = 3.14159265358979323846 / 180.0  # f64::to_radians: self * (PI / 180)
DPS = 50


def _read(name: str) -> str:
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _const_expr(text: str) -> float:
    """a constexpr initialiser of numbers, / - + * and parentheses, evaluated in f64 like the compiler does"""
    assert re.fullmatch(r"[0-9.eE+\-*/() ]+", text), text
    return float(eval(text, {"__builtins__": {}}))


def device_constants() -> dict:
    s = _read("pm_device.h")

    def get(name):
        m = re.search(r"static constexpr \w+ " + name + r" = ([^;]+);", s)
        assert m, name
        return _const_expr(m.group(1))

    return {"chord_min": get("PM_A_CHORD_MIN"), "a_max_safe": get("PM_A_MAX_SAFE"), "rad": get("PM_RAD"),
            "slot_bits": tuple(int(get(n)) for n in ("PM_CARVE_SLOT_BITS", "PM_CARVE_SLOT_BITS_BIG", "PM_CARVE_SLOT_BITS_MEM")),
            "bands": tuple(get(n) for n in ("PM_TIE_BAND", "PM_TIE_BAND_BIG", "PM_TIE_BAND_MEM"))}


_NUM = r"(-?[0-9.]+(?:e-?[0-9]+)?)"


def sin_band_source() -> dict:
    """sin_band's thresholds, pi pieces and coefficients (highest power first).  The pattern is the function's whole
    shape: a change of its structure fails here, loudly, instead of leaving the emulation behind."""
    s = _read("pm_validate.inc")
    m = re.search(r"__device__ __forceinline__ double sin_band\(double x\) \{(.*?)\n\}", s, re.S)
    assert m, "sin_band not found in pm_validate.inc"
    body = " ".join(re.sub(r"//[^\n]*", "", m.group(1)).split())
    shape = (r"double ax = fabs\(x\); if \(ax > {n}\) \{{ if \(ax > {n}\) return sin\(x\); ax = \({n} - ax\) \+ {n}; "
             r"x = x < 0\.0 \? -ax : ax; \}} const double z = x \* x; double p = {n}; ((?:p = fma\(p, z, -?[0-9.e-]+\); )+)"
             r"return fma\(x \* z, p, x\);").format(n=_NUM)
    mm = re.fullmatch(shape, body)
    assert mm, "sin_band's shape changed: update tests/distance_key_model.py with it\n" + body
    reflect, ocml, pi_hi, pi_lo, c0, steps = mm.groups()
    coefs = [float(c0)] + [float(c) for c in re.findall(r"p = fma\(p, z, (-?[0-9.e-]+)\);", steps)]
    return {"reflect": float(reflect), "ocml": float(ocml), "pi_hi": float(pi_hi), "pi_lo": float(pi_lo), "coefs": coefs}


def fma(a: float, b: float, c: float) -> float:
    """a * b + c rounded once (round to nearest even, like v_fma_f64)"""
    r = Fraction(a) * Fraction(b) + Fraction(c)
    if r == 0:  # the sign of an exact zero: that of a * b + c in f64 when the product is zero, else +0
        return a * b + c if (a == 0.0 or b == 0.0) else 0.0
    return float(r)  # (int / int true division: correctly rounded, subnormals included)


def sin_band(x: float, src: dict) -> float | None:
    """the device's sin_band, operation by operation; None where it calls OCML's sin"""
    ax = abs(x)
    if ax > src["reflect"]:
        if ax > src["ocml"]:
            return None
        ax = (src["pi_hi"] - ax) + src["pi_lo"]
        x = -ax if x < 0.0 else ax
    z = x * x
    p = src["coefs"][0]
    for c in src["coefs"][1:]:
        p = fma(p, z, c)
    return fma(x * z, p, x)


def chord_a(u1, u2) -> float:
    """prox_a's chord form from two unit vectors, operation by operation: 0.25 * fma(dx, dx, fma(dy, dy, dz * dz))"""
    dx, dy, dz = float(u2[0]) - float(u1[0]), float(u2[1]) - float(u1[1]), float(u2[2]) - float(u1[2])
    return 0.25 * fma(dx, dx, fma(dy, dy, dz * dz))


def halves(lat1, lon1, lat2, lon2):
    """the reference's f64 intermediates: dlat, dlon (radians, not yet halved) and lat1, lat2 in radians"""
    lat1, lon1, lat2, lon2 = (np.asarray(v, dtype=np.float64) for v in (lat1, lon1, lat2, lon2))
    return (lat2 - lat1) * RAD, (lon2 - lon1) * RAD, lat1 * RAD, lat2 * RAD


def exact_a_mp(lat1, lon1, lat2, lon2) -> list:
    dlat, dlon, p1, p2 = halves(lat1, lon1, lat2, lon2)
    out = []
    with mpmath.workdps(DPS):
        for a, b, c, d in zip(dlat.tolist(), dlon.tolist(), p1.tolist(), p2.tolist()):
            s1, s2 = mpmath.sin(mpmath.mpf(a) / 2), mpmath.sin(mpmath.mpf(b) / 2)
            out.append(s1 * s1 + mpmath.cos(mpmath.mpf(c)) * mpmath.cos(mpmath.mpf(d)) * (s2 * s2))
    return out


def exact_a_ld(lat1, lon1, lat2, lon2) -> np.ndarray:
    dlat, dlon, p1, p2 = (v.astype(np.longdouble) for v in halves(lat1, lon1, lat2, lon2))
    s1, s2 = np.sin(dlat / 2), np.sin(dlon / 2)
    return s1 * s1 + np.cos(p1) * np.cos(p2) * (s2 * s2)


def unit_mp(lat: float, lon: float):
    """(cos(lat), ux, uy, uz) of geo_of in 50 digits, from fl(lat * RAD), fl(lon * RAD)"""
    with mpmath.workdps(DPS):
        phi, lam = mpmath.mpf(float(np.float64(lat) * RAD)), mpmath.mpf(float(np.float64(lon) * RAD))
        c = mpmath.cos(phi)
        return c, c * mpmath.cos(lam), c * mpmath.sin(lam), mpmath.sin(phi)


def unit_ld(lat, lon):
    phi = (np.asarray(lat, np.float64) * RAD).astype(np.longdouble)
    lam = (np.asarray(lon, np.float64) * RAD).astype(np.longdouble)
    c = np.cos(phi)
    return c, c * np.cos(lam), c * np.sin(lam), np.sin(phi)


def truncation_step(slot_bits: int) -> float:
    """relative error of replacing the low slot_bits of an f64 by a slot: below 2^slot_bits ulps, i.e. 2^-(52 - slot_bits)"""
    return 2.0 ** -(52 - slot_bits)


def _ulps_around(x: float, k: int):
    out = [x]
    lo = hi = x
    for _ in range(k):
        lo, hi = math.nextafter(lo, -math.inf), math.nextafter(hi, math.inf)
        out += [lo, hi]
    return out


def sin_band_points(src: dict) -> list:
    """branch points +-1..4 ulp, the reflection zone, pi_hi +- k ulp (result near 0), zeros, subnormals, a grid"""
    pts = []
    for b in (src["reflect"], src["ocml"], src["pi_hi"], math.pi / 2):
        pts += _ulps_around(b, 4)
    pts += _ulps_around(src["pi_hi"], 64)[::3]
    pts += [0.0, 5e-324, 1e-320, 2.2250738585072009e-308, 2.2250738585072014e-308, 1e-200, 1e-160, 1e-20, 1.4901161193847656e-08]
    pts += np.linspace(0.0, src["ocml"], 2001).tolist()
    pts += np.linspace(src["reflect"], src["ocml"], 501).tolist()  # the reflection zone
    pts += np.geomspace(1e-12, 1.0, 301).tolist()
    rng = np.random.default_rng(11)
    pts += rng.uniform(0.0, src["ocml"], 1000).tolist()
    pts = [p for p in pts if abs(p) <= src["ocml"]]
    pts = sorted(set(pts + [-p for p in pts]), key=lambda v: (abs(v), math.copysign(1.0, v)))
    return pts + [-0.0]  # (a set keeps one of +0 and -0)
