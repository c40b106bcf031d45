"""The carve's distance key, as arithmetic: sin_band emulated operation by operation against mpmath, and the error budget
that makes the carve's certificate sound (protocol_amd/csrc/pm_validate.inc: sin_band, hav_a, prox_a, pack_key;
pm_device.h: PM_A_CHORD_MIN, the slot widths, the bands).  tests/test_gpu_distance_key.py checks the device against the
same emulation and bounds.

Why the budget is band / 4.  The reference orders candidates by d = 6371 * 2 * atan2(sqrt(a), sqrt(1 - a)) from glibc's a
(node_groups/mod.rs:218-231); d is monotone in a, so what matters is the order of a.  The carve orders by a key: the
device's own estimate of a with the low slot_bits of its f64 replaced by the slot.  Write eps_k for the key's relative
error against the exact a (the Haversine term of the reference's f64 intermediates, evaluated exactly) and eps_r for the
same error of glibc's a.  Two candidates i, j can be ordered differently by the key and by the reference only if their
exact terms lie within (eps_k + eps_r) * a of each other on both sides, i.e. within 2 (eps_k + eps_r) a; their keys are
then at most 2 (eps_k + eps_r) a + 2 eps_k a = (4 eps_k + 2 eps_r) a apart.  The certificate demands that
every candidate whose key lies within band * key of the selection's boundary shares the boundary's site; an inversion it
does not see needs keys more than band * a apart.  So with eps_r about 1e-15 (a handful of glibc ulps), the
certificate is sound when

    eps_k <= band / 4.

The truncation of pack_key takes up to 2^-(52 - slot_bits) = band / 8 of that (the bands are 8x the truncation step),
which leaves band / 8 for the error of the form that computed a: the sine form hav_a (about 4e-15 whatever a is) or the
chord form |u1 - u2|^2 / 4, whose error grows like 1/sqrt(a) and is why prox_a only takes it from PM_A_CHORD_MIN up.
That error is measured against the reference's a, whose intermediate fl(fl(lon2 - lon1) * RAD) the chord never
forms: the long way round the antimeridian it rounds by up to ~9e-16 radians, and the chord's error there reaches
1.3e-15 / sqrt(a) (2e-15 asserted) against 6e-16 / sqrt(a) (1e-15 asserted) for longitudes less than 180 degrees apart.

Measured here (mpmath, 50 digits): sin_band's emulation is within MEASURED_SIN_BAND relative of sin on |x| <= 3.2,
against the 1e-15 asserted.
"""
import math

import mpmath
import pytest

from distance_key_model import chord_a, device_constants, fma, sin_band, sin_band_points, sin_band_source, truncation_step

MEASURED_SIN_BAND = 3.3e-16  # max relative error of the emulated sin_band on sin_band_points (measured: 3.27e-16 at -1.5712)
SIN_BAND_BOUND = 1e-15       # asserted: pm_validate.inc's "|rel err| < 1e-15"
CHORD_BOUND = 2e-15          # asserted on the device (tests/test_gpu_distance_key.py): chord form error <= 2e-15 / sqrt(a)
                             # (1e-15 / sqrt(a) where the longitudes lie less than 180 degrees apart)
SINE_FORM_BOUND = 1e-14      # ... and the sine form's, whatever a is


def test_sources_parse():
    src, k = sin_band_source(), device_constants()
    assert len(src["coefs"]) >= 8
    assert 0.0 < k["chord_min"] < k["a_max_safe"] < 1.0
    assert k["rad"] == 3.14159265358979323846 / 180.0


def test_emulated_fma_rounds_once():
    # 1 + 2^-53 + 2^-106 rounds up only when nothing is dropped in between
    assert fma(1.0 + 2.0 ** -52, 1.0 + 2.0 ** -52, -1.0) == 2.0 ** -51 + 2.0 ** -104
    assert fma(2.0 ** -53 + 2.0 ** -105, 1.0, 1.0) == 1.0 + 2.0 ** -52
    assert fma(0.1, 10.0, -1.0) == 5.551115123125783e-17
    assert math.copysign(1.0, fma(-0.0, 1.0, -0.0)) == -1.0 and math.copysign(1.0, fma(2.0, 3.0, -6.0)) == 1.0


def test_sin_band_emulation_against_mpmath():
    """The polynomial and the reflection about the two-piece pi: within 1e-15 relative of sin on |x| <= the OCML
    threshold, odd, and exactly 0 at +-0."""
    src = sin_band_source()
    worst, where = 0.0, None
    with mpmath.workdps(50):
        for x in sin_band_points(src):
            got = sin_band(x, src)
            assert got is not None, x
            want = mpmath.sin(mpmath.mpf(x))
            if want == 0:
                assert got == 0.0, x  # (+0 for -0 too: fma(-0 * z, p, -0) = +0 + -0; it is only ever squared)
                continue
            err = float(abs((mpmath.mpf(got) - want) / want))
            if err > worst:
                worst, where = err, x
            assert sin_band(-x, src) == -got, x
    assert worst <= SIN_BAND_BOUND, (worst, where)
    assert worst <= MEASURED_SIN_BAND * 1.01, f"measured {worst:.3g} at x = {where!r}: update MEASURED_SIN_BAND"


def test_sin_band_covers_every_half_longitude_difference():
    """Half a difference of two longitudes in [-180, 180] is at most fl(360 * RAD) / 2: sin_band must take those through
    the polynomial (the OCML branch is for coordinates outside the reference's range), and reflect from pi / 2 on."""
    src, k = sin_band_source(), device_constants()
    x_max = (180.0 - -180.0) * k["rad"] * 0.5
    assert x_max < src["ocml"]
    assert src["reflect"] == math.pi / 2
    assert src["pi_hi"] == math.pi and abs(mpmath.mpf(src["pi_hi"]) + mpmath.mpf(src["pi_lo"]) - mpmath.pi) < 1e-31


@pytest.mark.parametrize("width", [0, 1, 2])
def test_certificate_budget(width):
    """Each band is 8x its truncation step, and at PM_A_CHORD_MIN — the chord form's worst place — the form's bound plus
    the truncation stays within band / 4 (and the chord bound alone within band / 8).  At 13 bits: 1.75e-12 + 1.82e-12
    <= 3.64e-12.  (PM_A_CHORD_MIN was 6.2e-7: the long way round the antimeridian the chord form measured 1.30e-15 /
    sqrt(a), 1.65e-12 there, and the bound 2e-15 / sqrt(a) gave 2.54e-12 > band / 8.)"""
    k = device_constants()
    sb, band = k["slot_bits"][width], k["bands"][width]
    trunc = truncation_step(sb)
    assert band == 8.0 * trunc, (sb, band)
    chord = CHORD_BOUND / math.sqrt(k["chord_min"])
    assert chord <= band / 8, (chord, band)
    assert chord + trunc <= band / 4, (chord, trunc, band)
    assert SINE_FORM_BOUND + trunc <= band / 4


def test_chord_emulation_is_a_quarter_of_the_squared_chord():
    u1 = (0.6, 0.0, 0.8)
    u2 = (0.0, 0.6, 0.8)
    assert chord_a(u1, u2) == 0.25 * (0.36 + 0.36)
    assert chord_a(u1, u1) == 0.0
