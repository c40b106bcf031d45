"""Neighbour rows and their certificates on the device against brute force (pm_debug_row_certificates).

Per wave the hook builds three rows from the same keys — stride by stride (near_row_offer), four strides at a time through the
out-of-line networks (near_row_offer_bulk<4>), and through their inline copy, which the streaming carve's sweep runs
(near_row_offer_bulk<4, true>) — and runs near_row_finish on each at every K = 1 .. 63.  Each of the three is held to the
set-wise reference of tests/near_row_cases.py: the 64 keys, tau, tau_hi, what the near-miss tracker answers for every site the
last entry could sit at (cut at tau_hi: the raw m1 / m2 / s1 may differ between the rows beyond the final window), and the flags
word and the lanes' entries at every K.  Whole arrays; on a mismatch the first five (wave, K, got, want) are printed and the
assertion names the word that is wrong.  tests/test_near_row_cases.py (CPU) holds the families to what they have to reach."""
import numpy as np
import pytest

import near_row_cases as C
from protocol_amd import engine as E

pytestmark = pytest.mark.gpu

ROWS = ("insertion", "networks", "networks-inline")
FIELDS = (("n_k", 0xFF), ("j_tail", 0xFF00), ("SAFE", E.ROW_SAFE), ("TAIL_CLEAR", E.ROW_TAIL_CLEAR), ("CLEAN", E.ROW_CLEAN),
          ("TAIL_OK", E.ROW_TAIL_OK), ("COMPLETE", E.ROW_COMPLETE))


@pytest.fixture(scope="module")
def eng():
    e = E.Engine()
    yield e
    e.close()


def _report(what, got, want, per_k=False):
    """'' if equal, else the name of what differs; prints the first five places: (wave, [K | site asked for], [lane]), got, want"""
    bad = np.argwhere(got != want)
    if not len(bad):
        return ""
    print(f"{what}: {len(bad)} differ:")
    for at in bad[:5]:
        at = tuple(int(i) for i in at)
        where = (at[0], at[1] + 1) + at[2:] if per_k else at
        print("   ", where, hex(int(got[at])), hex(int(want[at])))
    return what


def _compare(c, upto, out, ref, X, answers, word, mine):
    wrong = []
    tag = f"{c.geom.name}/{c.name}/upto={upto}"
    if out["mismatch"] != (0, 0):
        print(f"{tag}: the device's own comparison of insertion and networks: {out['mismatch']}")
        wrong.append("device-comparison")
    for r, rname in enumerate(ROWS):
        t = f"{tag}/{rname}"
        wrong.append(_report(f"{t}: keys", out["rows"][:, r], ref.row))
        wrong.append(_report(f"{t}: tau", out["tau"][:, r], ref.tau))
        wrong.append(_report(f"{t}: tau_hi", out["tau_hi"][:, r], ref.tau_hi))
        m1, m2, s1, hi = out["m1"][:, r, None], out["m2"][:, r, None], out["s1"][:, r, None], out["tau_hi"][:, r, None]
        got = np.where(s1 != X, m1, m2)
        got = np.where(got < hi, got, np.uint64(C.EMPTY))
        wrong.append(_report(f"{t}: tracker answer (s1 != X ? m1 : m2)", got, answers))
        flags = out["flags"][:, r]
        if not np.array_equal(flags, word):
            names = [n for n, bit in FIELDS if ((flags ^ word) & bit).any()]
            wrong.append(_report(f"{t}: flags [{', '.join(names)}]", flags, word, per_k=True))
        wrong.append(_report(f"{t}: mine", out["mine"][:, r], mine, per_k=True))
    return [w for w in wrong if w]


@pytest.mark.parametrize("family", list(C.FAMILIES))
@pytest.mark.parametrize("gname", list(C.GEOMETRIES))
def test_three_rows_and_their_certificates_equal_brute_force(eng, gname, family):
    g = C.GEOMETRIES[gname]
    wrong = []
    for c in C.FAMILIES[family](g):
        W, N = c.keys.shape
        assert 32 <= W <= 96 and W % 4 == 0
        ref = C.Reference(c.keys, c.sites, g)
        X = ref.probe_sites()
        answers = ref.answer(X)
        word, mine, _ = ref.flags()
        for upto in c.uptos:
            out = eng.debug_row_certificates(c.keys, c.sites, N, g.sb, g.ulps, min(upto, N + 256), g.band)
            wrong += _compare(c, upto, out, ref, X, answers, word, mine)
    assert not wrong, wrong[:8]
