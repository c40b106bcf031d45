"""The key families of tests/near_row_cases.py on the CPU: the stride-by-stride model of tests/test_near_row_model.py (the
algorithm of near_row_offer on Python integers) gives what the set-wise reference says a row is, whatever order the keys come
in — and the families reach what they were written to reach.  The second half are conditions on the generators, checked on the
reference alone: a family that stopped producing near misses, or both outcomes of a certificate, would let
tests/test_gpu_row_certificates.py pass without looking.  If one falls short, change the generator, not the bound."""
import numpy as np
import pytest

import near_row_cases as C
from protocol_amd import engine as E
from test_near_row_model import NearRow

GEOMS = list(C.GEOMETRIES)
MODEL_WAVES = 2        # waves per case through the Python model (it is slow; the reference sees every wave)
NEAR_MISS_FAMILIES = ("busy", "floor", "straddle", "noloc_some", "one_site")

_cache = {}


def cases(gname, family):
    """the family's cases with their reference and flags, made once"""
    if (gname, family) not in _cache:
        out = []
        for c in C.FAMILIES[family](C.GEOMETRIES[gname]):
            ref = C.Reference(c.keys, c.sites, c.geom)
            out.append((c, ref, ref.flags()))
        _cache[gname, family] = out
    return _cache[gname, family]


def _model(keys, sites, g):
    """one wave's keys, in this order, through the stride model"""
    row = NearRow(g.sb, g.ulps)
    ks = [int(k) for k in keys]
    ks += [C.EMPTY] * (-len(ks) % 64)
    site_of = lambda slot: int(sites[slot])
    for b in range(0, len(ks), 64):
        st = ks[b:b + 64]
        row.offer(st, [site_of(k & g.mask) if k != C.EMPTY else 0 for k in st], site_of)
    return row


@pytest.mark.parametrize("family", list(C.FAMILIES))
@pytest.mark.parametrize("gname", GEOMS)
def test_the_stride_model_gives_the_reference_in_any_order(gname, family):
    g = C.GEOMETRIES[gname]
    for c, ref, _ in cases(gname, family):
        X = ref.probe_sites()
        want = ref.answer(X)
        rng = np.random.default_rng(len(c.name))
        for w in range(0, c.keys.shape[0], max(1, c.keys.shape[0] // MODEL_WAVES))[:MODEL_WAVES]:
            for perm in range(3):
                keys = c.keys[w] if perm == 0 else c.keys[w][rng.permutation(c.keys.shape[1])]
                row = _model(keys, c.sites, g)
                assert row.key == [int(k) for k in ref.row[w]], (c.name, w, perm)
                assert (row.tau, row.tau_hi) == (int(ref.tau[w]), int(ref.tau_hi[w])), (c.name, w, perm)
                for x, a in zip(X[w], want[w]):
                    got = row.m1 if row.s1 != int(x) else row.m2
                    assert (got if got < row.tau_hi else C.EMPTY) == int(a), (c.name, w, perm, int(x))


@pytest.mark.parametrize("gname", GEOMS)
def test_every_wave_of_the_busy_families_has_a_near_miss_whose_answer_depends_on_the_site(gname):
    todo = [(f, c, ref) for f in NEAR_MISS_FAMILIES for c, ref, _ in cases(gname, f)]
    todo += [("lengths", c, ref) for c, ref, _ in cases(gname, "lengths") if c.meta["n"] >= 65 and c.meta["holes"] == 0.0]
    assert len(todo) == len(NEAR_MISS_FAMILIES) + sum(1 for n in C.LENGTHS if n >= 65)
    for f, c, ref in todo:
        assert ref.in_window.any(axis=1).all(), c.name
        a = ref.answer(ref.probe_sites())
        assert (a != a[:, :1]).any(axis=1).all(), c.name


@pytest.mark.parametrize("gname", GEOMS)
def test_levels_decide_the_tail_both_ways(gname):
    got = cases(gname, "levels")
    assert len(got) == len(C.LEVEL_CENTRES) == 4
    j = [k - 1 for k in C.EDGE_KS]
    for c, ref, (_, _, f) in got:
        assert c.keys.shape[0] == C.LEVEL_SEEDS == 40
        ok, decided, clear = f["tail_ok"][:, j], f["decided"][:, j], f["tail_clear"][:, j]
        counts = (int(ok.sum()), int((decided & ~ok).sum()), int(clear.sum()))
        assert counts[0] >= 100 and counts[1] >= 30 and counts[2] >= 5, (c.name, counts)


@pytest.mark.parametrize("gname", GEOMS)
def test_the_flag_bits_take_their_values(gname):
    clean, safe, j_tails = set(), set(), set()
    for family in C.FAMILIES:
        for c, ref, (word, mine, f) in cases(gname, family):
            clean |= set(np.unique(f["clean"]).tolist())
            safe |= set(np.unique(f["safe"]).tolist())
            j_tails |= set(np.unique(f["j_tail"][f["j_tail"] < f["n_k"]]).tolist())
            # the word is its fields
            assert np.array_equal(word & 0xFF, f["n_k"]) and np.array_equal((word >> 8) & 0xFF, f["j_tail"])
            assert np.array_equal((word & E.ROW_TAIL_OK) != 0, f["tail_ok"]) and not (f["tail_ok"] & f["tail_clear"]).any()
            # complete: exactly where the wave holds fewer keys than the row may list
            assert np.array_equal(f["complete"], ref.n_all[:, None] < C.KS[None, :])
            if family == "lengths":
                n = c.meta["n"]
                if n >= 255:
                    assert not f["complete"].any(), c.name
                if n <= 65 and c.meta["holes"]:
                    assert f["complete"].any(), c.name
                if n < 64 and not c.meta["holes"]:
                    assert f["complete"][:, n:].all() and not f["complete"][:, :n].any()
    assert clean == {True, False} and safe == {True, False} and len(j_tails) >= 3
    # the antipode family has the bound itself and a step either side of it among the listed values
    for c, ref, (_, _, f) in cases(gname, "antipode"):
        a_max = ref.a[:, :64].max(axis=1, where=ref.loc[:, :64], initial=0.0)
        assert (a_max > E.A_MAX_SAFE).any() and (a_max == E.A_MAX_SAFE).any() and ((a_max < E.A_MAX_SAFE) & (a_max > 0.999)).any()
        assert np.array_equal(f["safe"][:, -1], a_max <= E.A_MAX_SAFE)


@pytest.mark.parametrize("gname", GEOMS)
def test_the_edges_of_the_band_are_met_exactly(gname):
    g = C.GEOMETRIES[gname]
    (c, ref, (_, _, f)), = cases(gname, "edge_of_band")
    seen = set()
    for w, (kind, d, K) in enumerate(c.meta["plan"]):
        a_last = ref.a[w, K - 1]
        if kind == 0:      # the first unlisted key against `a_b - a_last <= a_b * 4 band + 1e-300`
            a_b = ref.a[w, K]
            assert a_b >= 1e-270 and (a_b - a_last == a_b * (4.0 * g.band)) == (d == 0)
            assert f["tail_clear"][w, K - 1] == (d > 0) and f["decided"][w, K - 1] == (d <= 0)
        else:              # a key at another site against `a - a_last <= a_last * 4 band + 1e-300`
            at = np.nonzero(ref.site[w] == 1)[0]
            at = at[at >= K][0]
            a = ref.a[w, at]
            assert f["decided"][w, K - 1] and (a - a_last == a_last * (4.0 * g.band)) == (d == 0)
            assert f["tail_ok"][w, K - 1] == (d > 0)
            seen.add((d, bool(at >= 64)))        # in the row's lanes, or left to the tracker
    assert seen == {(d, t) for d in (-1, 0, 1) for t in (False, True)}


@pytest.mark.parametrize("gname", GEOMS)
def test_the_entrant_schedule_gives_each_call_its_count(gname):
    got = cases(gname, "entrants")
    assert [c.meta["layout"] for c, _, _ in got] == list(C.LAYOUTS)
    s, p = E.NET_SERIAL_MAX, E.NET_PACK_KEYS
    assert C.ENTRANTS == (0, 1, s - 1, s, s + 1, 63, 64, 65, p - 1, p, p + 1, 255, 256)
    for c, ref, _ in got:
        n_ent = ref.entrants_per_call(c.keys)
        assert np.array_equal(n_ent, np.broadcast_to(np.array((256,) + C.ENTRANTS), n_ent.shape)), c.name
        assert c.uptos == (256, 300, 1 << 30)
