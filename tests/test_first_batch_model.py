"""The swarm families of tests/first_batch_cases.py reach what they exist for — by the references and the model walk alone,
before any GPU time is spent on them (tests/test_gpu_first_batch.py asserts the same again in front of every formation): the list
lengths and the seam offsets of the slot loc bitmap's two-word OR, the seed cap met, one below and one above, walks that stop in
front of ring 2, ring 3 and later ones, a drain in mid-run and a run of more than 256 entries, clipped runs, index entries of
another configuration inside the visited rings, and the run-outs."""
import numpy as np
import pytest

import first_batch_cases as F


@pytest.mark.parametrize("gi", F.all_members(), ids=F.member_id)
def test_family_reaches_what_it_exists_for(gi):
    fam = F.family(gi[0])[gi[1]]
    by_mode = F.reaches(fam)
    for mode, L in by_mode.items():
        assert len(F.sample(fam, L)) >= min(L.n_seeds, 48 if fam.n_drawn >= 32 else 18)


def test_bitmap_and_gaps():
    b = np.zeros(130, dtype=bool)
    b[[0, 63, 64, 129]] = True
    assert F.bitmap(b).tolist() == [1 | 1 << 63, 1, 2]
    c = F._with_gaps(200, F.SEAM_GAPS)
    assert c.sum() == 200 and len(c) == 265 and not c[1:64].any() and c[64]


def test_the_seed_cap_rule():
    """prop_limit_scan on three hand-made lists: all below the cap, the cap met at a word's end, the cap inside a word"""
    for n_loc, want_limit, want_seeds in ((511, 511, 511), (512, 512, 512), (513, 512, 512), (600, 512, 512)):
        rng = np.random.default_rng(n_loc)
        lat, lon = F._scatter(rng, n_loc)
        L = F.lists(F.swarm(lat, lon, np.ones(n_loc, dtype=bool), F.CFG_ONE), 0)
        assert (L.limit, L.n_seeds, L.prop_k) == (want_limit, want_seeds, 63)
        assert L.seed_slots.tolist() == list(range(want_seeds))
