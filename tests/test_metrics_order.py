"""tests/metrics_order.py on the model alone (no GPU): the detector columns detect.  These are conditions on the INPUTS of
tests/test_gpu_metrics_edges.py, not measurements of the engine: every detector series' total changes its bits when the pair it
watches changes places, and a family of them notices each whole-segment order a kernel could fall into — the segment reversed,
rotated by 64 (a tail added first), its 64-blocks exchanged, a pairwise tree."""
import itertools

import pytest

import metrics_model as M
import metrics_order as O

LENGTHS = [3, 4, 5, 63, 64, 65, 127, 128, 129, 193]


def _ledger(n, layout, first_row=10, first_series=7):
    rows = [M.MANUAL] + list(range(first_row, first_row + n - 1))
    per_row, dets = O.family(rows, list(range(first_series, first_series + n - 2)), layout)
    led = M.Ledger()
    led.ingest(*O.batch(per_row), first_series + n)
    return led, dets, per_row


@pytest.mark.parametrize("layout", [O.DENSE, O.TRIANGULAR])
@pytest.mark.parametrize("n", LENGTHS)
def test_every_detector_notices_its_pair(n, layout):
    led, dets, per_row = _ledger(n, layout)
    assert [d.p for d in dets] == list(range(1, n - 1))
    O.check_detectors(led, dets)
    for d in dets:
        assert len(d.values) == (n if layout == O.DENSE else d.p + 2)
        assert M.bits(O.seq_sum(O.exchanged(d.values, d.p))) == M.bits(1.0)
    lens = [len(per_row[r]) for r in per_row]
    assert lens == ([n - 2] * n if layout == O.DENSE else [n - 2] * 3 + list(range(n - 3, 0, -1)))
    # the batch in another row order, and beat by beat, is the same ledger
    other = M.Ledger()
    beats, entries = O.batch(per_row, order=list(per_row)[::-1])
    for b in range(0, n, 16):
        other.ingest(beats[b:b + 16], entries, n + 7)
    assert other.listing() == led.listing() and other.totals() == led.totals()


@pytest.mark.parametrize("n", LENGTHS)
def test_a_family_notices_every_whole_segment_order(n):
    """at least one series of the family changes its total (no single detector can: one whose three places keep their
    relative order through a rotation sums as before)"""
    _, dets, _ = _ledger(n, O.DENSE)
    assert O.family_notices(dets, O.reversed_order)
    if n >= 4:                                             # (three values: the pairwise tree IS the sequential sum)
        assert O.family_notices(dets, list, add=O.tree_sum)
    if n > 64:
        assert O.family_notices(dets, O.rotated)
        assert O.family_notices(dets, O.blocks_exchanged)
    if n % 64 and n > 64:                                  # the tail in front of the whole 64-tiles
        assert O.family_notices(dets, lambda v: v[len(v) // 64 * 64:] + v[:len(v) // 64 * 64])
    assert not O.family_notices(dets, list)                # (and the stated order is the stated order)
    # the triangular layout: every segment has its own length, and the pair is its end
    _, tri, _ = _ledger(n, O.TRIANGULAR)
    assert O.family_notices(tri, O.reversed_order)
    if n > 64:
        assert O.family_notices(tri, O.rotated) and O.family_notices(tri, O.blocks_exchanged)


@pytest.mark.parametrize("n", [3, 4, 5, 6])
def test_a_family_misses_only_the_two_orders_no_sum_can_tell_apart(n):
    """exhaustively: of all n! orders of the segment the family misses the stated one and the one with positions 0 and 1
    exchanged — which commute in any sequential sum from +0.0"""
    _, dets, _ = _ledger(n, O.DENSE)
    missed = [perm for perm in itertools.permutations(range(n))
              if not O.family_notices(dets, lambda v, perm=perm: [v[i] for i in perm])]
    assert missed == [tuple(range(n)), (1, 0) + tuple(range(2, n))]


def test_short_segments_have_no_detector():
    for n in (0, 1, 2):
        per_row, dets = O.family(list(range(n)), [])
        assert per_row == {} and dets == []
    with pytest.raises(AssertionError):
        O.family([3, 2, 5], [0])                           # not in ledger order
    with pytest.raises(AssertionError):
        O.family([2, 3, M.MANUAL], [0])                    # the manual row comes first
