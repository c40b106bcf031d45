"""The metrics ledger's kernels (pm_metrics.inc) past the first tile of each of them, and the ORDER of its sums.
tests/test_gpu_metrics.py holds the ledger to the model at a few hundred rows, three radix chunks and about eight random
doubles a series; here

  - the one-workgroup scan carries its running total across tiles: row offsets of 4095 to 8193 rows, named listings of 4096 to
    8193 rows, histogram matrices of one tile exactly, of two and of three;
  - the radix sort runs over 1 to 33 chunks, two and three passes, on detector families (tests/metrics_order.py): values whose
    total changes its bits if any two neighbours of a segment change places, so a sort that loses stability at one seam or a sum
    that adds its tail first cannot pass;
  - the sum kernel's whole tiles and its tail meet at every segment length around 64, 128 and 192;
  - the liveness hook marks more rows than one workgroup holds, in a table of three scan tiles;
  - the fold's compaction behind a REPLACE drops a different number of slots in each of its sixteen rounds.

Every expected value is tests/metrics_model.py's Ledger, compared bit for bit (Rig, of tests/test_gpu_metrics.py).

Not here: the fourth radix pass (n_series > 2^24).  Its totals arrays alone are 128 MB and the Python model takes minutes over
them, which does not fit a test of a few seconds; the pass loop is the same code as the third."""
import copy

import numpy as np
import pytest

from protocol_amd import engine as E

import liveness_model as LM
import metrics_model as M
import metrics_order as O
from test_gpu_metrics import ERANGE, ON, VALUES, Rig, _beats, _code, _cols, _entries, _listing, _want

pytestmark = pytest.mark.gpu

SCAN_TILE = 4096          # the words of one tile of mx_scan_kernel (pm_metrics.inc), a literal there: `base += 4096u`
CHUNK = E.MX_CHUNK        # the entries of one radix chunk


def _scan_tiles(words):
    return -(-words // SCAN_TILE)


def _ingest_detectors(r, beats, entries, n_series, detectors, tag=""):
    """the conditions on the inputs first, on a model of their own; then the engine"""
    led = copy.deepcopy(r.led)
    led.ingest(beats, entries, n_series)
    O.check_detectors(led, detectors)
    r.ingest(beats, entries, n_series, tag)


def _bits(xs):
    return [M.bits(float(x)) for x in xs]


# ------------------------------------------------------------------------------------------------ the scan's tile carry

def _general(rng, special=0.2):
    """a double of mixed sign over twelve decades; one in five a special one (zeros, infinities, a NaN, a subnormal)"""
    return float(VALUES[int(rng.integers(0, len(VALUES)))]) if rng.random() < special else \
        float(rng.normal() * 10.0 ** int(rng.integers(-6, 7)))


def _names(rng, n, W, occupied):
    """n named rows: half of them rows that hold something, duplicates, the manual row, empty rows, a descending stretch"""
    occ = np.array([w for w in occupied if w != M.MANUAL])
    names = np.where(rng.random(n) < 0.5, rng.choice(occ, size=n), rng.integers(0, W, size=n)).tolist()
    names[n // 4:n // 4 + 600] = sorted(names[n // 4:n // 4 + 600], reverse=True)
    for at in (0, 17, n // 2, SCAN_TILE - 1, n - 1):
        names[at] = M.MANUAL
    names[n - 2], names[SCAN_TILE - 2] = names[3], names[5]
    return [int(x) for x in names]


@pytest.mark.parametrize("R", [SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE + 1])
def test_offsets_copy_and_listings_across_scan_tiles(R):
    """R rows (the manual row and W = R - 1 workers), most of them empty: the scan of the row lengths ends inside its first
    tile, at its end, one word into the second, one word into the third.  Internal row i is worker i - 1."""
    W, S = R - 1, 40
    rng = np.random.default_rng(R)
    r = Rig(W)
    edge = [i - 1 for i in (SCAN_TILE - 2, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1) if i - 1 < W]
    occupied = sorted({M.MANUAL, W - 1, *edge, *(int(w) for w in rng.choice(W - 1, size=300, replace=False))}, key=O.ledger_key)
    per_row = {row: [(int(s), 0, _general(rng)) for s in rng.choice(S, size=int(rng.integers(1, 6)), replace=False)] for row in occupied}
    order = [occupied[int(i)] for i in rng.permutation(len(occupied))]
    r.ingest(*O.batch(per_row, kind=M.REPLACE, order=order), S, "the first batch")
    assert _scan_tiles(R) == 1 + (R > SCAN_TILE) + (R > 2 * SCAN_TILE) and len(_listing(r.eng)) > 600
    r.check_totals("the first batch")

    # the second batch: both sides of every tile boundary take a beat of each kind, a row is emptied, an empty row filled;
    # every other row is the copy kernel's
    sides = sorted({i - 1 for b in range(SCAN_TILE, R, SCAN_TILE) for i in (b - 1, b)} | {W - 2, W - 1})
    held = [w for w in occupied if w not in sides and w != M.MANUAL]
    gone = held[len(held) // 2]
    fresh = next(w for w in range(SCAN_TILE // 2, W) if w not in occupied and w not in sides)
    beats, entries = [], []

    def beat(row, kind, ents):
        beats.append((row, kind, len(entries), len(ents)))
        entries.extend(ents)

    # (a row's beats lie apart in the batch, the rows in a seeded order: the host puts them side by side, stably)
    for w in rng.permutation(sides).tolist():
        beat(w, M.REPLACE, [(1, 0, _general(rng)), (38, 1, _general(rng)), (7, 0, _general(rng))])
    beat(gone, M.DELETE, [(s, 0, 0.0) for s in r.led.rows[gone]] + [(39, 0, 0.0)])
    for w in rng.permutation(sides).tolist():
        beat(w, M.MERGE, [(38, 1, 2.5), (0, 0, _general(rng)), (39, 0, -0.0)])
    beat(fresh, M.MERGE, [(5, 0, 1.0), (3, 0, _general(rng)), (39, 1, 4.0)])
    for w in rng.permutation(sides).tolist():
        beat(w, M.DELETE, [(7, 0, 0.0), (20, 0, 0.0)])
    r.ingest(beats, entries, S, "the second batch")
    assert gone not in {row for row, _, _ in _listing(r.eng)} and len(_listing(r.eng, [fresh])) == 3
    r.check_totals("the second batch")
    r.ingest([(7, M.MERGE, 0, 1)], [(11, 0, 0.75)], S, "a one-row ingest")
    r.check_totals("a one-row ingest")

    # named listings: the scan over the named rows' lengths
    now = [row for row in r.led.order()]
    for n in (SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE + 1):
        names = _names(rng, n, W, now)
        want = _want(r.led, names)
        assert len(names) == n and len(want) > n // 2 and any(not r.led.rows.get(w) for w in names)
        assert _listing(r.eng, names) == want, n

    # an upload that drops the row identities: the manual row stays, every worker row is empty, an ingest afterwards is right
    manual = _want(r.led, [M.MANUAL])
    r.eng.upload_workers(_cols(W))
    r.led.clear_workers()
    assert _listing(r.eng) == manual == _want(r.led) and manual
    r.check_totals("after the upload")
    back = {row: [(int(s), 0, _general(rng)) for s in rng.choice(S, size=3, replace=False)] for row in [0, M.MANUAL, W - 1] + sides}
    r.ingest(*O.batch(back), S, "after the upload")
    r.check_totals("an ingest after the upload")
    names = _names(rng, SCAN_TILE + 1, W, r.led.order())
    assert _listing(r.eng, names) == _want(r.led, names)
    r.close()


# ------------------------------------------------------------------------------------------------ the sort's seams

def _family_size(n, layout):
    return n * (n - 2) if layout == O.DENSE else (n - 2) * (n + 3) // 2


def _sort_case(N, layout, n_series, detector_ids, seed):
    """A ledger of exactly N entries: one detector family over the manual row and n - 1 workers, as large as fits under N with
    room for forty fillers, and plain fillers (small dyadic values on series of their own) on every row, the family's included.
    -> (W, per_row, detectors)"""
    rng = np.random.default_rng(seed)
    n = 3
    while _family_size(n + 1, layout) <= N - 40:
        n += 1
    ids = detector_ids(n - 2)
    assert len(set(ids)) == n - 2 and max(ids) < n_series
    ids = [ids[int(i)] for i in rng.permutation(n - 2)]
    rows = [M.MANUAL] + [3 + i + i // 7 for i in range(n - 1)]
    W = rows[-1] + 9
    per_row, dets = O.family(rows, ids, layout)
    everyone = [M.MANUAL] + list(range(W))
    free = [0, n_series - 1] + [int(s) for s in rng.permutation(n_series)[:64]]
    free = [s for i, s in enumerate(free) if s not in set(ids) and s not in free[:i]]
    n_fill = N - _family_size(n, layout)
    assert 40 <= n_fill <= len(everyone) * len(free)
    everyone = [everyone[int(i)] for i in rng.permutation(len(everyone))]
    fill = {}
    for k in range(n_fill):                                               # (a row takes a filler series once)
        fill.setdefault(everyone[k % len(everyone)], []).append((free[k // len(everyone)], 0, float(k % 17 - 8) + 0.5))
    return W, [per_row, fill], dets


def _two_pass_ids(k):
    """k consecutive series around 512: 64 neighbours in a row have 64 different low digits, and one of two high digits"""
    return list(range(512 - k // 2, 512 - k // 2 + k))


def _three_pass_ids(k):
    """both sides of 255 | 256 and of 65535 | 65536"""
    a = k // 2
    return list(range(256 - a // 2, 256 - a // 2 + a)) + list(range(65537 - (k - a), 65537))


def _sort_test(N, layout, n_series, detector_ids, tiles):
    W, parts, dets = _sort_case(N, layout, n_series, detector_ids, N)
    beats, entries = O.batch(*parts)
    chunks = -(-N // CHUNK)
    assert len(entries) == N and _scan_tiles(256 * chunks) == tiles
    r = Rig(W)
    _ingest_detectors(r, beats, entries, n_series, dets)
    r.check_totals()
    first = r.totals()
    assert sum(first[1]) == N and len(first[0]) == n_series
    assert r.totals() == first
    # a second engine, the same ledger in another split: two halves with their rows the other way round, then three dozen rows
    # one ingest each, so that the table is rebuilt (and every entry copied) many times
    other = Rig(W)
    rows = [b[0] for b in beats]
    singles = rows[::max(len(rows) // 36, 1)][:36]
    rest = [row for row in rows if row not in singles][::-1]
    for part in (rest[:len(rest) // 2], rest[len(rest) // 2:], *[[row] for row in singles]):
        b, e = O.batch(*parts, order=part)
        other.eng.metrics_ingest(_beats(b), _entries(e), n_series)
    assert len(singles) >= 30 and _listing(other.eng) == _want(r.led)
    assert other.totals() == first
    other.close()
    r.close()


@pytest.mark.parametrize("layout", [O.DENSE, O.TRIANGULAR])
@pytest.mark.parametrize("N,tiles", [(CHUNK - 1, 1), (CHUNK, 1), (CHUNK + 1, 1), (16 * CHUNK, 1), (16 * CHUNK + 1, 2), (32 * CHUNK + 1, 3)])
def test_two_radix_passes_at_the_chunk_and_histogram_tile_edges(N, tiles, layout):
    """N entries: one chunk less one, one chunk, one more; sixteen chunks — a histogram matrix of 4096 words, one scan tile
    exactly; seventeen — one carry; thirty-three — two.  Sums and counts are the model's bits, and those of another engine"""
    _sort_test(N, layout, 1000, _two_pass_ids, tiles)


@pytest.mark.parametrize("layout", [O.DENSE, O.TRIANGULAR])
def test_one_radix_pass_keeps_the_row_order(layout):
    """n_series = 256: a scatter that lost its stability would still sort — only the order of the addends could show it"""
    _sort_test(2 * CHUNK + 1, layout, 256, lambda k: list(range(100, 100 + k)), 1)


@pytest.mark.parametrize("layout", [O.DENSE, O.TRIANGULAR])
def test_three_radix_passes_over_seventeen_chunks(layout):
    _sort_test(16 * CHUNK + 1, layout, 65537, _three_pass_ids, 2)


# ------------------------------------------------------------------------------------------------ the sum's tiles and tail

def test_sum_tiles_and_tail_at_every_segment_length():
    """one dense family per segment length, each over its own rows: every pair of neighbours of every segment has its detector,
    the pairs across the 64-entry seams of mx_sum_kernel — (63, 64), (64, 65), (127, 128), (128, 129) — among them.  A series
    nobody holds lies between the two longest families; series 0 and the last one are held"""
    lengths = [193, 129, 63, 64, 65, 127, 128, 2, 1]
    parts, dets, series_of = [], [], {}
    row0, ser0, nobody = 0, 0, None
    for n in lengths:
        rows = ([M.MANUAL] if n == 193 else []) + list(range(row0, row0 + n - (n == 193)))
        row0 = rows[-1] + 3
        if n >= 3:
            ids = list(range(ser0, ser0 + n - 2))
            per_row, d = O.family(rows, ids)
            parts.append(per_row)
            dets += d
        else:                                                         # (too short for a pair: plain values)
            ids = [ser0]
            parts.append({row: [(ser0, 0, 1.5 + k)] for k, row in enumerate(rows)})
        series_of[n] = ids
        ser0 = ids[-1] + 1
        if n == 193:
            nobody, ser0 = ser0, ser0 + 1
    S, W = ser0, row0
    assert series_of[193][0] == 0 and series_of[1] == [S - 1] and series_of[193][-1] < nobody < series_of[129][0]
    for p in (63, 64, 127, 128):
        assert any(d.p == p and len(d.values) == 193 for d in dets)
    r = Rig(W)
    beats, entries = O.batch(*parts)
    _ingest_detectors(r, beats, entries, S, dets)
    r.check_totals()
    s, c = r.eng.metrics_totals()
    for n in lengths:
        assert [int(c[i]) for i in series_of[n]] == [n] * len(series_of[n]), n
    assert int(c[nobody]) == 0 and M.bits(float(s[nobody])) == M.bits(0.0)       # +0.0, not -0.0
    assert int(c.sum()) == len(entries)
    r.close()


# ------------------------------------------------------------------------------------------------ the liveness hook

def test_a_sweep_empties_dead_rows_across_workgroups_and_scan_tiles():
    """W = 8192 (three scan tiles of row lengths), every third worker holds metrics, 650 rows fall silent: the transition list and
    mx_mark_dead_kernel's grid are three workgroups long.  Then rows that hold nothing die: the table stays as it is"""
    rng = np.random.default_rng(5)
    W, S = 2 * SCAN_TILE, 12
    flags = np.full(W, ON, dtype=np.uint32)
    eng = E.Engine()
    eng.upload_workers(_cols(W))
    eng.liveness_enable(True, 1)
    eng.metrics_enable(True)
    led = M.Ledger()
    per_row = {row: [(int(s), 0, _general(rng, special=0.0)) for s in rng.choice(S, size=int(rng.integers(1, 5)), replace=False)]
               for row in [M.MANUAL] + list(range(0, W, 3))}
    beats, entries = O.batch(per_row, kind=M.REPLACE)
    eng.metrics_ingest(_beats(beats), _entries(entries), S)
    led.ingest(beats, entries, S)
    must = [SCAN_TILE - 3, SCAN_TILE - 2, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, W - 1, 0]   # (workers and internal rows 4094 .. 4097)
    silent = np.array(sorted(set(must) | {int(w) for w in rng.choice(W, size=640, replace=False)}))
    assert len(silent) >= 600 and any(w % 3 == 0 for w in must) and any(w % 3 for w in must)
    live = LM.Ledger(flags, 1)
    now = 1_760_000_000_000

    def totals():
        s, c = eng.metrics_totals()
        return _bits(s), c.tolist()

    def sweep(silent_rows, apply):
        nonlocal now
        now += 15_000
        last = np.full(W, now - 1000, dtype=np.uint64)
        last[silent_rows] = now - 200_000
        want_rows, want_census = live.sweep(now, last)
        n, census = eng.liveness_sweep(now, last, None, apply=apply)
        assert n == len(want_rows) and census.tolist() == want_census
        got = eng.liveness_transitions()
        assert [(int(a), int(b)) for a, b in zip(got["worker"], got["new_status"])] == [(w, new) for w, _, new, _ in want_rows]
        return [w for w, _, new, _ in want_rows if new == LM.DEAD]

    total_dead = 0
    for k in range(3):                                                  # Healthy -> Unhealthy -> Dead -> Dead
        dead = sweep(silent, apply=(k == 1))
        total_dead += len(dead)
        for w in dead:
            led.clear_row(w)
        assert _listing(eng) == _want(led), k
        ws, wc = led.totals()
        assert totals() == (_bits(ws), wc), k
    assert total_dead == len(silent) > 512
    # rows that hold nothing fall silent and die: nothing to rebuild, the totals still served, the listing as it was
    before, served = _listing(eng), totals()
    was_silent = set(silent.tolist())
    empty = np.array([w for w in list(range(1, W, 3))[:300] + [SCAN_TILE + 3, W - 3] if w not in was_silent])
    assert len(empty) > 256 and all(w % 3 and not led.rows.get(int(w)) for w in empty.tolist())
    both = np.concatenate([silent, empty])
    assert sweep(both, apply=False) == []
    assert _listing(eng) == before and totals() == served
    assert sorted(sweep(both, apply=True)) == sorted(int(w) for w in set(empty.tolist()))
    assert _listing(eng) == before == _want(led) and totals() == served
    eng.metrics_ingest(_beats([(int(empty[0]), M.MERGE, 0, 1)]), _entries([(0, 0, 2.0)]), S)
    led.ingest([(int(empty[0]), M.MERGE, 0, 1)], [(0, 0, 2.0)], S)
    assert _listing(eng) == _want(led)
    eng.close()


# ------------------------------------------------------------------------------------------------ the fold's compaction

def _class_value(series, place):
    """the three rows' values of a series: (2^53, 1, -2^53) turned by series % 3, so a value in another series' slot shows"""
    return (O.BIG, 1.0, -O.BIG)[(place + series) % 3]


def test_a_replace_compacts_a_full_row_over_sixteen_uneven_rounds():
    """three rows of PM_MX_ROW_MAX series; a REPLACE keeps an irregular third of one of them — each 64-slot round of the
    compaction drops a different number — and adds new series up to exactly the bound; the same batch with one series more, on
    the next row, is refused"""
    rng = np.random.default_rng(64)
    R = E.MX_ROW_MAX
    assert R == M.ROW_MAX and R % 64 == 0
    rounds = R // 64
    r = Rig(8)
    A, B = 3, 5
    places = {M.MANUAL: 0, A: 1, B: 2}
    keep_counts = [int(x) for x in rng.permutation(np.arange(14, 14 + rounds))]
    kept = sorted(int(64 * k + j) for k, n in enumerate(keep_counts) for j in rng.choice(64, size=n, replace=False))
    assert len({64 - n for n in keep_counts}) == rounds and abs(len(kept) - R / 3) < R / 50
    new = list(range(R, R + R - len(kept)))
    S = new[-1] + 2
    r.ingest(*O.batch({row: [(s, 0, _class_value(s, place)) for s in range(R)] for row, place in places.items()}), S, "three full rows")
    r.check_totals("three full rows")
    sums = r.led.totals()[0]
    assert {M.bits(x) for x in sums[:R]} == {M.bits(0.0), M.bits(1.0)}
    # a kept series: every other one keeps its old value (PM_MXF_MAX against -inf), the others take the next class's
    ents = [(s, M.F_MAX, float("-inf")) if i & 1 else (s, 0, _class_value(s + 1, 1)) for i, s in enumerate(kept)]
    ents += [(s, 0, float(s) + 0.25) for s in new]
    ents = [ents[int(i)] for i in rng.permutation(len(ents))]
    r.ingest([(A, M.REPLACE, 0, len(ents))], ents, S, "the replace")
    got = _listing(r.eng, [A])
    assert len(got) == R and [s for _, s, _ in got] == kept + new
    r.check_totals("the replace")
    before, totals = _listing(r.eng), r.totals()
    # one series too many, on the next row: refused, nothing changes
    over = ents + [(S - 1, 0, 9.0)]
    assert _code(lambda: r.eng.metrics_ingest(_beats([(B, M.REPLACE, 0, len(over))]), _entries(over), S)) == ERANGE
    with pytest.raises(M.Refused):
        r.led.ingest([(B, M.REPLACE, 0, len(over))], over, S)
    assert _listing(r.eng) == before == _want(r.led) and r.totals() == totals
    # and the batch that fits, on that row too, its slots shuffled first by a DELETE and a MERGE in front of the REPLACE
    moved = [kept[0], kept[7], 100, kept[-1], 1000]
    batch = [(s, 0, 0.0) for s in moved] + [(s, 0, r.led.rows[B][s]) for s in moved[::-1]] + ents
    r.ingest([(B, M.DELETE, 0, 5), (B, M.MERGE, 5, 5), (B, M.REPLACE, 10, len(ents))], batch, S, "the second row")
    assert len(_listing(r.eng, [B])) == R
    r.check_totals("the second row")
    r.close()
