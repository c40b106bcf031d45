"""Order detectors for the metrics ledger's totals: value columns whose sequential sum changes its BITS when two neighbouring
addends change places.  No GPU, no numpy.

pm_metrics_totals adds a series' values one by one from +0.0 in ascending row order, the manual row first
(tests/metrics_model.py, Ledger.totals).  Random doubles notice a wrong order only by luck.  A detector notices it
by construction: for a series whose segment holds n entries, the detector of the pair of positions (p, p + 1), 1 <= p, is

    position 0: 2^53     position p: 1.0     position p + 1: -2^53     every other position: +0.0

In order the 1.0 is rounded away (2^53 + 1 is a tie, and 2^53 is the even neighbour) and -2^53 cancels the rest: +0.0.  Of the
six relative orders of the three positions only (0, p, p + 1) and (p, 0, p + 1) give +0.0; the other four give 1.0 (2^53 - 1
is a double, so nothing is rounded away once -2^53 came before 2^53 or the 1.0 met -2^53 alone).  So detector p misses an
order only if position p + 1 comes behind both position 0 and position p — and an order of the whole segment that ALL the
detectors p = 1 .. n - 2 miss keeps 1 < 2 < ... < n - 1 and has position 0 in front of position 2: the stated order, or the one
with positions 0 and 1 exchanged, which no sequential sum from +0.0 can tell from it.  A family of detector series, one per p,
held by the same rows, therefore turns "some reordering somewhere in the segment" into a wrong total in at least one series.

Two layouts of a family over the rows r_0 < r_1 < ... < r_(n-1) (ledger order):
  DENSE       every row holds every detector series: every segment is n long.
  TRIANGULAR  row r_q holds detector p only if q <= p + 1 (the zeros behind the pair are left out): the segment of detector p
              is p + 2 long, the rows' lengths fall from n - 2 to 1.
"""
import metrics_model as M

BIG = 2.0 ** 53
DENSE, TRIANGULAR = "dense", "triangular"


def ledger_key(row):
    """the ledger's row order: the manual row first, then ascending worker"""
    return (row + 1) & 0xFFFFFFFF


def column(n, p):
    """the detector of the pair (p, p + 1) in a segment of n entries"""
    assert 1 <= p and p + 1 < n
    col = [0.0] * n
    col[0], col[p], col[p + 1] = BIG, 1.0, -BIG
    return col


def seq_sum(values):
    """the ledger's sum: from +0.0, one value after the other"""
    acc = 0.0
    for v in values:
        acc += v
    return acc


def tree_sum(values):
    """a pairwise tree: neighbours first, then neighbouring pairs, ... (what a reduction over lanes would do)"""
    level = list(values) or [0.0]
    while len(level) > 1:
        level = [level[i] + level[i + 1] if i + 1 < len(level) else level[i] for i in range(0, len(level), 2)]
    return 0.0 + level[0]


def exchanged(values, p):
    out = list(values)
    out[p], out[p + 1] = out[p + 1], out[p]
    return out


def reversed_order(values):
    return list(values)[::-1]


def rotated(values, k=64):
    k %= max(len(values), 1)
    return list(values[k:]) + list(values[:k])


def blocks_exchanged(values, k=64):
    """the first two k-blocks change places (the second one may be short)"""
    return list(values[k:2 * k]) + list(values[:k]) + list(values[2 * k:])


class Detector:
    """one detector series: `series` is held by `rows` (ledger order) with the values `values`; the pair is (p, p + 1)"""

    def __init__(self, series, rows, p):
        self.series, self.rows, self.p = series, list(rows), p
        self.values = column(len(self.rows), p)


def family(rows, series, layout=DENSE):
    """Detectors for every pair (p, p + 1), 1 <= p <= n - 2, of a segment over `rows` (n of them, in ledger order); detector p
    takes series[p - 1].  Fewer than three rows have no pair to detect: no detector, nothing held.
    -> (per_row {row: [(series, flags, value)]}, [Detector])"""
    rows = list(rows)
    n = len(rows)
    assert all(ledger_key(a) < ledger_key(b) for a, b in zip(rows, rows[1:])), "rows in ledger order, each once"
    assert len(series) == max(n - 2, 0) and len(set(series)) == len(series)
    assert layout in (DENSE, TRIANGULAR)
    detectors = []
    per_row = {r: [] for r in rows} if n >= 3 else {}
    for p in range(1, n - 1):
        held = rows if layout == DENSE else rows[:p + 2]
        d = Detector(series[p - 1], held, p)
        detectors.append(d)
        for r, v in zip(held, d.values):
            per_row[r].append((d.series, 0, v))
    return per_row, detectors


def batch(*parts, kind=M.MERGE, order=None):
    """{row: [(series, flags, value)]} dicts laid side by side -> (beats, entries) for Ledger.ingest and Rig.ingest: one beat a
    row, the rows in `order` (default: as they come).  A row's entries keep the order of the parts."""
    per_row = {}
    for part in parts:
        for r, ents in part.items():
            per_row.setdefault(r, []).extend(ents)
    beats, entries = [], []
    for r in (order if order is not None else per_row):
        beats.append((r, kind, len(entries), len(per_row[r])))
        entries += per_row[r]
    return beats, entries


def held_column(led, series):
    """the values of `series` in the model's ledger, in the order of the sums"""
    return [led.rows[r][series] for r in led.order() if series in led.rows[r]]


def check_detectors(led, detectors):
    """What makes a detector one, asserted on the model: the ledger holds the column as designed, its total is the model's
    total, and the total of the same values with positions p and p + 1 exchanged differs from it in bits.  A detector that does
    not detect is a bug of the test."""
    sums, counts = led.totals()
    for d in detectors:
        col = held_column(led, d.series)
        assert [M.bits(v) for v in col] == [M.bits(v) for v in d.values], d.series
        assert [r for r in led.order() if d.series in led.rows[r]] == d.rows, d.series
        assert counts[d.series] == len(col) and M.bits(sums[d.series]) == M.bits(seq_sum(col)) == M.bits(0.0), d.series
        assert M.bits(seq_sum(exchanged(col, d.p))) != M.bits(sums[d.series]), (d.series, d.p)


def family_notices(detectors, reorder, add=seq_sum):
    """does at least one detector's total change its bits when every segment is put through `reorder` and added with `add`?"""
    return any(M.bits(add(reorder(d.values))) != M.bits(seq_sum(d.values)) for d in detectors)
