"""The metrics ledger on the GPU (pm_metrics_* of include/pm_engine.h, kernels in pm_metrics.inc) against the model of
tests/metrics_model.py, which tests/test_metrics_model.py holds to the reference (metrics_store.rs, heartbeat.rs:94-151): every
row and value bit for bit through pm_metrics_rows after every batch; the totals' bits, their bound and their determinism; the
join against pm_get_groups; the liveness hook; every error; what the ledger leaves alone."""
import math

import numpy as np
import pytest

from protocol_amd import engine as E
from protocol_amd import host
from protocol_amd.churn import ChurnStream
from protocol_amd.swarm import make_swarm
from helpers import engine_groups

import liveness_model as LM
import metrics_cases as MC
import metrics_model as M
from test_metrics_model import run_store

pytestmark = pytest.mark.gpu
EINVAL, ESTATE, ERANGE = -1, -4, -5
ON = E.W_HEALTHY | E.W_HAS_P2P
U = 2.0 ** -53


def _cols(n, flags=ON):
    z = np.zeros(n, dtype=np.uint32)
    return dict(flags=np.full(n, flags, dtype=np.uint32), gpu_count=z, gpu_mem_mb=z, gpu_model_class=z, cpu_cores=z, ram_mb=z,
                storage_gb=z, price=z, lat=np.zeros(n), lon=np.zeros(n))


def _code(call):
    with pytest.raises(E.EngineError) as ei:
        call()
    return ei.value.code


def _beats(beats):
    return np.array(beats, dtype=E.mx_beat_dt) if beats else np.zeros(0, dtype=E.mx_beat_dt)


def _entries(entries):
    return np.array(entries, dtype=E.mx_entry_dt) if entries else np.zeros(0, dtype=E.mx_entry_dt)


def _listing(eng, rows=None):
    r = eng.metrics_rows(rows)
    assert not r["_pad"].any()
    return [(int(a), int(b), M.bits(float(c))) for a, b, c in zip(r["row"], r["series"], r["value"])]


def _want(led, rows=None):
    return [(r, s, M.bits(v)) for r, s, v in led.listing(rows)]


class Rig:
    """an engine with W plain workers and the ledger on, and the model beside it"""

    def __init__(self, W):
        self.eng = E.Engine()
        if W:
            self.eng.upload_workers(_cols(W))
        self.eng.metrics_enable(True)
        self.led = M.Ledger()

    def ingest(self, beats, entries, n_series, tag=""):
        self.eng.metrics_ingest(_beats(beats), _entries(entries), n_series)
        self.led.ingest(beats, entries, n_series)
        assert _listing(self.eng) == _want(self.led), tag

    def totals(self):
        s, c = self.eng.metrics_totals()
        return [M.bits(float(x)) for x in s], c.tolist()

    def check_totals(self, tag=""):
        """bit-equal to the model's ordered sums (a NaN as a NaN: its sign is the adder's)"""
        s, c = self.eng.metrics_totals()
        ws, wc = self.led.totals()
        assert c.tolist() == wc, tag
        for k, (x, y) in enumerate(zip(s.tolist(), ws)):
            assert (math.isnan(x) and math.isnan(y)) or M.bits(x) == M.bits(y), (tag, k, x, y)

    def close(self):
        self.eng.close()


# ------------------------------------------------------------------------------------------------ rows

SIZES = [0, 1, 63, 64, 65, 128, 129]


def test_row_sizes_before_and_after_a_beat():
    """every (before, after) pair of 0, 1, 63, 64, 65, 128, 129 — the edges of a 64-slot look — three ways: a REPLACE whose
    series overlap the old ones by half, a MERGE that grows the row, a DELETE that shrinks it; all rows in one batch"""
    pairs = [(b, a) for b in SIZES for a in SIZES]
    r = Rig(3 * len(pairs))
    S = 400
    beats, entries = [], []
    for k, (b, _) in enumerate(pairs):
        for j in range(3):
            beats.append((3 * k + j, M.MERGE, len(entries), b))
            entries += [(2 * i + 1, 0, float(1000 * k + i)) for i in range(b)]      # (odd series, descending places mixed below)
    r.ingest(beats, entries, S, "before")
    beats, entries = [], []
    for k, (b, a) in enumerate(pairs):
        keep = min(a, b) // 2                                                      # REPLACE: half of the old ones, the rest new
        named = [2 * i + 1 for i in range(keep)] + [2 * i for i in range(a - keep)]
        beats.append((3 * k, M.REPLACE, len(entries), a))
        entries += [(s, i & 1, float(-i)) for i, s in enumerate(reversed(named))]
        if a >= b:                                                                 # MERGE: a - b new series, every old one touched
            beats.append((3 * k + 1, M.MERGE, len(entries), a))
            entries += [(2 * i, 0, 0.5 * i) for i in range(a - b)] + [(2 * i + 1, 1, float(1000 * k + i) + (i % 3) - 1) for i in range(b)]
        if a <= b:                                                                 # DELETE: b - a of them, and an absent one
            beats.append((3 * k + 2, M.DELETE, len(entries), b - a + 1))
            entries += [(2 * i + 1, 7, float("nan")) for i in range(b - a)] + [(0, 0, 0.0)]
    r.ingest(beats, entries, S, "after")
    lens = {}
    for row, _, _ in _listing(r.eng):
        lens[row] = lens.get(row, 0) + 1
    for k, (b, a) in enumerate(pairs):
        assert lens.get(3 * k, 0) == a and (a < b or lens.get(3 * k + 1, 0) == a) and (a > b or lens.get(3 * k + 2, 0) == a)
    r.check_totals()
    r.close()


def test_a_row_at_the_bound_and_a_refused_one():
    R = E.MX_ROW_MAX
    assert R == M.ROW_MAX >= 1024
    r = Rig(8)
    full = [(s, 0, float(s) - 0.5) for s in range(R - 1, -1, -1)]
    r.ingest([(3, M.MERGE, 0, R), (5, M.MERGE, 0, 2)], full, R + 2, "a row at the bound")
    before = _listing(r.eng)
    assert len(before) == R + 2
    # one more series: the whole batch is refused, the beat of another row in front of it included
    bad_b, bad_e = [(4, M.MERGE, 0, 1), (3, M.MERGE, 1, 1)], [(0, 0, 1.0), (R, 0, 2.0)]
    assert _code(lambda: r.eng.metrics_ingest(_beats(bad_b), _entries(bad_e), R + 2)) == ERANGE
    with pytest.raises(M.Refused):
        r.led.ingest(bad_b, bad_e, R + 2)
    assert _listing(r.eng) == before == _want(r.led)
    # the bound holds at every moment of the fold: R + 1 series pass through the row although one is deleted later
    bad_b = [(3, M.MERGE, 0, 1), (3, M.DELETE, 0, 1)]
    assert _code(lambda: r.eng.metrics_ingest(_beats(bad_b), _entries([(R, 0, 2.0)]), R + 2)) == ERANGE
    assert _listing(r.eng) == before
    # a REPLACE drops first: a full row swapped for another full row, an entry of the old one among them; then what was
    # refused has room once a series has gone
    swap = [(s, s & 1, float(s)) for s in range(1, R + 1)]
    r.ingest([(3, M.REPLACE, 0, R)], swap, R + 2, "a full row replaced")
    r.ingest([(3, M.DELETE, 0, 1), (3, M.MERGE, 1, 1)], [(7, 0, 0.0), (R + 1, 0, 2.0)], R + 2, "room again")
    assert len(_listing(r.eng, [3])) == R
    r.check_totals()
    r.close()


def _play(r, host_side, ops, one_batch):
    for op in ops:
        if op[0] == "beat":
            host_side.heartbeat(op[1], op[2])
        elif op[0] == "store":
            host_side.store_metrics(op[2], op[1])
        elif op[0] == "manual":
            host_side.store_manual_metrics(op[1], op[2])
        elif op[0] == "delete":
            host_side.delete_metric(op[1], op[2], op[3])
        elif op[0] == "clear":
            host_side.clear_node(op[1])
        if op[0] == "flush" or not one_batch:
            r.ingest(*host_side.take())
    r.ingest(*host_side.take())


@pytest.mark.parametrize("one_batch", [True, False], ids=["one-batch", "a-batch-per-call"])
def test_every_named_case(one_batch):
    """the cases of tests/metrics_cases.py through a host's interner and queue: the ledger holds the hand-written hashes"""
    r = Rig(len(MC.ADDRESSES))
    for c in MC.CASES:
        r.eng.metrics_enable(True)                                   # (enabling again empties the ledger)
        r.led = M.Ledger()
        assert _listing(r.eng) == []
        h = M.Host(MC.ADDRESSES)
        _play(r, h, c["ops"], one_batch)
        assert M.same_fields(h.fields(r.led.listing()), c["want"]), c["name"]
        got = [(int(a), int(b), float(v)) for a, b, v in zip(*[r.eng.metrics_rows()[k] for k in ("row", "series", "value")])]
        assert M.same_fields(h.fields(got), c["want"]), c["name"]
        assert M.same_fields(run_store(c["ops"]).fields(), c["want"]), c["name"]
    r.close()


VALUES = [0.0, -0.0, 1.0, -1.0, 2.5, 1e300, -1e300, float("inf"), float("-inf"), float("nan"), 5e-324, 3.0]


def test_two_hundred_seeded_batches():
    """W = 200 and the manual row; a batch leaves about 30 % of the rows alone and gives the others 1 to 5 beats of mixed kinds,
    with series repeated inside a beat, its beats in a seeded order across the rows; everything compared after every batch"""
    rng = np.random.default_rng(2024)
    W, S = 200, 48
    r = Rig(W)
    kinds = [M.REPLACE, M.REPLACE, M.MERGE, M.MERGE, M.DELETE]
    for k in range(200):
        per_row = []
        for row in list(range(W)) + [M.MANUAL]:
            if rng.random() < 0.3:
                continue
            for _ in range(int(rng.integers(1, 6))):
                n = int(rng.integers(0, 9))
                ser = rng.integers(0, S, size=n)
                if n >= 3 and rng.random() < 0.5:
                    ser[n - 1] = ser[0]                                  # a series twice in one beat
                vals = [float(VALUES[int(i)]) if rng.random() < 0.4 else float(rng.normal() * 10.0 ** int(rng.integers(-3, 4)))
                        for i in rng.integers(0, len(VALUES), size=n)]
                per_row.append((row, int(kinds[int(rng.integers(0, len(kinds)))]),
                                [(int(s), int(rng.integers(0, 2)), v) for s, v in zip(ser, vals)]))
        order = rng.permutation(len(per_row)) if k % 2 else np.arange(len(per_row))   # (every other batch comes sorted by row)
        beats, entries = [], []
        for i in order:
            row, kind, ents = per_row[int(i)]
            beats.append((row, kind, len(entries), len(ents)))
            entries += ents
        r.ingest(beats, entries, S, f"batch {k}")
        if k % 20 == 19:
            r.check_totals(f"batch {k}")
            some = [int(x) for x in rng.integers(0, W, size=7)] + [M.MANUAL, 0, 0]
            assert _listing(r.eng, some) == _want(r.led, some), k
    assert any(M.MANUAL == row for row, _, _ in _listing(r.eng))
    r.close()


# ------------------------------------------------------------------------------------------------ totals

@pytest.mark.parametrize("S", [1, 2, 256, 257, 65536, 65537])
def test_totals_at_the_digit_edges(S):
    """n_series at the edges of the radix regroup's eight-bit digits, a few entries each: small integers, so every order
    sums exactly — sums and counts are the model's bits"""
    r = Rig(9)
    series = sorted({0, S - 1, S // 2, min(255, S - 1), min(256, S - 1), min(65535, S - 1)})
    beats, entries = [], []
    for row in [M.MANUAL, 0, 3, 4, 8]:
        mine = [s for i, s in enumerate(series) if (i + (0 if row == M.MANUAL else row)) % 2 == 0] or series[:1]
        beats.append((row, M.MERGE, len(entries), len(mine)))
        entries += [(s, 0, float((s % 7) - 3 + (0 if row == M.MANUAL else row))) for s in mine]
    r.ingest(beats, entries, S)
    s, c = r.eng.metrics_totals()
    assert len(s) == len(c) == S
    ws, wc = r.led.totals()
    assert [M.bits(x) for x in s.tolist()] == [M.bits(x) for x in ws] and c.tolist() == wc
    assert sum(wc) == len(entries)
    r.close()


def _general_ledger(rng, W, S, per_row, stated=None):
    """every row holds per_row of the series below S; the batch states `stated` series (S if not given)"""
    r = Rig(W)
    beats, entries = [], []
    for row in [M.MANUAL] + list(range(W)):
        ser = rng.choice(S, size=per_row, replace=False)
        beats.append((row, M.REPLACE, len(entries), per_row))
        entries += [(int(s), 0, float(rng.normal() * 10.0 ** int(rng.integers(-8, 9)))) for s in ser]
    r.ingest(beats, entries, stated or S)
    return r


def test_totals_of_general_doubles_are_exact_in_order_and_within_the_bound():
    """2,412 entries (three radix chunks), 300 series (two digits), doubles of mixed sign over sixteen decades: every sum within
    the a-priori bound of ANY summation order, |sum - fsum| <= (n-1)u / (1 - (n-1)u) * sum|x| + u |fsum|, u = 2^-53 — and
    bit-equal to the model's ascending-row sum, which is the order the header states"""
    rng = np.random.default_rng(99)
    r = _general_ledger(rng, 200, 300, 12)
    s, c = r.eng.metrics_totals()
    by_series = {}
    for row in r.led.order():
        for ser, v in r.led.rows[row].items():
            by_series.setdefault(ser, []).append(v)
    worst = 0.0
    for ser in range(300):
        xs = by_series.get(ser, [])
        n = len(xs)
        assert int(c[ser]) == n
        exact = math.fsum(xs)
        bound = ((n - 1) * U / (1 - (n - 1) * U)) * math.fsum(abs(x) for x in xs) + U * abs(exact) if n else 0.0
        err = abs(float(s[ser]) - exact)
        print(f"series {ser}: n {n}, |sum - fsum| {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (ser, n, err, bound)
        worst = max(worst, err / bound if bound else 0.0)
    print(f"worst error / bound: {worst:.3f}")
    r.check_totals()
    r.close()


def test_totals_are_the_same_bits_on_every_call():
    rng = np.random.default_rng(7)
    r = _general_ledger(rng, 150, 70, 9, stated=72)                         # (series 70 and 71: nobody holds them)
    first = r.totals()
    assert r.totals() == first                                              # the cached answer
    # an unrelated ingest and its undo: the table is rebuilt twice, the totals computed afresh
    r.ingest([(11, M.MERGE, 0, 1), (M.MANUAL, M.MERGE, 1, 1)], [(70, 0, 123.25), (71, 1, float("-inf"))], 72)
    assert r.totals() != first
    was = [(s, 0, v) for s, v in r.led.rows[M.MANUAL].items() if s != 71]
    r.ingest([(11, M.DELETE, 0, 1), (M.MANUAL, M.REPLACE, 1, len(was))], [(70, 0, 0.0)] + was, 72)
    assert r.totals() == first
    # the listing in between does not disturb it, and a second engine with the same ledger gives the same bits
    _listing(r.eng)
    assert r.totals() == first
    b, e = [], []
    for row in r.led.order():
        b.append((row, M.MERGE, len(e), len(r.led.rows[row])))
        e += [(s, 0, v) for s, v in r.led.rows[row].items()]
    other = Rig(150)
    other.ingest(b[::-1], e, 72)                                            # (the rows in another batch order)
    assert other.totals() == first
    other.close()
    r.close()


# ------------------------------------------------------------------------------------------------ the join

def _check_join(eng, tag):
    gow, groups, _ = eng.get_groups()
    rows = eng.metrics_rows()
    assert len(rows) > 0
    seen_grouped = seen_free = 0
    for row, gid, cfg in zip(rows["row"].tolist(), rows["group_id"].tolist(), rows["config"].tolist()):
        if row == M.MANUAL or gow[row] < 0:
            assert (gid, cfg) == (M.NONE, 0), (tag, row)
            seen_free += 1
        else:
            g = groups[gow[row]]
            assert (gid, cfg) == (int(g["id"]), int(g["config"])), (tag, row)
            seen_grouped += 1
    named = [M.MANUAL, 0, eng.W - 1, 5]
    sub = eng.metrics_rows(named)
    assert sub["row"].tolist() == [r for r in named if r in set(rows["row"].tolist())]     # (one entry a row, or none yet)
    for row, gid, cfg in zip(sub["row"].tolist(), sub["group_id"].tolist(), sub["config"].tolist()):
        want = (M.NONE, 0) if row == M.MANUAL or gow[row] < 0 else (int(groups[gow[row]]["id"]), int(groups[gow[row]]["config"]))
        assert (gid, cfg) == want, (tag, row)
    print(f"{tag}: {seen_grouped} entries of grouped workers, {seen_free} of others")
    return seen_grouped, seen_free


def _one_entry_each(eng, W):
    rows = [M.MANUAL] + list(range(W))
    eng.metrics_ingest(_beats([(r, M.REPLACE, i, 1) for i, r in enumerate(rows)]), _entries([(0, 0, float(i)) for i in range(len(rows))]), 1)


def test_join_follows_the_groups_through_ticks_churn_and_dissolution():
    cs = ChurnStream(3, 3, W0=220, n_churn=12, n_new=10, T0=40)
    sw = cs.sw_all
    packed = host.pack_workers(sw)
    pick = lambda idx: {k: np.ascontiguousarray(v[idx]) for k, v in packed.items()}
    eng = E.Engine(group_id_seed=1)
    cfg_rows, alt_rows, req_models = host.pack_configs(sw.configs)
    eng.set_configs(cfg_rows, alt_rows)
    eng.set_model_table(host.build_model_table(req_models, sw.model_names), len(req_models), len(sw.model_names))
    eng.upload_workers(pick(np.arange(cs.W0)))
    eng.upload_tasks(cs.masks, cs.created, cs.uid)
    eng.set_enabled_mask(sw.enabled_mask())
    eng.metrics_enable(True)
    _one_entry_each(eng, cs.W0)
    assert _check_join(eng, "before any tick")[0] == 0
    eng.tick()
    grouped, free = _check_join(eng, "after a tick")
    assert grouped > 0 and free > 0
    flags = packed["flags"].astype(np.int64)
    for k in range(2):
        leave, idx_new, new_tasks = cs.step()
        eng.on_worker_status_many(leave, flags[leave] & ~E.W_HEALTHY, np.ones(len(leave), dtype=np.uint32))
        _check_join(eng, f"churn {k}: deaths pending")
        eng.append_workers(pick(idx_new))
        eng.tasks_insert_front(*new_tasks[:3])
        _check_join(eng, f"churn {k}: rows appended")
        eng.tick()
        _one_entry_each(eng, cs.W)                                          # the appended rows report too
        assert _check_join(eng, f"churn {k}: after the tick")[0] > 0
    gid = engine_groups(eng)[0][0]
    members = engine_groups(eng)[0][2]
    assert eng.dissolve_group_by_id(gid)
    _check_join(eng, "after pm_dissolve_group_by_id")
    got = eng.metrics_rows(members)
    assert (got["group_id"] == M.NONE).all() and not got["config"].any()
    eng.close()


def test_join_after_a_solo_merge_and_both_uploads():
    """130 adopted single-node groups of a (1, 3) configuration, which the tick's merge pass folds into trios; then pm_upload_workers
    keeping the groups (rows behind the known ones are new and empty) and dropping them (every worker row emptied, the manual
    row kept)"""
    W = 130
    eng = E.Engine(group_id_seed=5)
    cfg_rows, alt_rows, _ = host.pack_configs([("trio", 1, 3, None)])
    eng.set_configs(cfg_rows, alt_rows)
    eng.upload_workers(_cols(W))
    eng.upload_tasks(np.array([1, 1], dtype=np.uint64), np.array([5, 4], dtype=np.int64), np.array([101, 102], dtype=np.uint64))
    g = np.zeros(W, dtype=E.group_dt)
    for i in range(W):
        g[i] = (0x7000 + i, 0, 1, i, M.NONE)
    eng.adopt_groups(g, np.arange(W, dtype=np.uint32), 77)
    eng.metrics_enable(True)
    _one_entry_each(eng, W)
    assert _check_join(eng, "adopted solos") == (W, 1)
    stats = eng.tick()
    print("merged", stats["n_merged"], "groups", stats["n_groups"])
    assert stats["n_merged"] > 0
    sizes = {len(m) for _, _, m, _ in engine_groups(eng)}
    assert max(sizes) > 1
    _check_join(eng, "after the solo merge")
    before = _listing(eng)
    eng.upload_workers(_cols(W + 40), keep_groups=True)
    assert _listing(eng) == before                                          # the new rows are empty
    assert _check_join(eng, "upload keeping the groups")[0] > 0
    eng.metrics_ingest(_beats([(W + 39, M.MERGE, 0, 1)]), _entries([(0, 0, 9.0)]), 1)
    assert _listing(eng, [W + 39]) == [(W + 39, 0, M.bits(9.0))]
    eng.upload_workers(_cols(W - 30))
    assert _listing(eng) == [(M.MANUAL, 0, M.bits(0.0))]                    # the manual row alone
    s, c = eng.metrics_totals()
    assert (s.tolist(), c.tolist()) == ([0.0], [1])
    _one_entry_each(eng, W - 30)
    assert _check_join(eng, "upload dropping the groups") == (0, W - 29)
    eng.close()


# ------------------------------------------------------------------------------------------------ the liveness hook

def test_a_sweep_empties_the_rows_that_became_dead():
    rng = np.random.default_rng(12)
    W = 200
    flags = np.full(W, ON, dtype=np.uint32)
    cols = _cols(W)
    a, b = E.Engine(), E.Engine()                                           # b never hears of metrics
    for eng in (a, b):
        eng.upload_workers(cols)
        eng.liveness_enable(True, 1)
    a.metrics_enable(True)
    led = M.Ledger()
    beats, entries = [], []
    for row in [M.MANUAL] + list(range(0, W, 2)):                           # every other worker holds metrics
        n = int(rng.integers(1, 6))
        beats.append((row, M.REPLACE, len(entries), n))
        entries += [(int(s), 0, float(rng.integers(-9, 9))) for s in rng.choice(10, size=n, replace=False)]
    a.metrics_ingest(_beats(beats), _entries(entries), 10)
    led.ingest(beats, entries, 10)
    live = LM.Ledger(flags, 1)
    now = 1_760_000_000_000
    silent = np.array(sorted(rng.choice(W, size=40, replace=False).tolist()))
    total_dead = 0
    for k in range(3):                                                      # Healthy -> Unhealthy -> Dead -> Dead
        now += 15_000
        last = np.full(W, now - 1000, dtype=np.uint64)
        last[silent] = now - 200_000
        want_rows, want_census = live.sweep(now, last)
        na, ca = a.liveness_sweep(now, last, None, apply=(k == 1))
        nb, cb = b.liveness_sweep(now, last, None, apply=(k == 1))
        assert na == nb == len(want_rows) and ca.tolist() == cb.tolist() == want_census
        assert a.liveness_transitions().tobytes() == b.liveness_transitions().tobytes()
        dead = [w for w, _, new, _ in want_rows if new == LM.DEAD]
        total_dead += len(dead)
        for w in dead:
            led.clear_row(w)
        assert _listing(a) == _want(led), k
        assert engine_groups(a) == engine_groups(b)
    assert total_dead == 40 and any(w % 2 == 0 for w in silent) and any(w % 2 for w in silent)
    s, c = a.metrics_totals()
    ws, wc = led.totals()
    assert s.tolist() == ws and c.tolist() == wc
    # metrics off again: the sweep goes on as before
    a.metrics_enable(False)
    now += 15_000
    last = np.full(W, now - 1000, dtype=np.uint64)
    assert a.liveness_sweep(now, last)[0] == b.liveness_sweep(now, last)[0] == 40
    assert a.liveness_transitions().tobytes() == b.liveness_transitions().tobytes()
    a.close(), b.close()


# ------------------------------------------------------------------------------------------------ errors and neutrality

def test_errors_leave_the_ledger_as_it_was():
    W = 50
    eng = E.Engine()
    one_b, one_e = _beats([(M.MANUAL, M.MERGE, 0, 1)]), _entries([(0, 0, 1.0)])
    # off
    assert _code(lambda: eng.metrics_ingest(one_b, one_e, 1)) == ESTATE
    assert _code(eng.metrics_totals) == ESTATE
    assert _code(eng.metrics_rows) == ESTATE
    # on, no workers: the manual row works, a worker row is PM_ESTATE
    eng.metrics_enable(True)
    eng.metrics_ingest(one_b, one_e, 1)
    assert _listing(eng) == [(M.MANUAL, 0, M.bits(1.0))]
    assert _code(lambda: eng.metrics_ingest(_beats([(0, M.MERGE, 0, 1)]), one_e, 1)) == ESTATE
    assert _code(lambda: eng.metrics_rows([0])) == ESTATE
    assert _listing(eng, [M.MANUAL]) == [(M.MANUAL, 0, M.bits(1.0))]
    eng.upload_workers(_cols(W))
    led = M.Ledger()
    led.ingest([(M.MANUAL, M.MERGE, 0, 1)], [(0, 0, 1.0)], 1)
    b, e = [(7, M.REPLACE, 0, 2), (49, M.MERGE, 2, 1)], [(1, 0, 2.0), (2, 1, 3.0), (0, 0, 4.0)]
    eng.metrics_ingest(_beats(b), _entries(e), 3)
    led.ingest(b, e, 3)
    before, totals = _want(led), eng.metrics_totals()

    def unchanged():
        assert _listing(eng) == before
        s, c = eng.metrics_totals()
        assert s.tobytes() == totals[0].tobytes() and c.tolist() == totals[1].tolist()

    unchanged()
    L, h = E.lib(), eng._h
    good = _beats([(7, M.MERGE, 0, 1)])
    assert L.pm_metrics_ingest(h, None, 1, one_e.ctypes.data, 1, 3) == EINVAL               # null arguments
    assert L.pm_metrics_ingest(h, good.ctypes.data, 1, None, 1, 3) == EINVAL
    assert L.pm_metrics_totals(h, None, None, 0, None) == EINVAL
    assert _code(lambda: eng.metrics_ingest(_beats([(7, M.MERGE, 0, 1), (7, 3, 0, 1)]), one_e, 3)) == EINVAL      # an unknown kind
    assert _code(lambda: eng.metrics_ingest(good, _entries([(0, 2, 1.0)]), 3)) == EINVAL                          # an unknown flag
    assert _code(lambda: eng.metrics_ingest(_beats([(7, M.MERGE, 0, 1), (8, M.MERGE, 1, 1)]), one_e, 3)) == EINVAL  # first + n
    assert _code(lambda: eng.metrics_ingest(_beats([(7, M.MERGE, 0xFFFFFFFF, 2)]), one_e, 3)) == EINVAL
    unchanged()
    assert _code(lambda: eng.metrics_ingest(_beats([(7, M.MERGE, 0, 1), (W, M.MERGE, 0, 1)]), one_e, 3)) == ERANGE  # a row >= W
    assert _code(lambda: eng.metrics_ingest(good, _entries([(3, 0, 1.0)]), 3)) == ERANGE                          # a series >= n_series
    assert _code(lambda: eng.metrics_ingest(_beats([(7, M.DELETE, 0, 1)]), _entries([(3, 0, 1.0)]), 3)) == ERANGE
    assert _code(lambda: eng.metrics_rows([0, W])) == ERANGE
    unchanged()
    eng.metrics_ingest(_beats([(7, M.DELETE, 0, 1)]), _entries([(0, 99, 1.0)]), 3)           # a DELETE's flags are ignored
    unchanged()
    # short buffers: the count comes back, nothing is copied
    n = E.C.c_uint32(0)
    small = np.zeros(len(before), dtype=E.mx_row_dt)
    assert L.pm_metrics_rows(h, None, 0, small.ctypes.data, len(before) - 1, E.C.byref(n)) == ERANGE
    assert n.value == len(before) and not small["series"].any() and not small["value"].any()
    assert L.pm_metrics_rows(h, None, 0, None, 1 << 20, E.C.byref(n)) == ERANGE and n.value == len(before)
    s, c = np.zeros(3), np.zeros(3, dtype=np.uint32)
    assert L.pm_metrics_totals(h, s.ctypes.data, c.ctypes.data, 2, E.C.byref(n)) == ERANGE
    assert n.value == 3 and not s.any() and not c.any()
    unchanged()
    # a stepwise tick in progress
    sw = make_swarm(5, 40, W)
    host.load_swarm(eng, sw)
    led.clear_workers()
    before = _want(led)
    assert _listing(eng) == before
    totals = eng.metrics_totals()
    eng.dist_configure(0, 1)
    eng.dist_tick_begin()
    assert _code(lambda: eng.metrics_ingest(one_b, one_e, 3)) == ESTATE
    assert _code(eng.metrics_totals) == ESTATE
    assert _code(eng.metrics_rows) == ESTATE
    assert _code(lambda: eng.metrics_enable(True)) == ESTATE
    assert _code(lambda: eng.metrics_enable(False)) == ESTATE
    eng.dist_carve_wait()
    eng.dist_match_begin()
    eng.dist_tick_end()
    unchanged()
    # multi-GPU engines are out of scope, both ways round
    assert _code(lambda: eng.dist_configure(0, 2, np.zeros(W, dtype=np.uint8))) == ESTATE
    unchanged()
    eng.metrics_enable(False)
    eng.dist_configure(0, 2, np.zeros(W, dtype=np.uint8))
    assert _code(lambda: eng.metrics_enable(True)) == ESTATE
    eng.close()


def test_the_ledger_leaves_the_tick_alone():
    """the same churn stream through an engine with the ledger on and fed between the ticks (ingests, totals, listings, with
    status changes pending) and through one that never enabled it: groups, published rows and the counters of every tick equal.
    The counters compared are the ones that are a function of the engine's state: groups, formed, merged, carve steps and pair
    evaluations.  The others of pm_stats (proposals, fast steps, launches, candidates scanned) count how the streaming carve's row
    makers and its validator met in time and differ between two runs of one engine: proposals read 491 against 492 in one run of
    this test and equal in two others."""
    def make():
        cs = ChurnStream(2, 4, W0=600, n_churn=20, n_new=30, T0=100)
        sw = cs.sw_all
        packed = host.pack_workers(sw)
        eng = E.Engine(group_id_seed=1)
        cfg_rows, alt_rows, req_models = host.pack_configs(sw.configs)
        eng.set_configs(cfg_rows, alt_rows)
        eng.set_model_table(host.build_model_table(req_models, sw.model_names), len(req_models), len(sw.model_names))
        eng.upload_workers({k: np.ascontiguousarray(v[:cs.W0]) for k, v in packed.items()})
        eng.upload_tasks(cs.masks, cs.created, cs.uid)
        eng.set_enabled_mask(sw.enabled_mask())
        return cs, packed, eng

    (ca, pa, a), (cb, pb, b) = make(), make()
    a.metrics_enable(True)
    rng = np.random.default_rng(1)
    counters = ("n_groups", "n_formed", "n_merged", "carve_steps", "pair_evals")
    flags = pa["flags"].astype(np.int64)

    def feed():
        rows = rng.choice(a.W, size=60, replace=False).tolist() + [M.MANUAL]   # (a.W: the rows the engine holds now)
        a.metrics_ingest(_beats([(r, M.REPLACE, 2 * i, 2) for i, r in enumerate(rows)]),
                         _entries([(int(s), int(s) & 1, float(s)) for s in rng.integers(0, 20, size=2 * len(rows))]), 20)
        a.metrics_totals()
        a.metrics_rows()
        a.metrics_rows(rows[:5])

    for k in range(4):
        if k:
            for cs, packed, eng in ((ca, pa, a), (cb, pb, b)):
                leave, idx_new, new_tasks = cs.step()
                eng.on_worker_status_many(leave, flags[leave] & ~E.W_HEALTHY, np.ones(len(leave), dtype=np.uint32))
                if eng is a:
                    pushes = a.debug_delta_pushes()
                    feed()                                                  # with the deaths pending
                    assert a.debug_delta_pushes() == pushes
                eng.append_workers({k2: np.ascontiguousarray(v[idx_new]) for k2, v in packed.items()})
                eng.tasks_insert_front(*new_tasks[:3])
        feed()
        sa, sb = a.tick(), b.tick()
        assert {c: sa[c] for c in counters} == {c: sb[c] for c in counters}, k
        la, lb = a.last_stats(), b.last_stats()
        assert {c: la[c] for c in counters} == {c: lb[c] for c in counters}, k
        feed()
        assert engine_groups(a) == engine_groups(b), k
        for w in range(ca.W):
            x, y = a.lookup(w), b.lookup(w)
            assert (x.task, x.group_slot, x.group_index, x.group_size, x.next_worker, x.group_id) == \
                   (y.task, y.group_slot, y.group_index, y.group_size, y.next_worker, y.group_id), (k, w)
    a.close(), b.close()
