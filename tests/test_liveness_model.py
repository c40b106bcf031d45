"""tests/liveness_model.py against the reference's own tests (tests/golden/status_update_kats.json, transcribed from
orchestrator/src/status_update/mod.rs:407-1073) and against the hand-written outcomes of tests/liveness_cases.py; every arm
of the model must be reached by them.  No GPU."""
import json
import os

import numpy as np
import pytest

import liveness_cases as LC
import liveness_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "status_update_kats.json")))["kats"]
DEFAULT_THRESHOLD = 3  # status_update/mod.rs:43


@pytest.mark.parametrize("kat", KATS, ids=[k["test"] for k in KATS])
def test_model_gives_what_the_references_tests_assert(kat):
    m = DEFAULT_THRESHOLD if kat["threshold"] is None else kat["threshold"]
    s, c, _, _, _ = M.step(M.NAMES.index(kat["status"]), kat["counter"], kat["beat"], kat["in_pool"], m)
    assert (M.NAMES[s], c) == (kat["want_status"], kat["want_counter"])


def test_the_kats_name_every_test_of_the_reference():
    names = {k["test"].split(" (")[0] for k in KATS}
    assert len(names) == 9 and all(k["lines"] for k in KATS)


@pytest.mark.parametrize("c", LC.CASES, ids=[c["name"] for c in LC.CASES])
def test_named_case(c):
    present = M.beat_present(LC.NOW_MS, LC.beat_ms(c))
    s, cnt, listed, _, _ = M.step(c["status"], c["counter"], present, c["in_pool"], c["m"])
    assert (s, cnt, listed) == c["want"]


def test_every_label_is_reached():
    arms, counters = set(), set()
    for c in LC.CASES:
        _, _, _, arm, cl = M.step(c["status"], c["counter"], M.beat_present(LC.NOW_MS, LC.beat_ms(c)), c["in_pool"], c["m"])
        arms.add(arm), counters.add(cl)
    assert arms == set(M.LABELS) and counters == set(M.COUNTER_LABELS)


def test_case_names_are_distinct_and_thresholds_cover_the_edges():
    assert len({c["name"] for c in LC.CASES}) == len(LC.CASES)
    assert LC.THRESHOLDS == [0, 1, 3]


def test_beat_edge_is_the_headers():
    now = LC.NOW_MS
    assert M.beat_present(now, now - 89_999) and M.beat_present(now, now - 90_000) and not M.beat_present(now, now - 90_001)
    assert M.beat_present(now, now + 1) and M.beat_present(now, now) and not M.beat_present(now, 0)
    assert not M.beat_present(50, 0) and M.beat_present(50, 1)          # (a clock that starts near zero)


def test_ledger_sweep_lists_ascending_and_counts_everyone():
    rng = np.random.default_rng(5)
    W = 300
    flags = np.where(rng.random(W) < 0.5, M.W_HEALTHY, 0)
    led = M.Ledger(flags, 3)
    assert led.status == [M.HEALTHY if f else M.DISCOVERED for f in flags]
    led.set([5, 5, 7], [M.BANNED, M.WAITING, M.DEAD], [1, 2, 3])           # (a repeated index: its last entry)
    assert (led.status[5], led.counter[5], led.status[7], led.counter[7]) == (M.WAITING, 2, M.DEAD, 3)
    beats = np.where(rng.random(W) < 0.5, LC.NOW_MS - 10, 0)
    pool = M.pack_bits(rng.random(W) < 0.5)
    rows, census = led.sweep(LC.NOW_MS, beats, pool)
    assert [r[0] for r in rows] == sorted(r[0] for r in rows) and sum(census) == W
    assert all(led.status[w] == new and led.counter[w] == c for w, _, new, c in rows)
    led.append([M.W_HEALTHY, 0])
    assert led.status[-2:] == [M.HEALTHY, M.DISCOVERED] and led.counter[-2:] == [0, 0]
