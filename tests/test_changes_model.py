"""tests/changes_model.py against brute force: the per-row bits, accumulation over publishes, the resync rule and the
word-prefix expansion of the drain's list — and the Python binding's names for the feed (no GPU needed)."""
import random

import pytest

import changes_model as M


def _table(rng, W, n_groups=5, tasks=(None, 11, 12)):
    t = []
    for w in range(W):
        if rng.random() < 0.3:
            t.append(M.NO_GROUP)
        else:
            t.append((1000 + rng.randrange(n_groups), rng.randrange(3), 1 + rng.randrange(3), rng.randrange(W), rng.choice(tasks)))
    return t


def test_bits_of_one_row():
    a = (7, 0, 2, 5, 11)
    assert M.what(a, a) == 0
    assert M.what(a, (8, 0, 2, 5, 11)) == M.GROUP
    assert M.what(a, (7, 1, 2, 5, 11)) == M.RING
    assert M.what(a, (7, 0, 3, 5, 11)) == M.RING
    assert M.what(a, (7, 0, 2, 6, 11)) == M.RING
    assert M.what(a, (7, 0, 2, 5, 12)) == M.TASK
    assert M.what(a, (7, 0, 2, 5, None)) == M.TASK
    assert M.what(a, M.NO_GROUP) == M.ALL
    assert M.what(M.NO_GROUP, M.NO_GROUP) == 0
    assert M.what(M.NO_GROUP, (7, 0, 1, 3, None)) == M.GROUP | M.RING     # a solo group without a task: size 0 -> 1, next
    assert M.row_of(M.NONE, 99, 1, 2, 3, 4) == M.NO_GROUP and M.row_of(0, 99, 1, 2, 3, 4) == (99, 1, 2, 3, 4)


def test_appended_rows_compare_against_no_group():
    prev = [(7, 0, 1, 0, 11)]
    cur = prev + [M.NO_GROUP, (8, 0, 1, 2, None)]
    assert M.diff(prev, cur) == [0, 0, M.GROUP | M.RING]


@pytest.mark.parametrize("seed", range(5))
def test_accumulation_is_a_union_of_per_publish_differences(seed):
    rng = random.Random(seed)
    W = 200
    tables = [_table(rng, W) for _ in range(5)]
    tables.append(tables[3])                                   # (changed and changed back: stays listed)
    f = M.Feed()
    f.publish(tables[0])
    rows, flag = f.drain()
    assert flag and rows == [(w, M.ALL) for w in range(W)]
    assert f.drain() == ([], False)
    for t in tables[1:]:
        f.publish(t)
    want = [0] * W
    for a, b in zip(tables, tables[1:]):
        for w in range(W):
            want[w] |= M.what(a[w], b[w])
    rows, flag = f.drain()
    assert not flag and rows == [(w, b) for w, b in enumerate(want) if b]
    assert [w for w, _ in rows] == sorted(w for w, _ in rows)
    back = [w for w in range(W) if tables[4][w] != tables[3][w]]
    assert back and all(dict(rows).get(w) for w in back)
    assert f.drain() == ([], False)


def test_resync_lists_every_row_once_and_drops_marks_of_rows_that_went():
    rng = random.Random(9)
    f = M.Feed()
    f.publish(_table(rng, 50))
    f.drain()
    f.publish(_table(rng, 50))                                 # marks pending ...
    f.resync()
    f.publish(_table(rng, 20))                                 # ... a shorter table behind a resync
    rows, flag = f.drain()
    assert flag and rows == [(w, M.ALL) for w in range(20)]
    t = _table(rng, 20)
    f.publish(t)
    f.publish(t)
    rows, flag = f.drain()
    assert not flag and all(w < 20 for w, _ in rows)


@pytest.mark.parametrize("W", [1, 63, 64, 65, 255, 256, 257, 4097])
@pytest.mark.parametrize("density", ["0", "1", "1/64", "random"])
def test_word_prefix_expansion_against_brute_force(W, density):
    rng = random.Random(W * 7 + len(density))
    p = {"0": 0.0, "1": 1.0, "1/64": 1 / 64, "random": rng.random()}[density]
    what = [rng.randrange(1, 8) if rng.random() < p else 0 for _ in range(W)]
    brute = [(w, b) for w, b in enumerate(what) if b]
    assert M.drain_list(what) == brute
    words = M.bitmap_of(what)
    assert len(words) == (W + 63) // 64 and all(not (words[-1] >> b) & 1 for b in range(W - 64 * (len(words) - 1), 64))
    # any shape of the scanning workgroup gives the same prefix (passes of 1, 2 and many threads' worth)
    ref = M.word_prefix(words)
    for wpt, thr in ((1, 1), (4, 2), (3, 5), (4, 256)):
        assert M.word_prefix(words, wpt, thr) == ref
    acc = 0
    for j, word in enumerate(words):
        assert ref[0][j] == acc
        acc += bin(word).count("1")
    assert ref[1] == acc == len(brute)


def test_the_binding_names_the_feed():
    from protocol_amd import engine as E
    assert {"pm_enable_assignment_changes", "pm_drain_assignment_changes"} <= set(E.EXPORTS)
    assert E.change_row_dt.names == ("worker", "what") and E.change_row_dt.itemsize == 8
    assert (E.CHG_GROUP, E.CHG_RING, E.CHG_TASK, E.CHANGES_RESYNC) == (M.GROUP, M.RING, M.TASK, 1)
    assert callable(E.Engine.enable_assignment_changes) and callable(E.Engine.drain_assignment_changes)
