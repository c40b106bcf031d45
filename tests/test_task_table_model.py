"""tests/task_table_model.py against brute force (CPU): a few hundred seeded sequences of upload / insert_front / delete, after
every operation each answer of the incremental list recomputed from a freshly sorted bag of rows; the shadow of the index
space against its invariants and against hand-worked thresholds; the detector masks' promises."""
import numpy as np
import pytest

from oracle import oracle_ffi as orc
from protocol_amd.swarm import wide_config_swarm
import task_table_model as M

C = 24
NONE = M.NONE


class Bag:
    """rows with their arrival stamps; the list is re-sorted for every answer: created_at descending, ties in arrival order
    of their batch (later batches are strictly newer, so ties only happen inside one)"""

    def __init__(self):
        self.rows = []                                   # (created, tie rank, mask, uid or None)

    def upload(self, mask, created, uid):
        self.rows = [(int(c), i, int(m), None if uid is None else int(uid[i])) for i, (m, c) in enumerate(zip(mask, created))]

    def insert(self, mask, created, uid):
        self.rows += [(int(c), i, int(m), None if uid is None else int(uid[i])) for i, (m, c) in enumerate(zip(mask, created))]

    def sorted(self):
        return sorted(self.rows, key=lambda r: (-r[0], r[1]))

    def delete(self, uids):
        for u in set(int(x) for x in uids):
            for r in self.sorted():
                if r[3] == u:
                    self.rows.remove(r)
                    break


def _brute_answers(rows, cfg_of_node, col):
    T = len(rows)
    newest = NONE
    for i, r in enumerate(rows):
        if newest == NONE or r[0] >= rows[newest][0]:
            newest = i
    first_w = np.full(len(cfg_of_node), NONE, dtype=np.uint32)
    count_w = np.zeros(len(cfg_of_node), dtype=np.uint32)
    for w, c in enumerate(cfg_of_node):
        if c < 0:
            continue
        hits = [i for i, r in enumerate(rows) if (r[2] >> int(c)) & 1]
        count_w[w] = len(hits)
        if hits:
            first_w[w] = hits[0]
    first_t = np.full(T, NONE, dtype=np.uint32)
    count_t = np.zeros(T, dtype=np.uint32)
    for i, r in enumerate(rows):
        hits = [w for w, m in enumerate(col) if int(m) & r[2]]
        count_t[i] = len(hits)
        if hits:
            first_t[i] = hits[0]
    return newest, first_w, count_w, first_t, count_t


@pytest.fixture(scope="module")
def cfgs():
    sw = wide_config_swarm(5, 30, 40, C)
    _n, cfgs, _t, _e = orc.from_swarm(sw)
    return cfgs


@pytest.mark.parametrize("seed0", range(0, 300, 25))
def test_list_answers_equal_brute_force(seed0, cfgs):
    for seed in range(seed0, seed0 + 25):
        rng = np.random.default_rng(seed)
        W = 23
        cfg_of_node = rng.integers(-1, C, W).astype(np.int32)
        col = rng.integers(0, 1 << C, W).astype(np.uint64) * (rng.random(W) < 0.7)
        lst, bag, shadow = M.TaskList(), Bag(), M.IndexShadow()
        next_g, next_uid, clock = 0, 1000, 10 ** 6
        with_uid = seed % 5 != 0
        for step in range(8):
            op = 0 if step == 0 else int(rng.integers(0, 8))
            if op == 0 or (op == 1 and not with_uid):                        # upload
                n = int(rng.integers(0, 130))
                g = np.arange(next_g, next_g + n)
                mask = M.detector_masks(g, C)
                created = np.sort(clock + rng.integers(0, max(n // 2, 1), n))[::-1]   # (ties)
                uid = np.arange(next_uid, next_uid + n, dtype=np.uint64) if with_uid else None
                if with_uid and n > 4 and seed % 3 == 0:
                    uid[n // 2] = uid[1]                                       # a duplicated id
                next_uid += n
                clock += n + 1
                lst.upload(mask, created, uid)
                bag.upload(mask, created, uid)
                shadow.upload(n, with_uid)
            elif op in (2, 3, 4):                                              # insert in front
                n = int(rng.integers(0, 70))
                next_g -= n
                mask = M.detector_masks(np.arange(next_g, next_g + n), C)
                created = np.sort(clock + 1 + rng.integers(0, max(n // 2, 1), n))[::-1]
                uid = np.arange(next_uid, next_uid + n, dtype=np.uint64) if with_uid else None
                if with_uid and n > 2 and len(lst) > 2 and seed % 3 == 0:
                    uid[n - 1] = lst.uid[len(lst) // 2]                        # the id of an older row
                next_uid += n
                clock += n + 2
                lst.insert_front(mask, created, uid)
                bag.insert(mask, created, uid)
                shadow.insert_front(n, with_uid)
            elif with_uid and len(lst):                                        # delete: some rows, an id twice, unknown ids
                k = int(rng.integers(1, max(2, len(lst) // 3)))
                uids = rng.choice(lst.uid, size=k, replace=True)
                uids = np.concatenate([uids, uids[:1], np.array([7, 8], dtype=np.uint64)])
                gone = lst.delete(uids)
                bag.delete(uids)
                shadow.delete(gone)
                assert len(gone) < 2 or (np.diff(gone) > 0).all()
            rows = bag.sorted()
            assert [r[2] for r in rows] == [int(m) for m in lst.mask], (seed, step)
            assert [r[0] for r in rows] == [int(c) for c in lst.created], (seed, step)
            if with_uid:
                assert [r[3] for r in rows] == [int(u) for u in lst.uid], (seed, step)
                for u in set(r[3] for r in rows[:20]):
                    assert lst.position_of(u) == [r[3] for r in rows].index(u)
                assert lst.position_of(5) == NONE
            newest, first_w, count_w, first_t, count_t = _brute_answers(rows, cfg_of_node, col)
            assert lst.newest() == newest, (seed, step)
            got_first, got_count = lst.per_worker(cfgs, cfg_of_node)
            assert np.array_equal(got_count, count_w), (seed, step)
            assert np.array_equal(got_first, first_w), (seed, step)
            got_first, got_count = lst.per_task(col)
            assert np.array_equal(got_first, first_t) and np.array_equal(got_count, count_t), (seed, step)
            # the shadow's invariants
            assert shadow.T == len(lst) and shadow.t_lo + len(shadow.cells) == shadow.t_cap
            assert shadow.t_cap % 64 == 0 and shadow.t_dead <= shadow.T + M.DEAD_SLACK
            assert len(shadow.cells) == 0 or shadow.cells[0]


def test_shadow_thresholds_by_hand():
    """4,300 rows: capacity 2 x 4,300 + 65,536 = 74,136 -> 74,176 (a multiple of 64).  With row 0 alive nothing is trimmed;
    t_dead == T + 4,096 at T = 102, t_dead = 4,198: no compaction; one more delete (T = 101, 4,199 > 4,197): a compaction."""
    assert M.task_capacity_for(0) == 65536 and M.task_capacity_for(4300) == 74176 and M.task_capacity_for(1) == 65600
    s = M.IndexShadow()
    s.upload(4300, True)
    assert s.state() == dict(t_lo=74176 - 4300, t_cap=74176, T=4300, t_dead=0, regrowths=0, compactions=0)
    s.delete(np.arange(1, 4199))                       # 4,198 rows behind row 0
    assert (s.T, s.t_dead, s.compactions, s.t_lo) == (102, 4198, 0, 74176 - 4300)
    s.delete([1])
    assert (s.T, s.t_dead, s.compactions, s.t_lo) == (101, 0, 1, 74176 - 101)
    # front deletes are trimmed, whole dead words too
    s.delete(np.arange(0, 70))
    assert (s.T, s.t_dead, s.t_lo) == (31, 0, 74176 - 31)
    # an insertion of exactly t_lo rows fits; one more regrows into task_capacity_for(T + n)
    a, b = M.IndexShadow(), M.IndexShadow()
    for x in (a, b):
        x.upload(100, True)
    lo = a.t_lo
    a.insert_front(lo, True)
    assert (a.t_lo, a.t_cap, a.regrowths, a.T) == (0, M.task_capacity_for(100), 0, 100 + lo)
    b.insert_front(lo + 1, True)
    cap = M.task_capacity_for(100 + lo + 1)
    assert (b.t_cap, b.regrowths, b.T, b.t_lo) == (cap, 1, 101 + lo, cap - 101 - lo)
    # an upload keeps a space that is large enough and not oversized, and re-allocates when the ids come or go
    a.upload(50, True)
    assert a.t_cap == M.task_capacity_for(100)
    a.upload(50, False)
    assert a.t_cap == M.task_capacity_for(50)
    a.upload(a.t_cap - 63, False)
    assert a.t_cap == M.task_capacity_for(M.task_capacity_for(50) - 63)


def test_detector_masks_keep_their_promises():
    g = np.arange(-5000, 5000)
    c = M.detector_config(g, C)
    assert (c[1:] != c[:-1]).all() and (c[64:] != c[:-64]).all() and c.min() == 0 and c.max() == C - 1
    m = M.detector_masks(g, C)
    valid = np.uint64((1 << C) - 1)
    single = np.array([bin(int(x)).count("1") == 1 for x in m & valid])
    plain = single & ((m & ~valid) == 0)
    assert plain.mean() > 0.9
    # the sprinkles: ~0, 0, bits at or above C only, and a configuration with such bits beside it
    assert (m == M.ALL).sum() > 50 and (m == 0).sum() > 50
    assert ((m != 0) & ((m & valid) == 0)).sum() > 50
    assert (single & ((m & ~valid) != 0) & (m != M.ALL)).sum() > 50
    # neighbours, and rows a word apart, still differ wherever both are plain
    both = plain[1:] & plain[:-1]
    assert (m[1:][both] != m[:-1][both]).all()
    both = plain[64:] & plain[:-64]
    assert (m[64:][both] != m[:-64][both]).all()
