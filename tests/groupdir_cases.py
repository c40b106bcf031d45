"""Named cases of the group directory: small states whose answers are written out by hand, the id edge set of the text order,
and the builders of the shapes the GPU tests install (tests/test_gpu_groupdir.py).  tests/test_groupdir_model.py holds the model
of tests/groupdir_model.py to the hand-written answers; the GPU tests hold the engine to the model."""
import numpy as np

import groupdir_model as M

H, U, D, W8, DI = M.HEALTHY, M.UNHEALTHY, M.DEAD, M.WAITING, M.DISCOVERED
RUN, PEND, NO = M.RUNNING, 0, M.TS_NONE


def id_edge_set():
    """the ids at which a text order can go wrong: the shortest texts, every 1 followed by k zeros, all ones, pairs that differ
    only in trailing zero digits, pairs equal in the top 8, 15 and 16 digits"""
    ids = [0, 1, 0xF, 0x10, 0xFF, 0x100, (1 << 64) - 1]
    ids += [1 << (4 * k) for k in range(16)]
    ids += [0xAB, 0xAB0, 0xAB00, 0xAB000000, 0xAB00000000000000]                      # trailing zero digits only
    ids += [0x12345678_00000001, 0x12345678_00000002, 0x12345678_9, 0x12345678]       # the top 8 digits equal
    ids += [0x123456789ABCDEF, 0x123456789ABCDEF0, 0x123456789ABCDEF1, 0x123456789ABCDEFF]  # the top 15
    ids += [0xFEDCBA9876543210, 0xFEDCBA987654321]                                   # 16 digits against their first 15
    out = []
    for i in ids:
        if i not in out:
            out.append(i)
    return out


# a case: W rows, n_cfgs, the task ids by position, groups [(id, config, members, task position or -1)], statuses per row (or
# None), ledger [(uid, state)] per row (or None), ranks per row; queries: [(query, the listed slots in order, totals)]
def _case(name, W, n_cfgs, tasks, groups, statuses, ledger, ranks, queries):
    return dict(name=name, W=W, n_cfgs=n_cfgs, tasks=tasks, groups=groups, statuses=statuses, ledger=ledger, ranks=ranks,
                queries=queries)


def _ledger(W, rows):
    led = [(0, NO)] * W
    for w, uid, st in rows:
        led[w] = (uid, st)
    return led


CASES = [
    _case("three_health_classes", 8, 2, [11, 12],
          [(0x100, 0, [0, 1], 0), (0xFF, 1, [2, 3, 4], -1), (0x2, 0, [5], 1)],
          [H, H, H, U, H, D, H, H], None, list(range(8)),
          [(M.query(), [0, 1, 2], (3, 6, (1, 1, 1), (0, 0, 0), 2)),
           (M.query(order=M.BY_ID_TEXT), [0, 2, 1], (3, 6, (1, 1, 1), (0, 0, 0), 2)),            # "100" < "2" < "ff"
           (M.query(order=M.BY_SIZE_DESC), [1, 0, 2], (3, 6, (1, 1, 1), (0, 0, 0), 2)),
           (M.query(health_mask=(1 << M.GH_LOST) | (1 << M.GH_DEGRADED), order=M.BY_ID_TEXT), [2, 1],
            (2, 4, (1, 1, 0), (0, 0, 0), 2)),
           (M.query(config_mask=2), [1], (1, 3, (0, 1, 0), (0, 0, 0), 2)),
           (M.query(holds=M.WITHOUT_TASK), [1], (1, 3, (0, 1, 0), (0, 0, 0), 2)),
           (M.query(size_min=2, size_max=2), [0], (1, 2, (0, 0, 1), (0, 0, 0), 2))]),
    _case("lost_beats_degraded", 4, 1, [],
          [(0x7, 0, [0, 1, 2, 3], -1)], [U, M.BANNED, DI, H], None, [3, 2, 1, 0],
          [(M.query(), [0], (1, 4, (1, 0, 0), (0, 0, 0), 1)),
           (M.query(health_mask=1 << M.GH_DEGRADED), [], (0, 0, (0, 0, 0), (0, 0, 0), 1))]),
    _case("rollout_classes", 9, 1, [11, 12, M.ALL_ONES],
          [(0xA, 0, [0, 1], 0), (0xB, 0, [2, 3], 0), (0xC, 0, [4], -1), (0xD, 0, [5, 6], 2), (0xE, 0, [7, 8], 1)],
          None, _ledger(9, [(0, 11, RUN), (1, 11, RUN), (2, 11, RUN), (3, 11, PEND), (4, 11, RUN),
                            (5, M.ALL_ONES, RUN), (6, M.ALL_ONES, RUN), (7, 11, RUN)]), list(range(9)),
          [(M.query(), [0, 1, 2, 3, 4], (5, 9, (0, 0, 0), (1, 1, 3), 1)),
           (M.query(rollout_mask=1 << M.GR_CONVERGED), [0], (1, 2, (0, 0, 0), (0, 1, 0), 1)),
           (M.query(rollout_mask=1 << M.GR_ROLLING, order=M.BY_ID_TEXT), [1, 3, 4], (3, 6, (0, 0, 0), (0, 0, 3), 1)),
           (M.query(rollout_mask=1 << M.GR_NO_TASK), [2], (1, 1, (0, 0, 0), (1, 0, 0), 1))]),
    _case("both_ledgers_and_equal_ranks", 6, 3, [21],
          [(0x10, 2, [5, 0, 3], 0), (0x1, 0, [1, 2], 0), (0x1000000000000000, 1, [4], -1)],
          [H, H, W8, H, M.EJECTED, H], _ledger(6, [(0, 21, RUN), (3, 21, RUN), (5, 21, RUN), (1, 21, RUN), (2, 22, RUN)]),
          [7, 7, 7, 7, 7, 7],
          [(M.query(order=M.BY_ID_TEXT), [1, 0, 2], (3, 6, (1, 1, 1), (1, 1, 1), 3)),          # "1" < "10" < "1000000000000000"
           (M.query(health_mask=1 << M.GH_SOUND, rollout_mask=1 << M.GR_CONVERGED), [0], (1, 3, (0, 0, 1), (0, 1, 0), 3)),
           (M.query(offset=1, limit=1), [1], (3, 6, (1, 1, 1), (1, 1, 1), 3)),
           (M.query(limit=0), [], (3, 6, (1, 1, 1), (1, 1, 1), 3))]),
    _case("no_groups", 3, 1, [5], [], [H, H, H], _ledger(3, []), [0, 1, 2],
          [(M.query(), [], (0, 0, (0, 0, 0), (0, 0, 0), 1))]),
]


def distinct_ids(n, rng):
    """n distinct ids of every text length"""
    out, seen = [], set()
    while len(out) < n:
        v = int(rng.integers(0, 1 << 63, dtype=np.uint64)) * 2 + int(rng.integers(0, 2))
        v >>= 4 * int(rng.integers(0, 16))
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out
