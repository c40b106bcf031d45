"""The model of the group directory (tests/groupdir_model.py) held to its definitions: the reference's id-text order, the
device's (A, L) key against it, the health rule over all eight statuses, the rollout class against the rollout ledger's model,
every filter alone and together, the windows, and the named cases' hand-written answers.  No GPU."""
import itertools
import random

import numpy as np
import pytest

import groupdir_cases as GC
import groupdir_model as M
import rollout_model as RM


def _text_sorted(ids):
    return sorted(ids, key=lambda x: format(x, "x"))


def test_the_edge_set_holds_what_it_promises():
    ids = GC.id_edge_set()
    assert len(set(ids)) == len(ids)
    for v in (0, 1, 0xF, 0x10, 0xFF, 0x100, (1 << 64) - 1):
        assert v in ids
    assert all(1 << (4 * k) in ids for k in range(16))
    assert format(0x100, "x") < format(0xFF, "x")                            # not numeric order


def test_the_text_key_is_the_reference_order_on_the_edge_set():
    ids = GC.id_edge_set()
    assert sorted(ids, key=M.text_key) == _text_sorted(ids)
    for a, b in itertools.permutations(ids, 2):                             # and pairwise: the key is a total order, the same one
        assert (M.text_key(a) < M.text_key(b)) == (format(a, "x") < format(b, "x")), (hex(a), hex(b))
    # the key needs its 68 bits: "1" and "1000000000000000" share A and differ in L alone, and a 16-digit id leaves no nibble
    # of A free to carry L ("1000000000000000" and "100000000000000f" differ in the lowest one)
    a, b = M.text_key(1), M.text_key(1 << 60)
    assert a[0] == b[0] and (a[1], b[1]) == (1, 16)
    assert M.text_key((1 << 60) | 0xF)[0] ^ b[0] == 0xF


def test_the_text_key_is_the_reference_order_on_random_ids():
    rng = np.random.default_rng(5)
    ids = GC.distinct_ids(3000, rng)
    assert {len(format(i, "x")) for i in ids} == set(range(1, 17))
    assert sorted(ids, key=M.text_key) == _text_sorted(ids)


def test_the_health_rule_over_all_eight_statuses():
    lost = {M.DEAD, M.EJECTED, M.BANNED, M.LOWBALANCE}
    for s in range(M.NS_N):
        want = M.GH_LOST if s in lost else M.GH_SOUND if s == M.HEALTHY else M.GH_DEGRADED
        assert M.health_of([s]) == want and M.health_of([M.HEALTHY, s, M.HEALTHY]) == want
    for a, b in itertools.product(range(M.NS_N), repeat=2):                 # first match: LOST beats DEGRADED beats SOUND
        assert M.health_of([a, b]) == min(M.health_of([a]), M.health_of([b]))
    assert M.health_of([]) == M.GH_SOUND


def _random_state(seed, W=60, n_cfgs=3):
    rnd = random.Random(seed)
    rows = list(range(W))
    rnd.shuffle(rows)
    tasks = [100 + t for t in range(4)] + [100, M.ALL_ONES]                 # a duplicate id and the id that never matches
    groups, at, ids = [], 0, GC.distinct_ids(20, np.random.default_rng(seed))
    while at < W - 10:
        n = rnd.randint(1, 5)
        groups.append((ids[len(groups)], rnd.randrange(n_cfgs), rows[at:at + n], rnd.randrange(-1, len(tasks))))
        at += n
    statuses = [rnd.randrange(M.NS_N) if rnd.random() < 0.3 else M.HEALTHY for _ in range(W)]
    ledger = [(rnd.choice(tasks + [7]), rnd.choice([M.RUNNING, M.RUNNING, 0, 5])) if rnd.random() < 0.8 else (0, M.TS_NONE)
              for _ in range(W)]
    ranks = [rnd.randrange(6) for _ in range(W)]
    return groups, statuses, ledger, ranks, tasks, n_cfgs


@pytest.mark.parametrize("seed", range(6))
def test_the_rollout_class_is_the_rollout_ledgers(seed):
    groups, statuses, ledger, ranks, tasks, n_cfgs = _random_state(seed)
    W = len(statuses)
    group_of = [-1] * W
    for s, (_, _, mem, _) in enumerate(groups):
        for w in mem:
            group_of[w] = s
    led = RM.Ledger()
    led.ingest([(w, st, uid) for w, (uid, st) in enumerate(ledger) if st != M.TS_NONE])
    ro = RM.read(W, group_of, groups, tasks, led)
    totals, _, rows, _ = M.directory(groups, statuses, ledger, ranks, tasks, n_cfgs, M.query())
    held = {r[1]: r for r in ro["groups"]}                                  # slot -> (id, slot, cfg, task, size, same, other, silent)
    assert totals[3][M.GR_CONVERGED] == ro["summary"][3] and totals[3][M.GR_NO_TASK] == len(groups) - ro["summary"][2]
    for r in rows:
        if r[1] not in held:
            assert r[7] == M.GR_NO_TASK and r[9:] == (0, 0, 0, 0)
            continue
        g = held[r[1]]
        assert (r[9], r[10], r[11], r[12]) == (g[5][M.RUNNING], sum(g[5]) - g[5][M.RUNNING], g[6], g[7])
        assert sum(r[9:]) == r[3] and (r[7] == M.GR_CONVERGED) == (g[5][M.RUNNING] == g[4])


FILTERS = [dict(config_mask=0b101), dict(holds=M.WITH_TASK), dict(holds=M.WITHOUT_TASK), dict(size_min=2, size_max=3),
           dict(health_mask=1 << M.GH_LOST), dict(health_mask=(1 << M.GH_LOST) | (1 << M.GH_DEGRADED)),
           dict(health_mask=1 << M.GH_SOUND), dict(rollout_mask=1 << M.GR_ROLLING), dict(rollout_mask=1 << M.GR_CONVERGED),
           dict(rollout_mask=1 << M.GR_NO_TASK)]


def _expect(groups, statuses, ledger, tasks, f):
    """the filter, said a second time with sets"""
    out = []
    for slot, (gid, cfg, mem, t) in enumerate(groups):
        st = {statuses[w] for w in mem}
        health = M.GH_LOST if st & {M.DEAD, M.EJECTED, M.BANNED, M.LOWBALANCE} else M.GH_SOUND if st <= {M.HEALTHY} else M.GH_DEGRADED
        conv = t >= 0 and all(ledger[w] == (tasks[t], M.RUNNING) and tasks[t] != M.ALL_ONES for w in mem)
        rollout = M.GR_NO_TASK if t < 0 else M.GR_CONVERGED if conv else M.GR_ROLLING
        if "config_mask" in f and not (f["config_mask"] >> cfg) & 1:
            continue
        if "holds" in f and (f["holds"] == M.WITH_TASK) != (t >= 0):
            continue
        if "size_min" in f and not f["size_min"] <= len(mem) <= f["size_max"]:
            continue
        if "health_mask" in f and not (f["health_mask"] >> health) & 1:
            continue
        if "rollout_mask" in f and not (f["rollout_mask"] >> rollout) & 1:
            continue
        out.append(slot)
    return out


@pytest.mark.parametrize("seed", range(4))
def test_every_filter_alone_and_together(seed):
    groups, statuses, ledger, ranks, tasks, n_cfgs = _random_state(seed)
    combos = FILTERS + [dict(a, **b) for a, b in itertools.combinations(FILTERS, 2)] + \
        [dict(config_mask=0b011, holds=M.WITH_TASK, size_min=1, size_max=4, health_mask=0b110, rollout_mask=0b110)]
    hit = 0
    for f in combos:
        for order in (M.BY_SLOT, M.BY_ID_TEXT, M.BY_SIZE_DESC):
            totals, by_config, rows, members = M.directory(groups, statuses, ledger, ranks, tasks, n_cfgs, M.query(order=order, **f))
            want = _expect(groups, statuses, ledger, tasks, f)
            if order == M.BY_ID_TEXT:
                want.sort(key=lambda s: format(groups[s][0], "x"))
            elif order == M.BY_SIZE_DESC:
                want.sort(key=lambda s: (-len(groups[s][2]), s))
            assert [r[1] for r in rows] == want, (f, order)
            assert totals[0] == len(want) and totals[1] == sum(len(groups[s][2]) for s in want) == len(members)
            assert sum(by_config) == sum(totals[2]) == sum(totals[3]) == len(want)
            at = 0
            for r in rows:                                                  # the members: laid end to end, (rank, row) order
                mem = members[r[5]:r[5] + r[3]]
                assert r[5] == at and sorted(mem) == sorted(groups[r[1]][2])
                assert [(ranks[w], w) for w in mem] == sorted((ranks[w], w) for w in mem)
                at += r[3]
            hit += bool(want)
    assert hit > len(combos)                                                # the filters are not all empty


def test_ledgers_off():
    groups, statuses, ledger, ranks, tasks, n_cfgs = _random_state(1)
    totals, _, rows, _ = M.directory(groups, None, None, ranks, tasks, n_cfgs, M.query())
    assert totals[0] == len(groups) and totals[2] == (0, 0, 0) and totals[3] == (0, 0, 0)
    assert all(r[6] == M.GH_NONE and r[7] == M.GR_NONE and not any(r[8]) and r[9:] == (0, 0, 0, 0) for r in rows)


def test_windows():
    assert M.window(10, 0, M.TO_END) == (0, 10) and M.window(10, 9, 5) == (9, 1) and M.window(10, 10, 5) == (10, 0)
    assert M.window(10, 11, 5) == (10, 0) and M.window(10, 0xFFFFFFFF, 0xFFFFFFFF) == (10, 0) and M.window(10, 3, 0) == (3, 0)
    groups, statuses, ledger, ranks, tasks, n_cfgs = _random_state(2)
    full = M.directory(groups, statuses, ledger, ranks, tasks, n_cfgs, M.query(order=M.BY_ID_TEXT))
    for off, lim in ((0, 1), (3, 4), (len(groups) - 1, 9), (len(groups), 1), (2, 0)):
        part = M.directory(groups, statuses, ledger, ranks, tasks, n_cfgs, M.query(order=M.BY_ID_TEXT, offset=off, limit=lim))
        first, n = M.window(len(groups), off, lim)
        assert part[0] == full[0] and part[1] == full[1]
        assert [r[:5] + r[6:] for r in part[2]] == [r[:5] + r[6:] for r in full[2][first:first + n]]
        assert part[3] == full[3][full[2][first][5] if n else 0:][:len(part[3])]


@pytest.mark.parametrize("case", GC.CASES, ids=[c["name"] for c in GC.CASES])
def test_named_cases(case):
    for q, slots, totals in case["queries"]:
        got = M.directory(case["groups"], case["statuses"], case["ledger"], case["ranks"], case["tasks"], case["n_cfgs"], q)
        assert [r[1] for r in got[2]] == slots and got[0] == totals, q
    if case["name"] == "both_ledgers_and_equal_ranks":                      # equal ranks: the members by row
        got = M.directory(case["groups"], case["statuses"], case["ledger"], case["ranks"], case["tasks"], case["n_cfgs"], M.query())
        assert got[3] == [0, 3, 5, 1, 2, 4] and [r[5] for r in got[2]] == [0, 3, 5]
