"""The node directory's model (tests/directory_model.py) against the reference: the comparator of NodeStore::get_nodes and the
reference's own tests (tests/golden/node_order_kats.json), so that the four-class key IS the comparator under a stable sort; the
window arithmetic at every edge; the named cases (tests/directory_cases.py)."""
import functools
import itertools
import json
import os
import random

import pytest

import directory_cases as DC
import directory_model as M

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "node_order_kats.json")))
SIGN = {"Less": -1, "Equal": 0, "Greater": 1}


def golden_cmp(a, b):
    """the reference's closure over two statuses (PM_NS_*), read from the table"""
    return SIGN[GOLDEN["comparator"][M.STATUS_NAMES[a]][M.STATUS_NAMES[b]]]


def reference_order(statuses):
    """get_nodes' sort: the store's order (here: the row index), stably sorted under the comparator"""
    return sorted(range(len(statuses)), key=functools.cmp_to_key(lambda x, y: golden_cmp(statuses[x], statuses[y])))


def test_the_table_has_every_pair_and_the_names_are_the_models():
    assert tuple(GOLDEN["statuses"]) == M.STATUS_NAMES
    assert all(set(GOLDEN["comparator"][a]) == set(M.STATUS_NAMES) for a in M.STATUS_NAMES) and len(GOLDEN["comparator"]) == M.NS_N
    for a, b in itertools.product(range(M.NS_N), repeat=2):
        ca, cb = M.status_class(a), M.status_class(b)
        assert golden_cmp(a, b) == (ca > cb) - (ca < cb), (a, b)          # the comparator IS the class order
        assert golden_cmp(a, b) == -golden_cmp(b, a)


def test_every_status_multiset_up_to_five_sorts_as_the_comparator_does():
    n = 0
    for size in range(6):
        for statuses in itertools.product(range(M.NS_N), repeat=size):    # every sequence: every multiset in every order
            assert reference_order(statuses) == M.order_of(statuses, None, M.BY_ROW), statuses
            n += 1
    assert n == sum(8 ** k for k in range(6))


def test_a_thousand_seeded_lists_sort_as_the_comparator_does():
    rng = random.Random(20)
    for k in range(1000):
        statuses = [rng.randrange(M.NS_N) for _ in range(200)]
        assert reference_order(statuses) == M.order_of(statuses, None, M.BY_ROW), k
        # BY_ADDRESS: the store's order is the rank order, the sort on top of it is the same stable sort
        ranks = [rng.randrange(50) for _ in range(200)]
        base = sorted(range(200), key=lambda w: (ranks[w], w))
        by_ref = [base[i] for i in reference_order([statuses[w] for w in base])]
        assert by_ref == M.order_of(statuses, ranks, M.BY_ADDRESS), k


def _store(nodes):
    """the golden nodes as model inputs, in insertion order: statuses, and the addresses' ranks (their order as text)"""
    statuses = [M.STATUS_NAMES.index(n["status"]) for n in nodes]
    addrs = [n["address"] for n in nodes]
    ranks = [sorted(addrs).index(a) for a in addrs]
    z = [0] * len(nodes)
    return statuses, addrs, ranks, lambda q: M.directory(statuses, z, [-1] * len(nodes), [], [], None, ranks, q)


@pytest.mark.parametrize("order", [M.BY_ROW, M.BY_ADDRESS])
def test_node_sorting_as_the_reference_tests_it(order):
    g = GOLDEN["node_sorting"]
    _, addrs, _, read = _store(g["nodes"])
    total, counts, rows = read(M.query(order=order))
    assert total == 3 and [addrs[r[0]] for r in rows] == g["expected_order"]
    assert [r[2] for r in rows] == [M.DC_HEALTHY, M.DC_DISCOVERED, M.DC_DEAD]


def test_get_uninvited_nodes_as_the_reference_tests_it():
    g = GOLDEN["get_uninvited_nodes"]
    _, addrs, _, read = _store(g["nodes"])
    total, counts, rows = read(M.query(status_mask=1 << M.DISCOVERED))
    assert [addrs[r[0]] for r in rows] == g["expected"] and total == len(g["expected"])


def test_get_nodes_route_counts_as_the_reference_builds_them():
    g = GOLDEN["get_nodes_route"]
    _, addrs, _, read = _store(g["nodes"])
    total, counts, rows = read(M.query(status_mask=M.ALL if g["include_dead"] else M.NOT_DEAD))
    assert len(rows) == g["expected_len"] and addrs[rows[0][0]] == g["nodes"][0]["address"]
    assert {M.STATUS_NAMES[s]: c for s, c in enumerate(counts) if c} == g["expected_counts"]      # (the route names present statuses only)


def test_the_window_at_every_edge():
    T = 10
    assert M.window(T, 0, 3) == (0, 3) and M.window(T, 0, T) == (0, T) and M.window(T, 0, T + 1) == (0, T)
    assert M.window(T, T, 5) == (T, 0) and M.window(T, T + 1, 5) == (T + 1, 0) and M.window(T, 0xFFFFFFFF, 0xFFFFFFFF) == (0xFFFFFFFF, 0)
    assert M.window(T, 4, 0) == (4, 0) and M.window(0, 0, 0xFFFFFFFF) == (0, 0)
    assert M.window(T, 0, 0xFFFFFFFF) == (0, T) and M.window(T, 7, 0xFFFFFFFF) == (7, 3)          # offset + limit wraps in u32
    assert M.window(T, 9, 0xFFFFFFF8) == (9, 1) and M.window(0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFF) == (0xFFFFFFFE, 1)
    for off, lim in itertools.product([0, 1, 9, 10, 11, 0xFFFFFFFF], [0, 1, 9, 10, 11, 0xFFFFFFFE, 0xFFFFFFFF]):
        first, n = M.window(T, off, lim)
        assert list(range(T))[off:off + lim] == list(range(T))[first:first + n]                    # unbounded integers agree


@pytest.mark.parametrize("case", DC.CASES, ids=[c["name"] for c in DC.CASES])
def test_the_model_on_the_named_cases(case):
    run = DC.Run(case)
    for q, total, workers in case["queries"]:
        got_total, counts, rows = run.read(q)
        assert got_total == total and [r[0] for r in rows] == workers, q
        assert sum(counts) == total and len(rows) == M.window(total, q["offset"], q["limit"])[1]
        for w, status, cls, state, counter, slot, gid, size, cfg, task, uid in rows:
            assert status == case["statuses"][w] and cls == M.status_class(status)
            assert (slot == M.NONE) == (gid == M.NONE) == (size == 0) and (slot != M.NONE or (cfg, task) == (0, M.NONE))
            if case["reports"] is None or state == M.TS_NONE:
                assert (uid, state) == (0, M.TS_NONE)


def test_the_cases_cover_what_they_are_named_for():
    names = {c["name"] for c in DC.CASES}
    assert {f"status_{n}_alone" for n in M.STATUS_NAMES} <= names
    by = {c["name"]: DC.Run(c) for c in DC.CASES}
    gone = by["a_task_deleted_under_its_group"]
    assert gone.task_uids == [12] and gone.group_of == [-1, -1, 0, 0, -1] and gone.groups[0][3] == 0
    assert gone.read(M.query())[2][0][-1] == 11                           # the reporter keeps its report
    assert by["a_group_without_a_task"].read(M.query())[2][0][9] == M.NONE
    cleared = by["rollout_on_reports_and_a_cleared_row"].read(M.query())[2]
    assert [(r[10], r[3]) for r in cleared] == [(2, 2), (1, 0), (0, M.TS_NONE), (0xFFFFFFFFFFFFFFFF, 4)]
