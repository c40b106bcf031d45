"""tests/taskdir_model.py held to the definitions of include/pm_engine.h ("task directory") without a GPU: the hand-made answers
of tests/taskdir_cases.py, and — on the same cases and on random tables — brute-force restatements of what the header documents
for pm_task_report (three columns per list position) and for pm_rollout_tasks (one row per distinct claimed or reported id),
written here a second time with other loops."""
import random

import pytest

import taskdir_cases as TC
import taskdir_model as M


def task_report(groups, tasks, n_cfgs):
    """pm_task_report's documented columns: live groups that hold the task, their workers, live groups whose configuration the
    task's topologies allow"""
    running = [sum(1 for g in groups if g[3] == t) for t in range(len(tasks))]
    workers = [sum(len(g[2]) for g in groups if g[3] == t) for t in range(len(tasks))]
    allowed = [sum(1 for g in groups if g[1] < n_cfgs and (tasks[t][2] >> g[1]) & 1) for t in range(len(tasks))]
    return running, workers, allowed


def rollout_tasks(groups, ledger, tasks):
    """pm_rollout_tasks' documented rows, ascending by uid: (uid, task, groups, groups_converged, assigned, converged, reporters)"""
    ids = {tasks[g[3]][0] for g in groups if g[3] >= 0} | {uid for uid, st in ledger if st < M.TS_N}
    out = []
    for uid in sorted(ids):
        holders = [g for g in groups if g[3] >= 0 and tasks[g[3]][0] == uid]
        conv_of = lambda g: sum(1 for w in g[2] if uid != M.ALL_ONES and ledger[w] == (uid, M.TS_RUNNING))
        position = next((t for t, task in enumerate(tasks) if task[0] == uid), M.NONE) if uid != M.ALL_ONES else M.NONE
        out.append((uid, position, len(holders), sum(1 for g in holders if conv_of(g) == len(g[2])), sum(len(g[2]) for g in holders),
                    sum(conv_of(g) for g in holders), tuple(sum(1 for r in ledger if r == (uid, s)) for s in range(M.TS_N))))
    return out


def held_to_the_reports(groups, ledger, tasks, n_cfgs):
    rows, orphans = M.joined(groups, ledger, tasks, n_cfgs)
    running, workers, allowed = task_report(groups, tasks, n_cfgs)
    assert [r[5] for r in rows] == running and [r[6] for r in rows] == workers and [r[4] for r in rows] == allowed
    assert [r[:4] for r in rows] == [(u, c, m, t) for t, (u, c, m) in enumerate(tasks)]
    if ledger is None:
        assert all(r[7:10] == (0, 0, (0,) * M.TS_N) and r[11] == M.TKR_NONE for r in rows) and orphans == (0, 0)
        return
    ro = rollout_tasks(groups, ledger, tasks)
    by_task = {r[1]: r for r in ro if r[1] != M.NONE}
    for r in rows:
        want = by_task.get(r[3])
        assert r[7:10] == ((want[3], want[5], want[6]) if want else (0, 0, (0,) * M.TS_N)), r
    lost = [r for r in ro if r[1] == M.NONE]
    assert orphans == (len(lost), sum(sum(r[6]) for r in lost))
    # reporters sum to the reference's nodes_per_task: every reporting row is counted once, on a task or as an orphan
    assert sum(sum(r[9]) for r in rows) + orphans[1] == sum(1 for _, st in ledger if st < M.TS_N)
    for r in rows:  # the classes, from the definitions
        holders = [g for g in groups if g[3] == r[3]]
        serve = M.TKS_RUNNING if holders else M.TKS_WAITING if r[4] else M.TKS_STARVED
        conv = [all(M.member_converged(ledger[w], r[0]) for w in g[2]) for g in holders]
        rollout = M.TKR_UNHELD if not holders else M.TKR_CONVERGED if all(conv) else M.TKR_ROLLING
        assert (r[10], r[11]) == (serve, rollout), r


@pytest.mark.parametrize("case", TC.CASES, ids=[c["name"] for c in TC.CASES])
def test_named_cases(case):
    state = (case["groups"], case["ledger"], case["tasks"], case["n_cfgs"])
    held_to_the_reports(*state)
    for q, positions, totals in case["queries"]:
        got = M.directory(*state, q)
        assert [r[3] for r in got[2]] == positions, q
        if totals is not None:
            assert got[0] == totals, q
        assert got[0][0] == len(case["tasks"]) and got[0][9] == case["n_cfgs"] and len(got[1]) == case["n_cfgs"]


def test_the_named_cases_cover_what_the_issue_names():
    rows, orphans = M.joined(TC.GROUPS, TC.LEDGER, TC.TASKS, 3)
    assert {r[10] for r in rows} == {0, 1, 2} and {r[11] for r in rows} == {0, 1, 2}           # every class of both kinds
    assert any(r[2] == 0 for r in rows) and any(r[2] == M.ALL_ONES for r in rows) and any(r[0] == M.ALL_ONES for r in rows)
    assert rows[0][5] == 2 and rows[0][7] == 1 and rows[0][11] == M.TKR_ROLLING                # two holders, one converged
    assert rows[1][0] == rows[4][0] and sum(rows[1][9]) == 2 and sum(rows[4][9]) == 0          # the duplicate: the first row is credited
    assert rows[4][5] == 1 and rows[4][11] == M.TKR_CONVERGED and rows[1][7] == 1              # ... the classes go by the row held
    assert orphans == (2, 4)
    names = {c["name"] for c in TC.CASES}
    assert len(names) == len(TC.CASES) and {"rollout_off", "orders_with_ties", "windows", "filters_combined"} <= names
    orders = {q["order"] for c in TC.CASES for q, _, _ in c["queries"]}
    assert orders == {M.BY_LIST, M.BY_OLDEST, M.BY_WORKERS_DESC, M.BY_REPORTERS_DESC}


def test_the_definitions_on_random_tables():
    rng = random.Random(5)
    for trial in range(60):
        n_cfgs, T, W = rng.randint(1, 5), rng.randint(0, 12), rng.randint(0, 30)
        ids = [rng.choice([1, 2, 3, 4, 5, 6, M.ALL_ONES]) for _ in range(T)]
        tasks = [(ids[t], 100 - t, rng.choice([0, M.ALL_ONES, rng.getrandbits(n_cfgs + 1)])) for t in range(T)]
        groups, at = [], 0
        while at < W and rng.random() < 0.8:
            n = rng.randint(1, min(4, W - at))
            groups.append((1000 + at, rng.randrange(n_cfgs), list(range(at, at + n)), rng.randrange(-1, T) if T else -1))
            at += n
        ledger = [(rng.choice([1, 2, 3, 9, M.ALL_ONES]), rng.choice([M.TS_RUNNING, M.TS_RUNNING, 0, 4, M.TS_NONE])) for _ in range(W)]
        ledger = [(0, M.TS_NONE) if st == M.TS_NONE else (u, st) for u, st in ledger]
        for led in (ledger, None):
            held_to_the_reports(groups, led, tasks, n_cfgs)
            full = M.directory(groups, led, tasks, n_cfgs, M.query())
            assert [r[3] for r in full[2]] == list(range(T)) and full[0][1] == T
            for order in range(4):
                q = M.query(config_mask=rng.getrandbits(6) | 1, serve_mask=rng.randint(1, 7), workers_max=rng.randint(0, 6), order=order)
                whole = M.directory(groups, led, tasks, n_cfgs, q)
                assert whole[0][1] == len(whole[2]) and sum(whole[0][2]) == len(whole[2])
                assert whole[0][5] == sum(r[6] for r in whole[2]) and whole[0][6] == sum(sum(r[9]) for r in whole[2])
                keys = [(r[3] if order == 0 else -r[3] if order == 1 else (-r[6], r[3]) if order == 2 else (-sum(r[9]), r[3]))
                        for r in whole[2]]
                assert keys == sorted(keys)                                  # the order, ties by ascending position
                # any window is a slice of the whole list, and the totals do not depend on it
                off, lim = rng.randint(0, T + 1), rng.choice([0, 1, 3, M.TO_END])
                part = M.directory(groups, led, tasks, n_cfgs, dict(q, offset=off, limit=lim))
                assert part[0] == whole[0] and part[1] == whole[1] and part[2] == whole[2][off:off + min(lim, max(len(whole[2]) - off, 0))]
