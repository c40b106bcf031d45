"""A plain model of pm_task_directory (include/pm_engine.h), written from the header's definitions and from nothing else: no
numpy, no engine.  tests/test_taskdir_model.py holds it to the definitions; tests/test_gpu_taskdir.py compares the engine with it.

Inputs: groups = [(id, config, members, task position or -1)] as pm_get_groups reports them; ledger = [(uid, state)] per worker
row, state TS_NONE = no report, or None: the rollout ledger is off; tasks = [(uid, created_at, topo_mask)] in the caller's CURRENT
list order; n_cfgs; a query (query())."""
NONE = 0xFFFFFFFF
ALL_ONES = 0xFFFFFFFFFFFFFFFF
TO_END = 0xFFFFFFFF
TS_N, TS_RUNNING, TS_NONE = 8, 2, 255
BY_LIST, BY_OLDEST, BY_WORKERS_DESC, BY_REPORTERS_DESC = 0, 1, 2, 3
TKS_RUNNING, TKS_WAITING, TKS_STARVED, TKS_N = 0, 1, 2, 3
TKR_UNHELD, TKR_CONVERGED, TKR_ROLLING, TKR_N, TKR_NONE = 0, 1, 2, 3, 255
ALL_SERVE, ALL_ROLLOUT = (1 << TKS_N) - 1, (1 << TKR_N) - 1


def query(config_mask=ALL_ONES, serve_mask=ALL_SERVE, rollout_mask=ALL_ROLLOUT, workers_min=0, workers_max=NONE, order=BY_LIST,
          offset=0, limit=TO_END):
    return dict(config_mask=config_mask, serve_mask=serve_mask, rollout_mask=rollout_mask, workers_min=workers_min,
                workers_max=workers_max, order=order, offset=offset, limit=limit)


def member_converged(report, claimed):
    """PM_RO_CONVERGED: the member reports the claimed id, running; an id of all ones never matches"""
    uid, state = report
    return state < TS_N and uid == claimed and uid != ALL_ONES and state == TS_RUNNING


def first_rows(tasks):
    """id -> the FIRST position of the list that carries it; an id of all ones names no task"""
    first = {}
    for t, (uid, _, _) in enumerate(tasks):
        if uid != ALL_ONES and uid not in first:
            first[uid] = t
    return first


def joined(groups, ledger, tasks, n_cfgs):
    """every task's row as a tuple in pm_tdir_row's field order (without the padding), and (orphan_uids, orphan_reporters)"""
    T, valid = len(tasks), (1 << n_cfgs) - 1
    per_cfg = [0] * n_cfgs
    running, workers, hold_conv = [0] * T, [0] * T, [0] * T
    by_id = {}   # id -> [groups_converged, converged, reporters[TS_N]]: pm_rollout_tasks' row of the id
    for _, cfg, members, t in groups:
        per_cfg[cfg] += 1
        if t < 0:
            continue
        running[t] += 1
        workers[t] += len(members)
        if ledger is not None:
            claimed = tasks[t][0]
            conv = sum(member_converged(ledger[w], claimed) for w in members)
            row = by_id.setdefault(claimed, [0, 0, [0] * TS_N])
            row[0] += conv == len(members)
            row[1] += conv
            hold_conv[t] += conv == len(members)
    if ledger is not None:
        for uid, state in ledger:
            if state < TS_N:
                by_id.setdefault(uid, [0, 0, [0] * TS_N])[2][state] += 1
    first = first_rows(tasks)
    reported = [[0, 0, [0] * TS_N] for _ in range(T)]
    orphan_uids = orphan_reporters = 0
    for uid, row in by_id.items():
        if uid in first:
            reported[first[uid]] = row
        else:
            orphan_uids += 1
            orphan_reporters += sum(row[2])
    rows = []
    for t, (uid, created_at, mask) in enumerate(tasks):
        allowed = sum(per_cfg[c] for c in range(n_cfgs) if (mask & valid) >> c & 1)
        serve = TKS_RUNNING if running[t] else TKS_WAITING if allowed else TKS_STARVED
        rollout = TKR_NONE if ledger is None else TKR_UNHELD if not running[t] else \
            TKR_CONVERGED if hold_conv[t] == running[t] else TKR_ROLLING
        rows.append((uid, created_at, mask, t, allowed, running[t], workers[t], reported[t][0], reported[t][1],
                     tuple(reported[t][2]), serve, rollout))
    return rows, (orphan_uids, orphan_reporters)


def directory(groups, ledger, tasks, n_cfgs, q):
    """-> (totals, by_config, rows): totals = (tasks, total, by_serve, by_rollout, unrestricted, workers_running, reporters,
    orphan_uids, orphan_reporters, n_cfgs); rows = the window's"""
    valid = (1 << n_cfgs) - 1
    rows, orphans = joined(groups, ledger, tasks, n_cfgs)
    listed = []
    for r in rows:
        mask, w, serve, rollout = r[2], r[6], r[10], r[11]
        if q["config_mask"] != ALL_ONES and not (mask & valid & q["config_mask"]):
            continue
        if not (q["serve_mask"] >> serve) & 1:
            continue
        if ledger is not None and not (q["rollout_mask"] >> rollout) & 1:
            continue
        if not q["workers_min"] <= w <= q["workers_max"]:
            continue
        listed.append(r)
    by_serve, by_rollout = [0] * TKS_N, [0] * TKR_N
    by_config = [0] * n_cfgs
    for r in listed:
        by_serve[r[10]] += 1
        if ledger is not None:
            by_rollout[r[11]] += 1
        for c in range(n_cfgs):
            by_config[c] += (r[2] >> c) & 1
    totals = (len(tasks), len(listed), tuple(by_serve), tuple(by_rollout), sum(r[2] == ALL_ONES for r in listed),
              sum(r[6] for r in listed), sum(sum(r[9]) for r in listed), orphans[0], orphans[1], n_cfgs)
    order = q["order"]
    if order == BY_OLDEST:
        listed = listed[::-1]
    elif order == BY_WORKERS_DESC:
        listed = sorted(listed, key=lambda r: (-r[6], r[3]))
    elif order == BY_REPORTERS_DESC:
        listed = sorted(listed, key=lambda r: (-sum(r[9]), r[3]))
    n = 0 if q["offset"] >= len(listed) else min(q["limit"], len(listed) - q["offset"])
    return totals, by_config, listed[q["offset"]:q["offset"] + n]
