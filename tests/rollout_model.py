"""A plain model of the rollout ledger (pm_rollout_* of include/pm_engine.h), written from the reference's lines:

- `Store` is the three task fields NodeStore::update_node_task keeps per address (node_store.rs:339-377): both task_id and
  task_state present sets them (the state through TaskState::from, task.rs:24-37), anything else clears all three;
- `nodes_per_task` counts node.task_id the way the sync service does (metrics/sync_service.rs:243-267), named through the task
  list or "unknown";
- `Ledger` is the numeric face of the same record (an id and a state per worker row, last report wins), and `read` makes the
  classes and the three tables by brute force over dicts from the groups, the current task ids and the ledger."""
from collections import OrderedDict

TS_NAMES = ("PENDING", "PULLING", "RUNNING", "COMPLETED", "FAILED", "PAUSED", "RESTARTING", "UNKNOWN")
PENDING, PULLING, RUNNING, COMPLETED, FAILED, PAUSED, RESTARTING, UNKNOWN = range(8)
TS_N, TS_NONE = 8, 255
IDLE, STRAY, SILENT, OTHER, BEHIND, CONVERGED = range(6)
RO_N = 6
NONE = 0xFFFFFFFF
ALL_ONES = 0xFFFFFFFFFFFFFFFF


def task_state_from(s) -> int:
    """TaskState::from(&str): a match on the exact text; `"UNKNOWN" | &_` for everything else"""
    return TS_NAMES.index(s) if s in TS_NAMES else UNKNOWN


class Store:
    """address -> {task_id, task_state, task_details}: only update_node_task writes these fields"""

    def __init__(self):
        self.nodes = OrderedDict()

    def add_node(self, address):
        self.nodes.setdefault(address, {})

    def update_node_task(self, address, current_task, task_state, task_details=None):
        rec = self.nodes.setdefault(address, {})
        if current_task is not None and task_state is not None:  # (Some(task), Some(state), details)
            rec["task_id"] = current_task
            rec["task_state"] = TS_NAMES[task_state_from(task_state)]
            if task_details is not None:
                rec["task_details"] = task_details
            else:
                rec.pop("task_details", None)
        else:  # _ => hdel task_id, task_state, task_details
            for k in ("task_id", "task_state", "task_details"):
                rec.pop(k, None)

    def record(self, address):
        rec = self.nodes.get(address, {})
        return rec.get("task_id"), rec.get("task_state"), rec.get("task_details")


def nodes_per_task(store: Store, tasks) -> list:
    """tasks: [(id text, name)].  -> sorted [(task id text, task name or "unknown", count)] (the reference's order is a HashMap's)"""
    names = {tid: name for tid, name in tasks}
    counts = {}
    for rec in store.nodes.values():
        if rec.get("task_id") is not None:
            counts[rec["task_id"]] = counts.get(rec["task_id"], 0) + 1
    return sorted((tid, names.get(tid, "unknown"), n) for tid, n in counts.items())


class Ledger:
    """worker -> (uid, state); an absent worker reports nothing"""

    def __init__(self):
        self.rows = {}

    def ingest(self, reports):
        """reports: [(worker, state, uid)] in order; TS_NONE clears"""
        for w, st, uid in reports:
            if st == TS_NONE:
                self.rows.pop(w, None)
            else:
                assert 0 <= st < TS_N
                self.rows[w] = (uid, st)

    def clear(self):
        self.rows.clear()

    def get(self, idx):
        return [self.rows.get(w, (0, TS_NONE)) for w in idx]


def read(W, group_of, groups, task_uids, led: Ledger) -> dict:
    """group_of: slot or -1 per worker; groups: [(id, config, members, task position or -1)] in pm_get_groups order;
    task_uids: the ids of the current list in its order.  -> summary, tasks, groups, workers as plain tuples"""
    first_pos = {}
    for p, u in enumerate(task_uids):
        first_pos.setdefault(int(u), p)
    claimed = {}  # slot -> uid
    for s, (_gid, _cfg, _mem, t) in enumerate(groups):
        if t >= 0:
            claimed[s] = int(task_uids[t])
    cls, workers = [], []
    for w in range(W):
        s = int(group_of[w])
        rep = led.rows.get(w)
        if s < 0 or s not in claimed:
            c = STRAY if rep else IDLE
        elif rep is None:
            c = SILENT
        elif rep[0] != claimed[s] or rep[0] == ALL_ONES:
            c = OTHER
        else:
            c = CONVERGED if rep[1] == RUNNING else BEHIND
        cls.append(c)
        uid, st = rep if rep else (0, TS_NONE)
        workers.append((w, NONE if s < 0 else s, uid, c, st))
    group_rows, conv_of = [], {}
    for s, (gid, cfg, mem, t) in enumerate(groups):
        if s not in claimed:
            continue
        same, other, silent = [0] * TS_N, 0, 0
        for w in mem:
            if cls[w] == SILENT:
                silent += 1
            elif cls[w] == OTHER:
                other += 1
            else:
                same[led.rows[w][1]] += 1
        assert sum(same) + other + silent == len(mem)
        conv_of[s] = same[RUNNING]
        group_rows.append((gid, s, cfg, t, len(mem), tuple(same), other, silent))
    ids = set(claimed.values()) | {u for u, _ in led.rows.values()}
    task_rows = []
    for u in sorted(ids):
        reporters = [0] * TS_N
        for uid, st in led.rows.values():
            if uid == u:
                reporters[st] += 1
        slots = [s for s, cu in claimed.items() if cu == u]
        task_rows.append((u, NONE if u == ALL_ONES else first_pos.get(u, NONE), len(slots),
                          sum(conv_of[s] == len(groups[s][2]) for s in slots), sum(len(groups[s][2]) for s in slots),
                          sum(conv_of[s] for s in slots), tuple(reporters)))
    by_state = [0] * (TS_N + 1)
    for w in range(W):
        by_state[led.rows[w][1] if w in led.rows else TS_N] += 1
    summary = (tuple(cls.count(c) for c in range(RO_N)), tuple(by_state), len(claimed),
               sum(conv_of[s] == len(groups[s][2]) for s in claimed), len(task_rows))
    return dict(summary=summary, tasks=task_rows, groups=group_rows, workers=workers)
