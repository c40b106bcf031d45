"""A plain model of the node directory (pm_directory of include/pm_engine.h): the store's ordered listing
(NodeStore::get_nodes, store/domains/node_store.rs:163-209), filtered, paged and joined with the groups and the rollout
ledger.  Lists and a sort, nothing else: tests/test_directory_model.py holds it to the reference's comparator and tests, the
GPU tests hold the engine to it."""

DISCOVERED, WAITING, HEALTHY, UNHEALTHY, DEAD, EJECTED, BANNED, LOWBALANCE, NS_N = range(9)
# NodeStatus as `{:?}` prints it (models/node.rs), in PM_NS_* order; and as sync_service.rs:220 names the gauge's label
STATUS_NAMES = ("Discovered", "WaitingForHeartbeat", "Healthy", "Unhealthy", "Dead", "Ejected", "Banned", "LowBalance")
STATUS_LOWER = tuple(n.lower() for n in STATUS_NAMES)
DC_HEALTHY, DC_DISCOVERED, DC_OTHER, DC_DEAD, DC_N = range(5)
ANY, GROUPED, UNGROUPED = 0, 1, 2
BY_ROW, BY_ADDRESS = 0, 1
NONE = 0xFFFFFFFF
TS_NONE = 255
ALL = (1 << NS_N) - 1
NOT_DEAD = ALL & ~(1 << DEAD)
TO_END = 0xFFFFFFFF


def status_class(status):
    """the four levels of the comparator at node_store.rs:195-206"""
    return {HEALTHY: DC_HEALTHY, DISCOVERED: DC_DISCOVERED, DEAD: DC_DEAD}.get(status, DC_OTHER)


def window(total, offset, limit):
    """(first, n) of the window [offset, offset + limit) over a list of `total`, in 32-bit arithmetic that never forms
    offset + limit"""
    assert 0 <= offset <= 0xFFFFFFFF and 0 <= limit <= 0xFFFFFFFF
    if offset >= total:
        return offset, 0
    return offset, min(limit, total - offset)


def query(status_mask=ALL, membership=ANY, order=BY_ROW, offset=0, limit=TO_END):
    return dict(status_mask=status_mask, membership=membership, order=order, offset=offset, limit=limit)


def order_of(statuses, addr_rank, order, listed=None):
    """the listed rows in (class, base key, row) order"""
    rows = range(len(statuses)) if listed is None else listed
    key = (lambda w: (status_class(statuses[w]), w)) if order == BY_ROW else \
          (lambda w: (status_class(statuses[w]), addr_rank[w], w))
    return sorted(rows, key=key)


def directory(statuses, counters, group_of, groups, task_uids, ledger, addr_rank, q):
    """-> (total, counts [NS_N], rows).  groups: [(id, config, members, task position or -1)] as pm_get_groups lists them,
    group_of[w] a slot of that list or -1; task_uids: the current task list's ids (a claimed position lies inside it); ledger:
    None (rollout off) or [(uid, state)] per row; a row of the result: (worker, status, cls, state, counter, group_slot,
    group_id, group_size, config, task, uid)"""
    W = len(statuses)
    assert len(counters) == W and len(group_of) == W and len(addr_rank) == W and (ledger is None or len(ledger) == W)
    assert q["status_mask"] and not q["status_mask"] >> NS_N and q["membership"] in (ANY, GROUPED, UNGROUPED)
    assert q["order"] in (BY_ROW, BY_ADDRESS)

    def listed(w):
        grouped = group_of[w] >= 0
        return bool((q["status_mask"] >> statuses[w]) & 1) and (q["membership"] == ANY or (q["membership"] == GROUPED) == grouped)

    rows = order_of(statuses, addr_rank, q["order"], [w for w in range(W) if listed(w)])
    total = len(rows)
    counts = [0] * NS_N
    for w in rows:
        counts[statuses[w]] += 1
    first, n = window(total, q["offset"], q["limit"])
    out = []
    for w in rows[first:first + n]:
        s = group_of[w]
        if s >= 0:
            gid, cfg, mem, t = groups[s]
            assert w in mem and t < len(task_uids)
            grp = (s, gid, len(mem), cfg, NONE if t < 0 else t)
        else:
            grp = (NONE, NONE, 0, 0, NONE)
        uid, state = (0, TS_NONE) if ledger is None else ledger[w]
        out.append((w, statuses[w], status_class(statuses[w]), state, counters[w]) + grp + (uid,))
    return total, counts, out
