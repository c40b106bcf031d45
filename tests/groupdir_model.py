"""A plain model of the group directory (pm_group_directory of include/pm_engine.h), written from its definitions:

- the listed groups are the live groups in slot order that pass every filter;
- the health class is the first match of LOST (a Dead, Ejected, Banned or LowBalance member), DEGRADED (a member that is not
  Healthy), SOUND; the rollout class is NO_TASK, CONVERGED (every member reports the claimed id RUNNING; an id of all ones never
  matches) or ROLLING;
- the reference's order is `groups.sort_by(|a, b| a.id.cmp(&b.id))` over format!("{:x}", id) (node_groups/mod.rs:1040): here
  `sorted(..., key=format(id, "x"))`, a stable sort, so ties fall to the slot; `text_key` is the device's (A, L) key;
- a group's members are laid out by (addr_rank, row).

Everything is brute force over lists and dicts; nothing here knows a tile or a wave."""

STATUS_NAMES = ("Discovered", "WaitingForHeartbeat", "Healthy", "Unhealthy", "Dead", "Ejected", "Banned", "LowBalance")
DISCOVERED, WAITING, HEALTHY, UNHEALTHY, DEAD, EJECTED, BANNED, LOWBALANCE = range(8)
NS_N = 8
TS_N, TS_NONE, RUNNING = 8, 255, 2
NONE = 0xFFFFFFFF
ALL_ONES = 0xFFFFFFFFFFFFFFFF
TO_END = 0xFFFFFFFF
ANY, WITH_TASK, WITHOUT_TASK = 0, 1, 2
BY_SLOT, BY_ID_TEXT, BY_SIZE_DESC = 0, 1, 2
GH_LOST, GH_DEGRADED, GH_SOUND, GH_N, GH_NONE = 0, 1, 2, 3, 255
GR_NO_TASK, GR_CONVERGED, GR_ROLLING, GR_N, GR_NONE = 0, 1, 2, 3, 255
ALL_CLASSES = 7
ALL_CONFIGS = ALL_ONES
CONVERGED, BEHIND, OTHER, SILENT = range(4)  # a member's relation to its group's claim


def query(config_mask=ALL_CONFIGS, holds=ANY, size_min=0, size_max=NONE, health_mask=ALL_CLASSES, rollout_mask=ALL_CLASSES,
          order=BY_SLOT, offset=0, limit=TO_END):
    return dict(config_mask=config_mask, holds=holds, size_min=size_min, size_max=size_max, health_mask=health_mask,
                rollout_mask=rollout_mask, order=order, offset=offset, limit=limit)


def window(total, offset, limit):
    """-> (first, n) of the window [offset, offset + limit) over a list of `total`; offset + limit is never formed"""
    if offset >= total:
        return total, 0
    return offset, min(limit, total - offset)


def text_key(gid):
    """the device's key: (A, L), L = hex digits, A = the digits pushed to the top of 64 bits"""
    L = max(1, (gid.bit_length() + 3) // 4)
    return (gid << (4 * (16 - L))) & ALL_ONES, L


def health_of(member_statuses):
    if any(s in (DEAD, EJECTED, BANNED, LOWBALANCE) for s in member_statuses):
        return GH_LOST
    if any(s != HEALTHY for s in member_statuses):
        return GH_DEGRADED
    return GH_SOUND


def relation(report, claimed):
    """report: (uid, state) of the ledger row; claimed: the group's task id"""
    uid, st = report
    if st == TS_NONE:
        return SILENT
    if uid != claimed or uid == ALL_ONES:
        return OTHER
    return CONVERGED if st == RUNNING else BEHIND


def directory(groups, statuses, ledger, ranks, task_uids, n_cfgs, q):
    """groups: [(id, config, members, task position or -1)] the live groups in pm_get_groups order; statuses: per worker row, or
    None (liveness off); ledger: [(uid, state)] per worker row, or None (rollout off); ranks: addr_rank per row; task_uids: the
    ids of the current task list in its order.
    -> (totals, by_config, rows, members): totals = (total, members_total, by_health, by_rollout, n_cfgs); a row = (group_id,
    slot, config, size, task, member_begin, health, rollout, by_status, converged, behind, other, silent)"""
    listed = []
    for slot, (gid, cfg, mem, t) in enumerate(groups):
        by_status, rel = [0] * NS_N, [0] * 4
        health, rollout = GH_NONE, GR_NONE
        if statuses is not None:
            for w in mem:
                by_status[statuses[w]] += 1
            health = health_of([statuses[w] for w in mem])
        if ledger is not None:
            if t < 0:
                rollout = GR_NO_TASK
            else:
                for w in mem:
                    rel[relation(ledger[w], int(task_uids[t]))] += 1
                rollout = GR_CONVERGED if rel[CONVERGED] == len(mem) else GR_ROLLING
        ok = (q["config_mask"] >> cfg) & 1
        ok = ok and (q["holds"] == ANY or (q["holds"] == WITH_TASK) == (t >= 0))
        ok = ok and q["size_min"] <= len(mem) <= q["size_max"]
        ok = ok and (statuses is None or (q["health_mask"] >> health) & 1)
        ok = ok and (ledger is None or (q["rollout_mask"] >> rollout) & 1)
        if ok:
            listed.append((gid, slot, cfg, len(mem), NONE if t < 0 else t, health, rollout, tuple(by_status), *rel))
    if q["order"] == BY_ID_TEXT:
        listed.sort(key=lambda r: format(r[0], "x"))
    elif q["order"] == BY_SIZE_DESC:
        listed.sort(key=lambda r: -r[3])
    by_health, by_rollout, by_config = [0] * GH_N, [0] * GR_N, [0] * n_cfgs
    for r in listed:
        by_config[r[2]] += 1
        if r[5] != GH_NONE:
            by_health[r[5]] += 1
        if r[6] != GR_NONE:
            by_rollout[r[6]] += 1
    totals = (len(listed), sum(r[3] for r in listed), tuple(by_health), tuple(by_rollout), n_cfgs)
    first, n = window(len(listed), q["offset"], q["limit"])
    rows, members = [], []
    for r in listed[first:first + n]:
        rows.append(r[:5] + (len(members),) + r[5:])
        members += sorted(groups[r[1]][2], key=lambda w: (ranks[w], w))
    return totals, by_config, rows, members
