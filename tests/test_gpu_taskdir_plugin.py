"""The C++ plugin over the real engine: GpuMatchPlugin's task directory methods through pm_plugin_c.h (pmx_list_tasks,
pmx_task_counts, pmx_starved_tasks, pmx_orchestrator_statistics) on a 300-node swarm behind a tick and a short replay: new tasks
in front, reports, a deleted task.  Every listing, page by page and in every order, the counters and the statistics are the model's
(tests/taskdir_model.py) over the engine's other reads and the plugin's own task list."""
import ctypes as C

import pytest

from protocol_amd.swarm import make_swarm

from helpers import engine_groups
from plugin_cxx import PluginCxx, _check, _text, plugin_lib, uuid_of

import taskdir_model as M

pytestmark = pytest.mark.gpu
NOW = 1_760_000_000_000
ALL64, TO_END = 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF
SERVE, ROLLOUT = ("running", "waiting", "starved"), ("unheld", "converged", "rolling")
STRANGER = "a-task-nobody-lists"


def bind(L):
    vp, sz, s, u32, u64 = C.c_void_p, C.c_size_t, C.c_char_p, C.c_uint32, C.c_uint64
    L.pmx_enable_liveness.argtypes = [vp, u32]
    L.pmx_enable_rollout.argtypes = [vp]
    L.pmx_report_task.argtypes = [vp, s, s, s]
    L.pmx_flush_rollout.argtypes = [vp]
    L.pmx_list_tasks.argtypes = [vp, u64, u32, u32, u32, u32, u32, u32, u32, s, sz, C.POINTER(sz)]
    L.pmx_task_counts.argtypes = [vp, s, sz, C.POINTER(sz)]
    L.pmx_starved_tasks.argtypes = [vp, s, sz, C.POINTER(sz)]
    L.pmx_orchestrator_statistics.argtypes = [vp, s, sz, C.POINTER(sz)]
    return L


def list_tasks(p, q):
    text = _text(lambda o, c, n: p.L.pmx_list_tasks(p._p, q["config_mask"], q["serve_mask"], q["rollout_mask"], q["workers_min"],
                                                    q["workers_max"], q["order"], q["offset"], q["limit"], o, c, n))
    head, _, rest = text.partition("\n")
    tag, total, tasks = head.split("\t")
    assert tag == "total"
    return int(total), int(tasks), rest


def _lines(rows):
    return "".join("%s\ttask\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\n" % (uuid_of(r[0]), SERVE[r[10]], ROLLOUT[r[11]] if r[11] < 3 else "-", r[4], r[5],
                                                                    r[6], r[7], r[8], sum(r[9])) for r in rows)


def _state(p, tasks, ro):
    ledger = None
    if ro:
        uid, state = p.eng.rollout_get()
        ledger = list(zip(uid.tolist(), state.tolist()))
    return engine_groups(p.eng), ledger, list(tasks), len(p.config_names)


def _check_everything(p, tasks, ro, tag):
    orders = (M.BY_LIST, M.BY_OLDEST, M.BY_WORKERS_DESC) + ((M.BY_REPORTERS_DESC,) if ro else ())
    queries = [M.query(order=o) for o in orders] + [M.query(serve_mask=1 << M.TKS_STARVED), M.query(config_mask=2, workers_min=1, order=M.BY_WORKERS_DESC),
                                                    M.query(order=orders[-1], offset=3, limit=7)]
    if ro:
        queries += [M.query(rollout_mask=(1 << M.TKR_CONVERGED) | (1 << M.TKR_ROLLING), order=M.BY_REPORTERS_DESC)]
    got = [list_tasks(p, q) for q in queries]
    starved = _text(lambda o, c, n: p.L.pmx_starved_tasks(p._p, o, c, n))
    counts = _text(lambda o, c, n: p.L.pmx_task_counts(p._p, o, c, n))
    state = _state(p, tasks, ro)                                # (behind the directory: pm_get_groups compacts the group list)
    for q, g in zip(queries, got):
        totals, _, rows = M.directory(*state, q)
        assert g == (totals[1], totals[0], _lines(rows)), (tag, q)
    t, by_config, rows = M.directory(*state, M.query())
    assert starved == _lines([r for r in rows if r[10] == M.TKS_STARVED]), tag
    want = "tasks\t%d\nserve\t%d\t%d\t%d\nrollout\t%d\t%d\t%d\nunrestricted\t%d\nworkers_running\t%d\nreporters\t%d\norphans\t%d\t%d\n" % (
        t[0], *t[2], *t[3], t[4], t[5], t[6], t[7], t[8])
    want += "".join("%s\t%d\n" % kv for kv in sorted((p.config_names[c], n) for c, n in enumerate(by_config) if n))
    assert counts == want, tag
    # page by page, in the list's order
    joined = ""
    for off in range(0, t[1] + 9, 9):
        total, n_tasks, part = list_tasks(p, M.query(offset=off, limit=9))
        assert (total, n_tasks) == (t[1], t[0]) and part.count("\n") == max(0, min(9, t[1] - off))
        joined += part
    assert joined == _lines(rows), tag
    return state, rows, t


def test_the_task_directory_over_a_ticked_swarm():
    sw = make_swarm(43, 120, 300)
    W = sw.W
    bind(plugin_lib())
    p = PluginCxx(sw)
    p.set_clock(NOW)
    p.sync_nodes(range(W), set(range(W)))
    masks, created, uids = sw.task_masks(), sw.created_at, sw.task_uid
    p.sync_tasks(masks, created, uids)
    p.eng.W = W
    tasks = list(zip([int(u) for u in uids], [int(c) for c in created], [int(m) for m in masks]))
    p.tick()
    # the rollout ledger off: the listing works, the rows name no rollout class, a rollout filter and the order by reporters are refused
    state, rows, t = _check_everything(p, tasks, False, "rollout off")
    assert len(state[0]) > 20 and t[2][M.TKS_RUNNING] > 0 and {r[11] for r in rows} == {M.TKR_NONE}
    with pytest.raises(RuntimeError):
        list_tasks(p, M.query(rollout_mask=1 << M.TKR_ROLLING))
    with pytest.raises(RuntimeError):
        list_tasks(p, M.query(order=M.BY_REPORTERS_DESC))
    _check(p.L.pmx_enable_liveness(p._p, 3))
    _check(p.L.pmx_enable_rollout(p._p))
    state, rows, t = _check_everything(p, tasks, True, "nobody reports")
    assert t[3][M.TKR_CONVERGED] == 0 and t[3][M.TKR_ROLLING] == t[2][M.TKS_RUNNING] and t[6] == 0
    # the members of every other group that holds a task report it running; three nodes report a task nobody lists
    addr_of = [a.decode() for a in p.addr]
    held = [g for g in state[0] if g[3] >= 0]
    for g in held[::2]:
        for w in g[2]:
            _check(p.L.pmx_report_task(p._p, addr_of[w].encode(), uuid_of(tasks[g[3]][0]).encode(), b"RUNNING"))
    free = [w for w in range(W) if not any(w in g[2] for g in state[0])][:3]
    assert len(free) == 3
    for w in free:
        _check(p.L.pmx_report_task(p._p, addr_of[w].encode(), STRANGER.encode(), b"FAILED"))
    _check(p.L.pmx_flush_rollout(p._p))
    state, rows, t = _check_everything(p, tasks, True, "reported")
    assert t[3][M.TKR_CONVERGED] > 0 and t[7:9] == (1, 3) and t[6] == sum(len(g[2]) for g in held[::2])
    # a short replay: two new tasks in front, a tick, a held task deleted under its reporters
    for k in range(2):
        uid = 0x7000_0000_0000_0100 + k
        p.on_task_created(ALL64 if k else 1, int(created[0]) + 10 + k, uid)
        tasks.insert(0, (uid, int(created[0]) + 10 + k, ALL64 if k else 1))
    p.tick()
    _check_everything(p, tasks, True, "new tasks in front")
    victim = tasks[held[0][3] + 2]                              # (the positions moved by the two new rows)
    p.on_task_deleted(victim[0])
    tasks.remove(victim)
    state, rows, t = _check_everything(p, tasks, True, "a held task deleted")
    assert t[7] == 2 and t[8] == 3 + sum(len(g[2]) for g in held[::2] if g[3] == held[0][3])  # its reporters report an orphan now
    # what sync_orchestrator_statistics sets: present statuses, tasks_count, nodes_per_task with names, groups per configuration
    stats = _text(lambda o, c, n: p.L.pmx_orchestrator_statistics(p._p, o, c, n))
    state = _state(p, tasks, True)
    per_id = {}
    for uid, st in state[1]:
        if st < M.TS_N:
            per_id[uid] = per_id.get(uid, 0) + 1
    listed = {u for u, _, _ in tasks}
    strangers = [u for u in per_id if u not in listed]
    assert len(strangers) == 2
    text_of = {u: (uuid_of(u) if u == victim[0] else STRANGER) for u in strangers}
    groups = {}
    for g in state[0]:
        groups[p.config_names[g[1]]] = groups.get(p.config_names[g[1]], 0) + 1
    want = "nodes\thealthy\t%d\ntasks_count\t%d\n" % (W, len(tasks))
    want += "".join("nodes_per_task\t%s\t%s\t%d\n" % ((uuid_of(u), "task", n) if u in listed else (text_of[u], "unknown", n))
                    for u, n in sorted(per_id.items()))
    want += "".join("groups_count\t%s\t%d\n" % kv for kv in sorted(groups.items()))
    assert stats == want
    p.close()
