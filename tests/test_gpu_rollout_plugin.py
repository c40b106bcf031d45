"""The C++ plugin over the real engine: GpuMatchPlugin's rollout methods through pm_plugin_c.h (pmx_report_task & co.) on one
churned swarm of about 2,000 nodes — heartbeats' task fields as texts (task ids of the list, ids no task carries, states in the
wrong case, cleared fields), with ticks, deaths, a deleted and a created task between the rounds.  After every round the plugin's
reads equal the model of tests/rollout_model.py: the store's three fields per address for nodes_per_task, and the classes and
tables over what pm_get_groups reports at that moment."""
import ctypes as C
import random

import numpy as np
import pytest

from protocol_amd import engine as E
from protocol_amd.swarm import make_swarm
from helpers import engine_groups

import rollout_model as M
from plugin_cxx import PluginCxx, _check, _text, plugin_lib, uid_of, uuid_of

pytestmark = pytest.mark.gpu
ALL = (1 << M.RO_N) - 1


def bind(L):
    vp, sz, s = C.c_void_p, C.c_size_t, C.c_char_p
    L.pmx_enable_rollout.argtypes = [vp]
    L.pmx_report_task.argtypes = [vp, s, s, s]
    L.pmx_flush_rollout.argtypes = [vp]
    L.pmx_nodes_per_task.argtypes = [vp, s, sz, C.POINTER(sz)]
    L.pmx_rollout_summary.argtypes = [vp, vp]
    L.pmx_task_rollout.argtypes = [vp, s, sz, C.POINTER(sz)]
    L.pmx_group_rollout.argtypes = [vp, s, sz, C.POINTER(sz)]
    L.pmx_rollout_nodes.argtypes = [vp, C.c_uint32, s, sz, C.POINTER(sz)]
    return L


def reported_uid(text: str) -> int:
    """GpuMatchPlugin::reported_task_uid: the low 64 bits of a UUID text, else FNV-1a of the bytes"""
    t = text.replace("-", "")
    if (len(text) == 32 or (len(text) == 36 and [i for i, c in enumerate(text) if c == "-"] == [8, 13, 18, 23])) and len(t) == 32 and \
            all(c in "0123456789abcdefABCDEF" for c in t):
        return uid_of(text)
    h = 0xCBF29CE484222325
    for c in text.encode():
        h = ((h ^ c) * 0x100000001B3) & M.ALL_ONES
    return h


def test_reported_uid_is_the_plugins():
    assert reported_uid(uuid_of(0xFEDCBA9876543210)) == 0xFEDCBA9876543210 and reported_uid("a") == 0xAF63DC4C8601EC8C
    assert reported_uid("") == 0xCBF29CE484222325


def _lines(text):
    return [ln.split("\t") for ln in text.splitlines()]


def test_a_churned_swarm_through_the_c_face():
    sw = make_swarm(61, 60, 2000)
    W = sw.W
    bind(plugin_lib())
    p = PluginCxx(sw)
    p.sync_nodes(range(W), set(range(W)))
    p.sync_tasks(sw.task_masks(), sw.created_at, sw.task_uid)
    p.eng.W = W
    with pytest.raises(RuntimeError):                           # the ledger is off: the flush reports the engine's refusal
        _check(p.L.pmx_report_task(p._p, p.addr[0], uuid_of(1).encode(), b"RUNNING"))
        _check(p.L.pmx_flush_rollout(p._p))
    _check(p.L.pmx_enable_rollout(p._p))
    addr = [a.decode() for a in p.addr]
    row_of, addr_of_row = {}, {}
    for node in range(W):
        row = C.c_uint32(0)
        _check(p.L.pmx_row_of(p._p, p.addr[node], C.byref(row)))
        row_of[addr[node]] = row.value
        addr_of_row[row.value] = addr[node]
    store, led = M.Store(), M.Ledger()
    texts = {}                                                  # id -> the text it was first reported with
    for a in addr:
        store.add_node(a)
    rng = random.Random(9)
    healthy = set(range(W))
    states = list(M.TS_NAMES) + ["running", "Failed", ""]
    side = ["side-job-%d" % k for k in range(5)] + [uuid_of(0x7777000000000000 + k) for k in range(3)]

    def report(a, task, state):
        _check(p.L.pmx_report_task(p._p, a.encode(), None if task is None else task.encode(), None if state is None else state.encode()))
        store.update_node_task(a, task, state)
        if task is not None and state is not None:
            uid = reported_uid(task)
            texts.setdefault(uid, task)
            led.ingest([(row_of[a], M.task_state_from(state), uid)])
        else:
            led.ingest([(row_of[a], M.TS_NONE, 0)])

    def wave(share):
        gow, groups, _ = p.eng.get_groups()
        for a in rng.sample(addr, int(share * W)):
            g = gow[row_of[a]]
            t = int(groups[g]["task"]) if g >= 0 else M.NONE
            r = rng.random()
            if t != M.NONE and r < 0.7:
                report(a, uuid_of(p.tasks[t]), "RUNNING" if r < 0.6 else rng.choice(states))
            elif r < 0.8:
                report(a, uuid_of(rng.choice(p.tasks)), rng.choice(states))
            elif r < 0.9:
                report(a, rng.choice(side), rng.choice(states))
            else:
                report(a, *rng.choice([(None, None), (uuid_of(p.tasks[0]), None), (None, "RUNNING")]))

    def check(tag):
        uids = list(p.tasks)
        ids = [uuid_of(u) for u in uids]
        # nodes_per_task: the sync service's count over the store's records, named through the task list
        got = sorted((t, name, int(n)) for t, name, n in _lines(_text(lambda o, c, n: p.L.pmx_nodes_per_task(p._p, o, c, n))))
        assert got == M.nodes_per_task(store, [(i, "task") for i in ids]), tag
        # the classes and the tables over the engine's groups
        group_of, _, _ = p.eng.get_groups()
        groups = engine_groups(p.eng)
        want = M.read(W, group_of, groups, uids, led)
        s = np.zeros(1, dtype=E.ro_summary_dt)
        _check(p.L.pmx_rollout_summary(p._p, s.ctypes.data))
        assert (tuple(s[0]["by_class"].tolist()), tuple(s[0]["by_state"].tolist()), int(s[0]["groups_with_task"]),
                int(s[0]["groups_converged"]), int(s[0]["distinct_uids"])) == want["summary"], tag
        text_of = lambda uid, task: ids[task] if task != M.NONE else texts.get(uid, format(uid, "x"))
        want_tasks = [[text_of(u, t), "task" if t != M.NONE else "unknown", "-" if t == M.NONE else str(t), str(g), str(gc), str(a),
                       str(c)] + [str(x) for x in rep] for u, t, g, gc, a, c, rep in want["tasks"]]
        assert _lines(_text(lambda o, c, n: p.L.pmx_task_rollout(p._p, o, c, n))) == want_tasks, tag
        want_groups = [[format(gid, "x"), p.config_names[cfg], ids[t], str(size)] + [str(x) for x in same] + [str(other), str(silent)]
                       for gid, _slot, cfg, t, size, same, other, silent in want["groups"]]
        assert _lines(_text(lambda o, c, n: p.L.pmx_group_rollout(p._p, o, c, n))) == want_groups, tag
        first = {}
        for k, u in enumerate(uids):
            first.setdefault(u, k)
        want_nodes = [[addr_of_row[w], str(c), "-" if st == M.TS_NONE else str(st),
                       "-" if st == M.TS_NONE else text_of(u, M.NONE if u == M.ALL_ONES else first.get(u, M.NONE))]
                      for w, _slot, u, c, st in want["workers"]]
        assert _lines(_text(lambda o, c, n: p.L.pmx_rollout_nodes(p._p, ALL, o, c, n))) == want_nodes, tag
        lag = [r for r in want_nodes if int(r[1]) in (M.OTHER, M.BEHIND)]
        mask = (1 << M.OTHER) | (1 << M.BEHIND)
        assert _lines(_text(lambda o, c, n: p.L.pmx_rollout_nodes(p._p, mask, o, c, n))) == lag, tag
        return want

    wave(0.2)
    assert check("before any tick")["summary"][2] == 0
    for k in range(4):
        p.tick()
        wave(0.6)
        if k == 1:
            _check(p.L.pmx_flush_rollout(p._p))                 # (an explicit flush in front of the reads)
        want = check(f"round {k}")
        assert want["summary"][2] > 0 and want["summary"][0][M.CONVERGED] > 0
        if k == 0:                                              # deaths: their groups dissolve at once, their rows stay
            for node in rng.sample(sorted(healthy), 60):
                p.handle_status_change(node, healthy=False, dead=True)
                healthy.discard(node)
            check("after deaths, before the tick")
        if k == 1:                                              # the most reported task goes: its reporters stay, as an unknown id
            victim = max((r for r in want["tasks"] if r[1] != M.NONE and r[2]), key=lambda r: sum(r[6]))[0]
            p.on_task_deleted(victim)
            after = check("after a task was deleted")
            row = [r for r in after["tasks"] if r[0] == victim][0]
            assert row[1] == M.NONE and row[2] == 0 and sum(row[6]) > 0
        if k == 2:
            p.on_task_created(int(sw.task_masks()[0]), int(sw.created_at.max()) + 10, 0x1234567890)
            check("after a task was created")
    p.close()
