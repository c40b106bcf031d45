"""The C++ plugin over the real engine: GpuMatchPlugin's metrics methods through pm_plugin_c.h (pmx_beat_metrics & co.) — a
seeded replay of heartbeats, manual metrics, deletions and clean-ups on a small swarm, with ticks, deaths and a dissolution
between the calls.  After every round the plugin's reads equal the literal store of tests/metrics_model.py (values are small
integers and halves, so every order of adding is exact), and the sync service's list carries the group id and configuration
name that pm_get_groups reports at that moment."""
import ctypes as C
import random

import pytest

from protocol_amd.swarm import make_swarm
from helpers import engine_groups

import metrics_model as M
from plugin_cxx import PluginCxx, _check, _text, plugin_lib

pytestmark = pytest.mark.gpu


def bind(L):
    vp, sz, cpp, s = C.c_void_p, C.c_size_t, C.POINTER(C.c_char_p), C.c_char_p
    L.pmx_enable_metrics.argtypes = [vp]
    L.pmx_beat_metrics.argtypes = [vp, s, cpp, cpp, C.POINTER(C.c_double), C.c_uint32]
    L.pmx_store_metrics.argtypes = [vp, s, cpp, cpp, C.POINTER(C.c_double), C.c_uint32]
    L.pmx_store_manual_metric.argtypes = [vp, s, C.c_double]
    L.pmx_delete_metric.argtypes = [vp, s, s, s]
    L.pmx_clear_metrics.argtypes = [vp, s]
    L.pmx_flush_metrics.argtypes = [vp]
    L.pmx_aggregate_metrics.argtypes = [vp, s, s, sz, C.POINTER(sz)]
    L.pmx_metrics_for_node.argtypes = [vp, s, s, sz, C.POINTER(sz)]
    L.pmx_synced_metrics.argtypes = [vp, cpp, cpp, C.c_uint32, s, sz, C.POINTER(sz)]
    return L


def _arrays(mets):
    n = max(len(mets), 1)
    t = (C.c_char_p * n)(*[m[0].encode() for m in mets])
    lab = (C.c_char_p * n)(*[m[1].encode() for m in mets])
    v = (C.c_double * n)(*[m[2] for m in mets])
    return t, lab, v


def aggregate(p, task_id=None):
    text = _text(lambda o, c, n: p.L.pmx_aggregate_metrics(p._p, None if task_id is None else task_id.encode(), o, c, n))
    return {k: float.fromhex(v) for k, v in (ln.split("\t") for ln in text.splitlines())}


def for_node(p, address):
    text = _text(lambda o, c, n: p.L.pmx_metrics_for_node(p._p, address.encode(), o, c, n))
    out = {}
    for task, label, v in (ln.split("\t") for ln in text.splitlines()):
        out.setdefault(task, {})[label] = float.fromhex(v)
    return out


def synced(p, names):
    ids = (C.c_char_p * max(len(names), 1))(*[k.encode() for k in names])
    nm = (C.c_char_p * max(len(names), 1))(*[v.encode() for v in names.values()])
    text = _text(lambda o, c, n: p.L.pmx_synced_metrics(p._p, ids, nm, len(names), o, c, n))
    return [tuple(ln.split("\t")) for ln in text.splitlines()]


def test_a_replay_with_ticks_between_the_calls():
    sw = make_swarm(43, 120, 300)
    W = sw.W
    bind(plugin_lib())
    p = PluginCxx(sw)
    p.sync_nodes(range(W), set(range(W)))
    p.sync_tasks(sw.task_masks(), sw.created_at, sw.task_uid)
    p.eng.W = W
    with pytest.raises(RuntimeError):                           # the ledger is off: the flush reports the engine's refusal
        _check(p.L.pmx_store_manual_metric(p._p, b"uptime", 1.0))
        _check(p.L.pmx_flush_metrics(p._p))
    _check(p.L.pmx_enable_metrics(p._p))
    addr = [a.decode() for a in p.addr]
    row_of = {}
    for node in range(W):
        row = C.c_uint32(0)
        _check(p.L.pmx_row_of(p._p, p.addr[node], C.byref(row)))
        row_of[addr[node]] = row.value
    st = M.Store()
    rng = random.Random(5)
    tasks, labels = ["", "t1", "t2"], ["loss", "lr", "dashboard-progress", "dashboard:-progress", "a:b", "ab", "x/y"]
    names = {"t1": "first"}
    values = [0.0, -0.0, 1.0, -1.0, 2.5, 3.0, 64.0, -7.5]
    healthy = set(range(W))

    def check(tag):
        # the aggregates: every order of adding is exact for these values; the store adds in the ledger's order
        order = [M.ZERO] + sorted(addr, key=lambda a: row_of[a])
        assert aggregate(p) == st.get_aggregate_metrics_for_all_tasks(order), tag
        for t in ("t1", "t2", "manual", "nobody"):
            assert aggregate(p, t) == st.get_aggregate_metrics_for_task(t, order), (tag, t)
        for a in rng.sample(addr, 12) + [M.ZERO]:
            got, want = for_node(p, a), st.get_metrics_for_node(a)
            assert got == want and M.same_fields(got, want), (tag, a)
        # the sync service's list against the store's, the join against pm_get_groups
        gow, groups, _ = p.eng.get_groups()
        group_of_address = {a: (format(int(groups[gow[row_of[a]]]["id"]), "x"), p.config_names[int(groups[gow[row_of[a]]]["config"])])
                            for a in addr if gow[row_of[a]] >= 0}
        want = sorted((a, t, tn, lab, M.bits(v), gid or "-", cfg or "-") for a, t, tn, lab, v, gid, cfg in st.synced_metrics(names, group_of_address))
        got = synced(p, names)
        assert sorted((a, t, tn, lab, M.bits(float.fromhex(v)), gid, cfg) for a, t, tn, lab, v, gid, cfg in got) == want, tag
        assert [g[0] for g in got] == sorted((g[0] for g in got), key=lambda a: -1 if a == M.ZERO else row_of[a]), tag
        return sum(1 for g in got if g[5] != "-")

    for k in range(8):
        for _ in range(150):
            a = rng.choice(addr + [M.ZERO])
            mets = [(rng.choice(tasks), rng.choice(labels), rng.choice(values)) for _ in range(rng.randrange(0, 5))]
            what = rng.random()
            if what < 0.6:
                t, lab, v = _arrays(mets)
                _check(p.L.pmx_beat_metrics(p._p, a.encode(), t, lab, v, len(mets)))
                st.heartbeat(a, mets)
            elif what < 0.75:
                t, lab, v = _arrays(mets)
                _check(p.L.pmx_store_metrics(p._p, a.encode(), t, lab, v, len(mets)))
                st.store_metrics(mets, a)
            elif what < 0.85:
                lab, v = rng.choice(labels), rng.choice(values)
                _check(p.L.pmx_store_manual_metric(p._p, lab.encode(), v))
                st.store_manual_metrics(lab, v)
            elif what < 0.95:
                t, lab = rng.choice(["manual", "t1", "t2"]), rng.choice(labels)
                _check(p.L.pmx_delete_metric(p._p, t.encode(), lab.encode(), a.encode()))
                st.delete_metric(t, lab, a)
            else:
                _check(p.L.pmx_clear_metrics(p._p, a.encode()))
                st.clear_node(a)
        if k == 1:
            _check(p.L.pmx_flush_metrics(p._p))                 # (an explicit flush in front of a tick)
        p.tick()
        grouped = check(f"round {k}")
        assert k == 0 or grouped > 0
        if k == 3:                                              # deaths: their groups dissolve at once
            for node in rng.sample(sorted(healthy), 10):
                p.handle_status_change(node, healthy=False, dead=True)
                healthy.discard(node)
            check("after deaths, before the tick")
        if k == 5:
            gid = engine_groups(p.eng)[0][0]
            p.dissolve_group(format(gid, "x"))
            check("after a dissolution")
    p.close()
