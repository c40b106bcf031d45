"""The C++ plugin over the real engine: GpuMatchPlugin::enable_change_feed / changed_nodes through pm_plugin_c.h
(pmx_enable_change_feed, pmx_changed_nodes) against the model of tests/changes_model.py — after every interval of a small
replay (deaths, a new task, a tick) the listed addresses are those of the model's rows, in row order, with the model's bits."""
import ctypes as C

import numpy as np
import pytest

from protocol_amd.swarm import make_swarm

import changes_model as M
from plugin_cxx import PluginCxx, _check, _text, plugin_lib

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF


def bind(L):
    vp, sz = C.c_void_p, C.c_size_t
    L.pmx_enable_change_feed.argtypes = [vp, C.c_int32]
    L.pmx_changed_nodes.argtypes = [vp, C.c_char_p, sz, C.POINTER(sz)]
    return L


def changed_nodes(p):
    lines = _text(lambda o, c, n: p.L.pmx_changed_nodes(p._p, o, c, n)).splitlines()
    head = lines[0].split("\t")
    assert head[0] == "resync" and head[1] in ("0", "1")
    return [(a, int(b)) for a, b in (ln.split("\t") for ln in lines[1:])], head[1] == "1"


def test_changed_nodes_through_the_c_face():
    sw = make_swarm(43, 60, 400)
    bind(plugin_lib())
    p = PluginCxx(sw)
    with pytest.raises(RuntimeError):
        changed_nodes(p)                                       # the feed is off
    p.sync_nodes(range(sw.W), set(range(sw.W)))
    p.sync_tasks(sw.task_masks(), sw.created_at, sw.task_uid)
    _check(p.L.pmx_enable_change_feed(p._p, 1))
    n_rows = len(p.rows)
    row_of_node = {}
    for node in range(sw.W):
        row = C.c_uint32(0)
        _check(p.L.pmx_row_of(p._p, p.addr[node], C.byref(row)))
        row_of_node[node] = row.value
    addr_of_row = {r: p.addr[node].decode() for node, r in row_of_node.items()}
    assert len(addr_of_row) == n_rows == sw.W
    feed = M.Feed()

    def published():
        t = []
        for w in range(n_rows):
            a = p.eng.lookup(w)
            t.append(M.row_of(a.group_slot, a.group_id, a.group_index, a.group_size, a.next_worker,
                              None if a.task == NONE else p.tasks[a.task]))
        feed.publish(t)

    def check(tag):
        got, resync = changed_nodes(p)
        want, want_resync = feed.drain()
        assert resync == want_resync, tag
        assert got == [(addr_of_row[w], b) for w, b in want], tag
        return want

    p.tick()
    published()
    assert len(check("resync")) == n_rows
    rng = np.random.default_rng(2)
    alive = list(range(sw.W))
    seen = 0
    for k in range(4):
        for node in rng.choice(alive, 12, replace=False):
            p.handle_status_change(int(node), healthy=False, dead=True)
            alive.remove(int(node))
        if k == 2:
            p.on_task_created(int(sw.task_masks()[0]), int(sw.created_at.max()) + 10 + k, (1 << 41) + k)
        p.tick()
        published()
        want = check(f"interval {k}")
        assert 0 < len(want) < n_rows // 2, k
        for _, b in want:
            seen |= b
    assert seen & M.GROUP and seen & M.RING
    assert changed_nodes(p) == ([], False)
    _check(p.L.pmx_enable_change_feed(p._p, 0))
    with pytest.raises(RuntimeError):
        changed_nodes(p)
    p.close()
