"""The C++ plugin over the real engine: GpuMatchPlugin::enable_liveness / beat / sweep_statuses through pm_plugin_c.h
(pmx_enable_liveness, pmx_beat, pmx_sweep_statuses) — five intervals of beats and silences on a small swarm.  After every
interval the returned transitions and the ledger's statuses equal the model of tests/liveness_model.py, the groups equal the
oracle that was given the same flips, and a node that died and came back is served a task again."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle_ffi as orc
from protocol_amd import engine as E
from protocol_amd.swarm import make_swarm
from helpers import engine_groups, oracle_groups

import liveness_model as M
from plugin_cxx import PluginCxx, _check, _text, plugin_lib

pytestmark = pytest.mark.gpu
NOW = 1_760_000_000_000
STEP = 15_000


def bind(L):
    vp, sz = C.c_void_p, C.c_size_t
    L.pmx_enable_liveness.argtypes = [vp, C.c_uint32]
    L.pmx_beat.argtypes = [vp, C.c_char_p, C.c_uint64]
    L.pmx_sweep_statuses.argtypes = [vp, C.c_uint64, C.POINTER(C.c_char_p), C.c_uint32, C.c_char_p, sz, C.POINTER(sz)]
    return L


def sweep_statuses(p, now, out_of_pool=()):
    arr = (C.c_char_p * max(len(out_of_pool), 1))(*out_of_pool)
    text = _text(lambda o, c, n: p.L.pmx_sweep_statuses(p._p, now, arr, len(out_of_pool), o, c, n))
    return [(a, int(old), int(new)) for a, old, new in (ln.split("\t") for ln in text.splitlines())]


def test_five_intervals_of_beats_and_silences():
    sw = make_swarm(43, 120, 300)
    W = sw.W
    bind(plugin_lib())
    p = PluginCxx(sw)
    with pytest.raises(RuntimeError):
        sweep_statuses(p, NOW)                                 # liveness is off
    p.sync_nodes(range(W), set(range(W)))
    p.sync_tasks(sw.task_masks(), sw.created_at, sw.task_uid)
    for node in range(W):                                      # (synced in order: a node's row is its number)
        row = C.c_uint32(0)
        _check(p.L.pmx_row_of(p._p, p.addr[node], C.byref(row)))
        assert row.value == node
    p.eng.W = W
    _check(p.L.pmx_enable_liveness(p._p, 1))                   # m = 1: Healthy -> Unhealthy -> Dead in two silent intervals
    led = M.Ledger(np.full(W, M.W_HEALTHY), 1)
    nodes, cfgs, tasks, enabled = orc.from_swarm(sw)
    nodes["status"][:] = 2                                     # (the snapshot above: every node Healthy)
    st = orc.State(nodes, cfgs, enabled=enabled, tasks=tasks)

    def tick(tag):
        p.tick()
        st.try_form_new_groups()
        st.try_merge_solo_groups()
        for w in range(W):
            st.get_task_for_node(w)                            # (the oracle claims on this call)
        assert sorted(engine_groups(p.eng)) == sorted(oracle_groups(st)), tag

    tick("first")
    served = [g for g in engine_groups(p.eng) if len(g[2]) > 1 and g[3] >= 0]
    victim, bystander = served[0][2][0], served[1][2][0]
    mates = [w for w in served[0][2] if w != victim]
    assert p.task_for_node(victim) is not None and p.task_for_node(mates[0]) is not None
    beats = np.zeros(W, dtype=np.uint64)
    now = NOW
    #            interval:     0           1        2      3 (beats again)    4
    quiet = [{victim, bystander}, {victim}, {victim}, set(), set()]
    want_victim = [(M.HEALTHY, M.UNHEALTHY), (M.UNHEALTHY, M.DEAD), None, (M.DEAD, M.HEALTHY), None]
    for k in range(5):
        now += STEP
        for node in range(W):
            if node not in quiet[k]:
                _check(p.L.pmx_beat(p._p, p.addr[node], now - 100 - node))
                beats[node] = now - 100 - node
        # interval 1: the bystander beats again but is_node_in_pool says no -> Discovered; interval 2: in the pool -> Healthy
        out_of_pool = [p.addr[bystander]] if k == 1 else []
        pool = None if not out_of_pool else M.pack_bits(np.arange(W) != bystander)
        got = sweep_statuses(p, now, out_of_pool)
        rows, _ = led.sweep(now, beats, pool)
        assert got == [(p.addr[w].decode(), old, new) for w, old, new, _ in rows], k
        assert dict((w, (old, new)) for w, old, new, _ in rows).get(victim) == want_victim[k], k
        for w, _, new, _ in rows:
            st.set_node_status(int(w), int(new))
        s, c = p.eng.liveness_get(np.arange(W))
        assert s.tolist() == led.status and c.tolist() == led.counter, k
        if k == 1:                                             # the death: the whole group is gone at once, before any tick
            assert p.task_for_node(victim) is None and all(p.task_for_node(m) is None for m in mates)
        tick(f"interval {k}")
        if k == 2:
            assert p.task_for_node(victim) is None             # dead and silent: in no group
    # the bystander missed one beat: Unhealthy, Discovered (out of the pool), then Healthy again; it never died
    assert led.status[bystander] == M.HEALTHY and led.status[victim] == M.HEALTHY
    assert p.task_for_node(victim) is not None                 # revived, carved again, and served
    # a status the host sets elsewhere reaches the ledger through handle_status_change (here: Dead, the counter kept)
    p.handle_status_change(bystander, healthy=False, dead=True)
    s, c = p.eng.liveness_get([bystander])
    assert (int(s[0]), int(c[0])) == (M.DEAD, 0)
    p.close()
