"""The C++ plugin over the real engine: GpuMatchPlugin's directory methods through pm_plugin_c.h (pmx_list_nodes,
pmx_status_counts, pmx_uninvited_nodes, pmx_dead_nodes) on a 300-node swarm behind a tick with all eight statuses present and a
few task reports.  Every text equals, byte for byte, what the model of tests/directory_model.py gives over the engine's other
reads (the ledgers, pm_get_groups), rendered as pm_plugin_c.h says."""
import ctypes as C

import numpy as np
import pytest

from protocol_amd.swarm import make_swarm
from helpers import engine_groups

import directory_model as M
from plugin_cxx import PluginCxx, _check, _text, plugin_lib, uuid_of

pytestmark = pytest.mark.gpu


def bind(L):
    vp, sz, s, u32 = C.c_void_p, C.c_size_t, C.c_char_p, C.c_uint32
    L.pmx_enable_liveness.argtypes = [vp, u32]
    L.pmx_enable_rollout.argtypes = [vp]
    L.pmx_report_task.argtypes = [vp, s, s, s]
    L.pmx_flush_rollout.argtypes = [vp]
    L.pmx_list_nodes.argtypes = [vp, u32, u32, u32, u32, s, sz, C.POINTER(sz)]
    L.pmx_status_counts.argtypes = [vp, s, sz, C.POINTER(sz)]
    L.pmx_uninvited_nodes.argtypes = [vp, s, sz, C.POINTER(sz)]
    L.pmx_dead_nodes.argtypes = [vp, s, sz, C.POINTER(sz)]
    return L


def test_a_swarm_with_every_status_through_the_c_face():
    sw = make_swarm(77, 40, 300)
    W = sw.W
    bind(plugin_lib())
    p = PluginCxx(sw)
    p.sync_nodes(range(W), set(range(W)))
    p.sync_tasks(sw.task_masks(), sw.created_at, sw.task_uid)
    p.eng.W = W
    with pytest.raises(RuntimeError):                           # liveness is off: the engine's refusal travels
        _text(lambda o, c, n: p.L.pmx_status_counts(p._p, o, c, n))
    _check(p.L.pmx_enable_liveness(p._p, 3))
    _check(p.L.pmx_enable_rollout(p._p))
    p.tick()
    addr = [a.decode() for a in p.addr]
    addr_of_row = {}
    for node in range(W):
        row = C.c_uint32(0)
        _check(p.L.pmx_row_of(p._p, p.addr[node], C.byref(row)))
        addr_of_row[row.value] = addr[node]
    assert sorted(addr_of_row) == list(range(W))
    by_text = sorted(range(W), key=lambda w: addr_of_row[w])
    ranks = [0] * W
    for k, w in enumerate(by_text):
        ranks[w] = k                                            # the rank column sync_nodes keeps: the address text's order
    rng = np.random.default_rng(5)
    statuses = rng.integers(0, M.NS_N, W)
    assert len(set(statuses.tolist())) == M.NS_N
    p.eng.liveness_set(np.arange(W, dtype=np.uint32), statuses.astype(np.uint8), rng.integers(0, 50, W).astype(np.uint32))
    for node in range(0, W, 3):                                 # some task fields, as the heartbeat route hands them over
        _check(p.L.pmx_report_task(p._p, p.addr[node], uuid_of(p.tasks[node % len(p.tasks)]).encode(),
                                   [b"RUNNING", b"PULLING", b"FAILED"][node % 3]))
    _check(p.L.pmx_flush_rollout(p._p))

    texts = {}
    for dead, order, off, lim in ((0, 0, 0, M.TO_END), (1, 0, 0, M.TO_END), (1, 1, 0, M.TO_END), (0, 1, 0, 50), (0, 1, 50, 50),
                                  (1, 0, 120, 100), (1, 1, W - 1, 7), (0, 0, W, 3), (1, 1, 0, 0)):
        texts[(dead, order, off, lim)] = _text(lambda o, c, n: p.L.pmx_list_nodes(p._p, dead, order, off, lim, o, c, n))
    gauge = _text(lambda o, c, n: p.L.pmx_status_counts(p._p, o, c, n))
    uninvited = _text(lambda o, c, n: p.L.pmx_uninvited_nodes(p._p, o, c, n))
    gone = _text(lambda o, c, n: p.L.pmx_dead_nodes(p._p, o, c, n))

    # the model's inputs from the engine's other reads
    st, cnt = p.eng.liveness_get()
    assert st.tolist() == statuses.tolist()
    group_of, _, _ = p.eng.get_groups()
    groups = engine_groups(p.eng)
    uid, state = p.eng.rollout_get()
    ledger = list(zip(uid.tolist(), state.tolist()))
    assert any(g >= 0 for g in group_of) and any(s != M.TS_NONE for _, s in ledger)
    read = lambda q: M.directory(st.tolist(), cnt.tolist(), group_of.tolist(), groups, list(p.tasks), ledger, ranks, q)

    def render(dead, order, off, lim):
        total, counts, rows = read(M.query(status_mask=M.ALL if dead else M.NOT_DEAD, order=order, offset=off, limit=lim))
        out = ["total\t%d" % total]
        out += ["count\t%s\t%d" % (name, c) for name, c in sorted((M.STATUS_NAMES[s], c) for s, c in enumerate(counts) if c)]
        for w, status, _cls, tstate, counter, slot, gid, size, cfg, _task, _uid in rows:
            grp = ["-", "-", "-"] if slot == M.NONE else [format(gid, "x"), str(size), p.config_names[cfg]]
            out.append("\t".join([addr_of_row[w], M.STATUS_NAMES[status], str(counter), "-" if tstate == M.TS_NONE else str(tstate)] + grp))
        return "".join(line + "\n" for line in out)

    for key, got in texts.items():
        assert got == render(*key), key
    assert texts[(0, 0, 0, M.TO_END)].count("\n") > 200 and "\tDead\t" not in texts[(0, 0, 0, M.TO_END)]
    total, counts, _ = read(M.query(limit=0))
    assert gauge == "".join("%s\t%d\n" % nc for nc in sorted((M.STATUS_LOWER[s], c) for s, c in enumerate(counts) if c))
    assert uninvited == "".join(addr_of_row[r[0]] + "\n" for r in read(M.query(status_mask=1 << M.DISCOVERED))[2])
    assert gone == "".join(addr_of_row[r[0]] + "\n" for r in read(M.query(status_mask=1 << M.DEAD))[2])
    assert uninvited and gone
    p.close()
