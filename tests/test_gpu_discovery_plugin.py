"""The C++ plugin over the real engine: GpuMatchPlugin::set_endpoint / sync_discovery through pm_plugin_c.h (pmx_set_endpoint,
pmx_sync_discovery) on a small swarm: sightings by address in, outcomes out.  The outcomes and the ledger equal the literal
sequential pass of tests/discovery_model.py; a LowBalance update dissolves a whole group before any tick; the groups equal the
oracle that was given the same updates; the admitted nodes, appended by the caller and Healthy after their first beat, are
carved like the oracle's at the next tick."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle_ffi as orc
from protocol_amd.swarm import make_swarm
from helpers import engine_groups, oracle_groups

import discovery_model as M
from plugin_cxx import PluginCxx, _check, _text, plugin_lib

pytestmark = pytest.mark.gpu
NOW = 1_760_000_000_000


class Sighting(C.Structure):
    _fields_ = [("address", C.c_char_p), ("ip_address", C.c_char_p), ("port", C.c_uint16), ("is_validated", C.c_uint8),
                ("is_provider_whitelisted", C.c_uint8), ("is_active", C.c_uint8), ("location_new", C.c_uint8),
                ("specs_differ", C.c_uint8), ("balance_zero", C.c_uint8), ("last_updated_ms", C.c_uint64)]


def bind(L):
    vp, sz = C.c_void_p, C.c_size_t
    L.pmx_enable_liveness.argtypes = [vp, C.c_uint32]
    L.pmx_beat.argtypes = [vp, C.c_char_p, C.c_uint64]
    L.pmx_sweep_statuses.argtypes = [vp, C.c_uint64, C.POINTER(C.c_char_p), C.c_uint32, C.c_char_p, sz, C.POINTER(sz)]
    L.pmx_set_endpoint.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_uint16]
    L.pmx_sync_discovery.argtypes = [vp, C.c_uint64, C.POINTER(Sighting), C.c_uint32, C.c_uint32, C.c_char_p, sz, C.POINTER(sz)]
    return L


def sync_discovery(p, now, sightings, max_same):
    """sightings: the model's (discovery_model.sighting) -> per sighting (kind, cnt, old, final, ops letters, updates)"""
    arr = (Sighting * max(len(sightings), 1))()
    for k, d in enumerate(sightings):
        arr[k] = Sighting(d["id"].encode(), d["ip_address"].encode(), d["port"], d["is_validated"], d["is_provider_whitelisted"],
                          d["is_active"], 0, 0, d["latest_balance"] == 0, d["last_updated"] or 0)
    text = _text(lambda o, c, n: p.L.pmx_sync_discovery(p._p, now, arr, len(sightings), max_same, o, c, n))
    out = []
    for ln in text.splitlines():
        f = ln.split("\t")
        if f[1] != "synced":
            out.append((f[0], f[1], int(f[2])))
            continue
        updates = [tuple(int(x) for x in u.split(">")) for u in f[6].split(",") if u]
        out.append((f[0], "synced", int(f[2]), int(f[3]), int(f[4]), f[5], updates))
    return out


def test_sightings_in_outcomes_out_and_the_admitted_nodes_at_the_next_tick():
    sw = make_swarm(43, 120, 300)
    W0 = 290                                                   # the last ten nodes are not in the store yet
    bind(plugin_lib())
    p = PluginCxx(sw)
    p.sync_nodes(range(W0), set(range(W0)))
    p.sync_tasks(sw.task_masks(), sw.created_at, sw.task_uid)
    _check(p.L.pmx_enable_liveness(p._p, 3))
    addr = [a.decode() for a in p.addr]
    ip = lambda k: "10.1.%d.%d" % (k // 200, k % 200)
    for k in range(W0):
        _check(p.L.pmx_set_endpoint(p._p, p.addr[k], ip(k).encode(), 8080))
    nodes, cfgs, tasks, enabled = orc.from_swarm(sw)
    nodes["status"][:W0] = 2                                   # (the snapshot above: every stored node Healthy)
    nodes["status"][W0:] = 0
    st = orc.State(nodes, cfgs, enabled=enabled, tasks=tasks)

    def tick(tag):
        p.tick()
        st.try_form_new_groups()
        st.try_merge_solo_groups()
        for w in range(sw.W):
            st.get_task_for_node(w)                            # (the oracle claims on this call)
        assert sorted(engine_groups(p.eng)) == sorted(oracle_groups(st)), tag

    tick("first")
    served = [g for g in engine_groups(p.eng) if len(g[2]) > 1 and g[3] >= 0]
    victim, mover, host = served[0][2][0], served[1][2][0], served[2][2][0]
    mates = [w for w in served[0][2] if w != victim]
    assert p.task_for_node(mates[0]) is not None
    store = M.make_store([M.node(addr[k], M.HEALTHY, ip(k)) for k in range(W0)])
    discovery = [M.sighting(addr[W0 + 2], ip(mover)),                        # new, on the mover's endpoint BEFORE it moves: skipped
                 M.sighting(addr[victim], ip(victim), balance=0),            # LowBalance: its whole group dissolves
                 M.sighting(addr[mover], "172.16.0.1", whitelisted=False),   # Ejected, put back Healthy on the new ip
                 M.sighting(addr[W0], "172.16.0.2"),                         # new, alone: admitted
                 M.sighting(addr[W0 + 1], ip(mover)),                        # new, on the endpoint the mover has LEFT: admitted
                 M.sighting(addr[W0 + 3], ip(host))]                         # new, on a Healthy node's endpoint: skipped
    want, want_status, _, after, abi, _ = M.run_sequential(store, discovery, NOW, 1)
    got = sync_discovery(p, NOW, discovery, 1)
    assert [g[1] for g in got] == ["skipped", "synced", "synced", "admitted", "admitted", "skipped"]
    for g, w, d in zip(got, want, discovery):
        assert g[0] == d["id"] and g[2] == w["cnt"]
        if g[1] == "synced":
            letters = "".join(c for c, bit in (("i", M.DO_IP_REWRITE), ("l", M.DO_LOCATION), ("s", M.DO_SPECS_REWRITE),
                                               ("n", M.DO_STAMP_NOW)) if w["ops"] & bit)
            assert g[3:] == (w["old_status"], w["final_status"], letters, w["updates"])
        else:
            assert (g[1] == "admitted") == (w["ops"] == M.DO_ADMIT)
    assert got[1][6] == [(M.HEALTHY, M.LOWBALANCE)] and got[2][4:] == (M.HEALTHY, "i", [(M.HEALTHY, M.EJECTED)])
    s, _ = p.eng.liveness_get(np.arange(W0))
    assert s.tolist() == want_status
    # the dissolution is there before any tick; the put-back node kept its group
    assert p.task_for_node(victim) is None and all(p.task_for_node(m) is None for m in mates)
    assert p.task_for_node(mover) is not None
    for d, w in zip(discovery, want):
        for _, new in w["updates"]:
            st.set_node_status(addr.index(d["id"]), int(new))
        if w["updates"] and w["final_status"] == M.HEALTHY:
            st.set_node_status(addr.index(d["id"]), M.HEALTHY)
    tick("after the sync")
    assert p.task_for_node(victim) is None
    # the caller appends the admitted nodes (Discovered); their first beat makes them Healthy; the next tick carves them
    p.sync_nodes(range(W0 + 2), set(range(W0)) - {victim})
    s, _ = p.eng.liveness_get(np.arange(W0, W0 + 2))
    assert s.tolist() == [M.DISCOVERED, M.DISCOVERED]
    for k in range(W0 + 2):
        if k != victim:
            _check(p.L.pmx_beat(p._p, p.addr[k], NOW + 10))
    arr = (C.c_char_p * 1)()
    text = _text(lambda o, c, n: p.L.pmx_sweep_statuses(p._p, NOW + 20, arr, 0, o, c, n))
    assert [ln.split("\t") for ln in text.splitlines()] == [[addr[W0], "0", "2"], [addr[W0 + 1], "0", "2"]]
    st.set_node_status(W0, M.HEALTHY)
    st.set_node_status(W0 + 1, M.HEALTHY)
    tick("the admitted nodes")
    # their remembered endpoints: a further new node on the first one's endpoint is skipped
    got = sync_discovery(p, NOW + 30, [M.sighting(addr[W0 + 4], "172.16.0.2"), M.sighting(addr[W0 + 5], "172.16.0.1")], 1)
    assert [(g[1], g[2]) for g in got] == [("skipped", 1), ("skipped", 1)]
    p.close()
