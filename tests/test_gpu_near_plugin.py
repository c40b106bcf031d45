"""The C++ plugin over the real engine: GpuMatchPlugin::nearest_nodes through pm_plugin_c.h (pmx_nearest_nodes) against the
model of tests/near_model.py — node addresses for worker rows, configurations by name, both pools, the seed, the not-found
result for an unknown address and the error for an unknown configuration name."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle_ffi as orc
from protocol_amd import engine as E
from protocol_amd.swarm import make_swarm

import near_model as NM
from plugin_cxx import PluginCxx, _text, plugin_lib

pytestmark = pytest.mark.gpu


def bind(L):
    vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
    L.pmx_nearest_nodes.argtypes = [vp, C.c_char_p, C.c_char_p, u32, u32, C.POINTER(C.c_int32), C.c_char_p, sz, C.POINTER(sz)]
    return L


def nearest_nodes(p, address, name, pool, k):
    """None: not found; else (row fields, worker indices, km) with node indices for addresses"""
    found = C.c_int32(-1)
    a = None if address is None else address if isinstance(address, bytes) else address.encode()
    text = _text(lambda o, c, n: p.L.pmx_nearest_nodes(p._p, a, name.encode(), pool, k, C.byref(found), o, c, n))
    if not found.value:
        assert text == ""
        return None
    lines = text.splitlines()
    head = lines[0].split("\t")
    assert head[0] == "origin"
    nodes = [ln.split("\t") for ln in lines[1:]]
    row = dict(origin=NM.NONE if head[1] == "-" else p.node_of_addr[head[1]], n=len(nodes), candidates=int(head[2]),
               located=int(head[3]))
    workers = [p.node_of_addr[a] for a, _ in nodes] + [NM.NONE] * (k - len(nodes))
    km = [NM.F64_MAX if d == "-" else float(d) for _, d in nodes] + [NM.F64_MAX] * (k - len(nodes))
    return row, workers, km


def test_nearest_nodes_through_the_c_face():
    sw = make_swarm(41, 1200, 300)
    rng = np.random.default_rng(8)
    sw.lat = np.ascontiguousarray(rng.uniform(-50.0, 60.0, sw.W))     # (inside the tolerance's range: a <= 0.999)
    sw.lon = np.ascontiguousarray(rng.uniform(-100.0, 50.0, sw.W))
    bind(plugin_lib())
    p = PluginCxx(sw)
    p.sync_nodes(range(sw.W), set(range(sw.W)))
    p.sync_tasks(sw.task_masks(), sw.created_at, sw.task_uid)
    p.tick()
    for g in p.get_all_groups()[::2]:                                   # (the tick groups nearly everybody: free half again)
        p.dissolve_group(g["id"])
    cols = p.packed_all
    flags = cols["flags"].astype(np.uint32) | np.uint32(E.W_HEALTHY)   # (the snapshot: every node Healthy; a p2p id where the swarm has one)
    nodes, cfgs, _tasks, _enabled = orc.from_swarm(sw)
    compat = orc.compat_masks(nodes, cfgs)
    gof = np.full(sw.W, -1, dtype=np.int64)
    for gi, g in enumerate(p.get_all_groups()):
        gof[[p.node_of_addr[a] for a in g["nodes"]]] = gi
    assert (gof >= 0).sum() > 50 and (gof < 0).sum() > 50
    addr_of = {v: k for k, v in p.node_of_addr.items()}
    grouped, free = int(np.flatnonzero(gof >= 0)[0]), int(np.flatnonzero(gof < 0)[0])
    n_checked = 0
    for c, name in enumerate(p.config_names):
        for pool in (E.NEAR_IDLE, E.NEAR_ELIGIBLE):
            for origin, k in ((None, 16), (grouped, 5), (free, 256)):
                got = nearest_nodes(p, None if origin is None else addr_of[origin], name, pool, k)
                assert got is not None
                want = NM.nearest(E.NEAR_SEED if origin is None else origin, c, pool, k, compat, flags, gof,
                                  cols["lat"], cols["lon"])
                NM.check_query(got[0], got[1], got[2], want, False, f"{name} pool {pool} origin {origin}")
                n_checked += want["n"]
    assert n_checked > 500
    # an address the node table does not hold: the not-found result; an unknown configuration name: an error
    assert nearest_nodes(p, "0x" + "f" * 40, p.config_names[0], E.NEAR_IDLE, 4) is None
    with pytest.raises(RuntimeError):
        nearest_nodes(p, None, "no-such-configuration", E.NEAR_IDLE, 4)
    with pytest.raises(RuntimeError):
        nearest_nodes(p, None, p.config_names[0], E.NEAR_IDLE, 0)
    p.close()
