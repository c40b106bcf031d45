"""The C++ plugin over the real engine: GpuMatchPlugin::group_spread / configuration_spread / force_regroup through
pm_plugin_c.h (pmx_group_spread, pmx_configuration_spread, pmx_force_regroup) against the model of tests/spread_model.py —
rows keyed by group id text with node addresses for worker rows, the route's counts, the destroyed webhooks in id-text
order, the 404 for an unknown configuration name."""
import ctypes as C

import numpy as np
import pytest

from protocol_amd import engine as E
from protocol_amd.swarm import make_swarm

import spread_model as SM
from plugin_cxx import PluginCxx, _check, _text, plugin_lib

pytestmark = pytest.mark.gpu


def bind(L):
    vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
    L.pmx_group_spread.argtypes = [vp, C.c_char_p, sz, C.POINTER(sz)]
    L.pmx_configuration_spread.argtypes = [vp, C.c_char_p, sz, C.POINTER(sz)]
    L.pmx_force_regroup.argtypes = [vp, C.c_char_p, u32, C.c_double, C.POINTER(C.c_int32), C.POINTER(u32), C.POINTER(u32)]
    return L


def group_spread(p):
    """{group id text: row} with node indices for addresses"""
    node = lambda a: SM.NONE if a == "-" else p.node_of_addr[a]
    out = {}
    for line in _text(lambda o, c, n: p.L.pmx_group_spread(p._p, o, c, n)).splitlines():
        f = line.split("\t")
        out[f[0]] = dict(located=int(f[1]), ring_hops=int(f[2]), far_a=node(f[3]), far_b=node(f[4]), hop_from=node(f[5]),
                         diameter_km=float(f[6]), ring_km=float(f[7]), longest_hop_km=float(f[8]))
    return out


def configuration_spread(p):
    out = []
    for line in _text(lambda o, c, n: p.L.pmx_configuration_spread(p._p, o, c, n)).splitlines():
        f = line.split("\t")
        out.append(dict(name=f[0], groups=int(f[1]), measured=int(f[2]), hist=[int(x) for x in f[3:8]],
                        max_diameter_km=float(f[8]), max_hop_km=float(f[9]), sum_diameter_m=int(f[10]), sum_ring_m=int(f[11])))
    return out


def force_regroup(p, name, metric=E.REGROUP_ALL, threshold_km=0.0):
    found, g, w = C.c_int32(-1), C.c_uint32(0), C.c_uint32(0)
    _check(p.L.pmx_force_regroup(p._p, name.encode(), metric, threshold_km, C.byref(found), C.byref(g), C.byref(w)))
    p._take_webhooks()
    return None if not found.value else (g.value, w.value)


def test_group_spread_and_force_regroup_through_the_c_face():
    sw = make_swarm(41, 1200, 300)
    bind(plugin_lib())
    p = PluginCxx(sw)
    p.sync_nodes(range(sw.W), set(range(sw.W)))
    p.sync_tasks(sw.task_masks(), sw.created_at, sw.task_uid)
    p.tick()
    p.events.clear()
    cols = p.packed_all
    order = np.argsort(np.array([a.decode() for a in p.addr]))      # BTreeSet<String>: the address strings' byte order
    rank = np.empty(sw.W, dtype=np.uint32)
    rank[order] = np.arange(sw.W, dtype=np.uint32)
    groups = p.get_all_groups()                                        # id-text order (mod.rs:1040)
    assert len(groups) > 20 and [g["id"] for g in groups] == sorted(g["id"] for g in groups)
    members = [[p.node_of_addr[a] for a in g["nodes"]] for g in groups]
    want = [SM.group_spread(m, cols["flags"], cols["lat"], cols["lon"], rank) for m in members]
    got = group_spread(p)
    assert sorted(got) == [g["id"] for g in groups]
    SM.check_rows([got[g["id"]] for g in groups], want, cols["lat"], cols["lon"], None, "plugin")
    # per configuration, by name: exact functions of the rows
    cfg_of = [p.config_names.index(g["config"]) for g in groups]
    cs = configuration_spread(p)
    model = SM.config_spread([got[g["id"]] for g in groups], cfg_of, len(p.config_names))
    assert [c["name"] for c in cs] == p.config_names
    for c, m in zip(cs, model):
        assert (c["groups"], c["measured"], c["hist"]) == (int(m["groups"]), int(m["measured"]), m["hist"].tolist())
        assert (c["max_diameter_km"], c["max_hop_km"]) == (float(m["max_diameter_km"]), float(m["max_hop_km"]))
        assert (c["sum_diameter_m"], c["sum_ring_m"]) == (int(m["sum_diameter_m"]), int(m["sum_ring_m"]))
    # the 404
    assert force_regroup(p, "no-such-configuration") is None and p.events == []
    # by diameter, in the middle of a gap of the oracle's values of the fullest configuration
    name = max(p.config_names, key=lambda n: sum(1 for g in groups if g["config"] == n))
    mine = [k for k, g in enumerate(groups) if g["config"] == name]
    vals = sorted({want[k]["diameter_km"] for k in mine if want[k]["located"] >= 2 and want[k]["diameter_km"] <= SM.KM_AT_A_0_999})
    assert len(vals) >= 3
    lo, hi = vals[len(vals) // 2 - 1], vals[len(vals) // 2]
    assert hi - lo >= 1e-6 * hi
    thr = (lo + hi) / 2.0
    sel = [k for k in mine if want[k]["located"] >= 2 and want[k]["diameter_km"] >= thr]
    assert force_regroup(p, name, E.REGROUP_DIAMETER, thr) == (len(sel), sum(len(members[k]) for k in sel))
    assert [(e[0], format(e[1], "x")) for e in p.events] == [(E.GROUP_DESTROYED, groups[k]["id"]) for k in sel]   # id-text order
    assert all(p.get_node_group(groups[k]["nodes"][0]) is None for k in sel)
    # the route as the reference has it: what is left of the configuration, located or not
    p.events.clear()
    rest = [k for k in mine if k not in sel]
    assert force_regroup(p, name) == (len(rest), sum(len(members[k]) for k in rest))
    assert [format(e[1], "x") for e in p.events] == [groups[k]["id"] for k in rest]
    assert [g["id"] for g in p.get_all_groups()] == [g["id"] for g in groups if g["config"] != name]
    with pytest.raises(RuntimeError):
        force_regroup(p, name, 9, 0.0)
    p.close()
