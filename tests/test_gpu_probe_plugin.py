"""The C++ plugin over the real engine: GpuMatchPlugin::probe_configurations / configuration_overlap through pm_plugin_c.h
(pmx_probe_configurations, pmx_configuration_overlap) against the model of tests/probe_model.py — probes by requirement
string, one whose model name matches some of the spec models the plugin interned, the overlap keyed by installed
configuration name, and a requirement string that does not parse."""
import ctypes as C

import numpy as np
import pytest

from protocol_amd import engine as E
from protocol_amd import host
from protocol_amd.swarm import make_swarm

import probe_model as PM
from plugin_cxx import PluginCxx, PmxConfig, _text, plugin_lib

pytestmark = pytest.mark.gpu

PROBES = [("wants-h100", 2, 4, "gpu:count=8;gpu:model=h100"), ("anything", 1, 1, None), ("big-ram", 3, 3, "ram_mb=64000"),
          ("a-or-h", 2, 8, "gpu:count=1;gpu:model=a100;gpu:count=8;gpu:model=h100,a100"), ("nobody-has", 1, 2, "gpu:model=mi355x"),
          ("cpu", 1, 5, "cpu:cores=16;storage_gb=100")]


def bind(L):
    vp, sz = C.c_void_p, C.c_size_t
    L.pmx_probe_configurations.argtypes = [vp, C.POINTER(PmxConfig), C.c_uint32, C.c_char_p, sz, C.POINTER(sz)]
    L.pmx_configuration_overlap.argtypes = [vp, C.c_char_p, sz, C.POINTER(sz)]
    return L


def probe_configurations(p, probes):
    arr = (PmxConfig * max(len(probes), 1))()
    for i, (name, mn, mx, req) in enumerate(probes):
        arr[i] = PmxConfig(name.encode(), mn, mx, None if req is None else req.encode())
    text = _text(lambda o, c, n: p.L.pmx_probe_configurations(p._p, arr, len(probes), o, c, n))
    rows = np.zeros(len(probes), dtype=E.probe_row_dt)
    names, overlap = [], []
    for k, line in enumerate(text.splitlines()):
        f = line.split("\t")
        names.append(f[0])
        for j, key in enumerate(("eligible_meets", "idle_meets", "idle_located", "idle_exclusive", "groups_max", "groups_exclusive")):
            rows[k][key] = int(f[1 + j])
        rows[k]["why"] = [int(v) for v in f[7:17]]
        overlap.append([(kv.rsplit("=", 1)[0], int(kv.rsplit("=", 1)[1])) for kv in f[17:]])
    return names, rows, overlap


def test_probe_configurations_through_the_c_face():
    sw = make_swarm(43, 900, 400)
    bind(plugin_lib())
    p = PluginCxx(sw)
    p.sync_nodes(range(sw.W), set(range(sw.W)))
    p.sync_tasks(sw.task_masks(), sw.created_at, sw.task_uid)
    p.tick()
    for g in p.get_all_groups()[::2]:                                   # (the tick groups nearly everybody: free half again)
        p.dissolve_group(g["id"])
    names, rows, overlap = probe_configurations(p, PROBES)              # (before get_all_groups: the dissolutions are pending)
    cc_text = _text(lambda o, c, n: p.L.pmx_configuration_overlap(p._p, o, c, n))
    cols = dict(p.packed_all)
    cols["flags"] = cols["flags"].astype(np.uint32) | np.uint32(E.W_HEALTHY)  # (the snapshot: every node Healthy)
    gof = np.full(sw.W, -1, dtype=np.int64)
    for gi, g in enumerate(p.get_all_groups()):
        gof[[p.node_of_addr[a] for a in g["nodes"]]] = gi
    assert (gof >= 0).sum() > 50 and (gof < 0).sum() > 50
    cfg_rows, alt_rows, req_models = host.pack_configs(sw.configs)
    installed = (cfg_rows, alt_rows, host.build_model_table(req_models, sw.model_names))
    prb = host.pack_probes(PROBES, sw.model_names)
    want_rows, want_overlap, _ = PM.probe(cols, gof, sw.enabled_mask(), installed, prb[:3], len(sw.model_names))
    assert names == [q[0] for q in PROBES]
    assert np.array_equal(rows, want_rows), (rows, want_rows)
    for k in range(len(PROBES)):
        assert overlap[k] == [(n, int(want_overlap[k, c])) for c, n in enumerate(p.config_names)]
    # the model probes: "h100" / "a100" match some of the interned spec models, "mi355x" none
    by = dict(zip(names, rows))
    assert by["a-or-h"]["eligible_meets"] > 0 and by["a-or-h"]["why"][7] > 0
    assert by["nobody-has"]["eligible_meets"] == 0 and by["nobody-has"]["why"][7] > 0
    assert by["anything"]["eligible_meets"] == int(by["anything"]["why"].sum())
    want_cc = PM.config_overlap(cols, gof, installed, len(sw.model_names))
    lines = [ln.split("\t") for ln in cc_text.splitlines()]
    assert [ln[0] for ln in lines] == p.config_names
    assert np.array_equal(np.array([[int(v) for v in ln[1:]] for ln in lines], dtype=np.uint32), want_cc)
    # a requirement string that does not parse: the constructor's error; invalid sizes: the engine's refusal
    with pytest.raises(RuntimeError, match="broken"):
        probe_configurations(p, [("fine", 1, 1, None), ("broken", 1, 1, "gpu:count=x")])
    with pytest.raises(RuntimeError):
        probe_configurations(p, [("zero", 0, 1, None)])
    assert probe_configurations(p, [])[0] == []
    p.close()
