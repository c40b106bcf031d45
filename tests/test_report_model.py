"""The numpy restatement of the diagnostics reports (tests/report_model.py) against the CPU oracle: a reason code is 0
exactly when the oracle's compat bit is set, on make_swarm seeds, on wide_config_swarm up to 64 configurations and on every
`meets` known-answer vector of node.rs; the state and both reports on hand-made inputs."""
import json
import os

import numpy as np
import pytest

from oracle import oracle_ffi as orc
from protocol_amd import engine as E
from protocol_amd import host
from protocol_amd.swarm import make_swarm, wide_config_swarm

import report_model as RM

KATS = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "node_rs_kats.json")))


def model_why(sw):
    cfg_rows, alt_rows, req_models = host.pack_configs(sw.configs)
    bits = host.build_model_table(req_models, sw.model_names)
    return RM.why_codes(host.pack_workers(sw), cfg_rows, alt_rows, bits, len(sw.model_names))


def check_against_oracle(sw):
    why = model_why(sw)
    nodes, cfgs, _tasks, _enabled = orc.from_swarm(sw)
    masks = orc.compat_masks(nodes, cfgs)
    C = len(sw.configs)
    bits = ((masks[:, None] >> np.arange(C, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
    assert np.array_equal(why == 0, bits)
    assert why.max() < 10
    return why


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_codes_match_the_oracle_on_make_swarm(seed):
    why = check_against_oracle(make_swarm(seed, 200, 3000))
    assert (why != 0).any() and (why == 0).any()


@pytest.mark.parametrize("C", [1, 33, 63, 64])
def test_codes_match_the_oracle_on_wide_configs(C):
    check_against_oracle(wide_config_swarm(C, 300, 2000, C))


def kat_worker(specs):
    """the engine columns of create_compute_specs(count, model, mem, cores, ram, storage) (oracle.make_specs)"""
    count, model, mem, cores, ram, storage = (list(specs) + [None] * 6)[:6]
    f = E.W_HAS_SPECS | E.W_HEALTHY | E.W_HAS_P2P
    if count is not None or model is not None or mem is not None:
        f |= E.W_HAS_GPU
        f |= (E.W_GPU_COUNT if count is not None else 0) | (E.W_GPU_MEM if mem is not None else 0)
        f |= E.W_GPU_MODEL if model is not None else 0
    if cores is not None:
        f |= E.W_HAS_CPU | E.W_CPU_CORES
    f |= (E.W_RAM if ram is not None else 0) | (E.W_STORAGE if storage is not None else 0)
    col = lambda v: np.array([0 if v is None else v], dtype=np.uint32)
    return dict(flags=np.array([f], dtype=np.uint32), gpu_count=col(count), gpu_mem_mb=col(mem),
                gpu_model_class=col(0), cpu_cores=col(cores), ram_mb=col(ram), storage_gb=col(storage)), model


@pytest.mark.parametrize("kat", KATS["meets"], ids=lambda k: k["name"])
def test_codes_match_every_meets_vector(kat):
    w, model = kat_worker(kat["specs"])
    cfg_rows, alt_rows, req_models = host.pack_configs([("kat", 1, 1, kat["req"])])
    bits = host.build_model_table(req_models, [model or ""])
    why = RM.why_codes(w, cfg_rows, alt_rows, bits, 1)
    specs = orc.make_specs(*kat["specs"])
    code, req, err = orc.parse_requirements(kat["req"])
    assert code == 0, err
    assert orc.meets(specs, req) is kat["expect"]
    assert (int(why[0, 0]) == 0) is kat["expect"], int(why[0, 0])


def one(req, **specs):
    """the code of one kat-style worker for one requirement string"""
    w, model = kat_worker([specs.get(k) for k in ("count", "model", "mem", "cores", "ram", "storage")])
    cfg_rows, alt_rows, req_models = host.pack_configs([("x", 1, 1, req)])
    bits = host.build_model_table(req_models, [model or ""])
    return int(RM.why_codes(w, cfg_rows, alt_rows, bits, 1)[0, 0])


def test_every_code_is_reached():
    assert one(None, count=1) == RM.OK
    assert one("cpu:cores=4", ram=10) == RM.CPU
    assert one("cpu:cores=4", cores=2) == RM.CPU
    assert one("ram_mb=100", ram=10) == RM.RAM
    assert one("storage_gb=100", storage=10) == RM.STORAGE
    assert one("gpu:count=1", ram=10) == RM.GPU_NONE
    assert one("gpu:count=2", count=1) == RM.GPU_COUNT
    assert one("gpu:count=1", mem=10) == RM.GPU_COUNT            # count None, required 1
    assert one("gpu:count=0", mem=10) == RM.OK                   # count None passes a required 0
    assert one("gpu:model=h100", count=1, model="A100") == RM.GPU_MODEL
    assert one("gpu:memory_mb=100", count=1, mem=10) == RM.GPU_MEM
    assert one("gpu:total_memory_min=1", count=65536, mem=65536) == RM.GPU_TOTAL   # 2^32 wraps to 0
    assert one("gpu:total_memory_max=0", count=65536, mem=65536) == RM.OK
    # the largest code over alternatives: count fails in the first, memory (further on) in the second
    assert one("gpu:count=8;gpu:count=1;gpu:memory_mb=100", count=1, mem=10) == RM.GPU_MEM
    # no specs at all, with and without requirements
    w = dict(flags=np.array([E.W_HEALTHY], dtype=np.uint32), gpu_count=np.zeros(1, np.uint32),
             gpu_mem_mb=np.zeros(1, np.uint32), gpu_model_class=np.zeros(1, np.uint32), cpu_cores=np.zeros(1, np.uint32),
             ram_mb=np.zeros(1, np.uint32), storage_gb=np.zeros(1, np.uint32))
    cfg_rows, alt_rows, _ = host.pack_configs([("a", 1, 1, "ram_mb=1"), ("b", 1, 1, None)])
    assert RM.why_codes(w, cfg_rows, alt_rows).tolist() == [[RM.NO_SPECS, RM.OK]]


def test_state_and_reports_on_a_small_table():
    flags = np.array([E.W_HEALTHY | E.W_HAS_P2P, E.W_HEALTHY, E.W_HAS_P2P, E.W_HEALTHY | E.W_HAS_P2P,
                      E.W_HEALTHY | E.W_HAS_P2P], dtype=np.uint32)
    group_of = np.array([0, -1, 0, -1, 1])
    assert RM.worker_state(flags, group_of).tolist() == [E.WS_IN_GROUP, E.WS_NO_P2P, E.WS_IN_GROUP, E.WS_IDLE,
                                                         E.WS_IN_GROUP]
    why = np.array([[0, 3], [0, 0], [0, 2], [0, 0], [5, 0]], dtype=np.uint8)
    groups = [(0, 2, 1), (1, 1, -1)]
    masks = np.array([1, 2, 3, ~np.uint64(0)], dtype=np.uint64)
    rep = RM.config_report(why, flags, group_of, 0b01, groups, masks)
    assert rep["enabled"].tolist() == [1, 0]
    assert rep["why"][0].tolist() == [2, 0, 0, 0, 0, 1, 0, 0, 0, 0]   # rows 0, 3 (eligible), row 4: code 5
    assert rep["why"][1].tolist() == [2, 0, 0, 1, 0, 0, 0, 0, 0, 0]
    assert rep["idle_meets"].tolist() == [1, 1]
    assert rep["groups"].tolist() == [1, 1] and rep["members"].tolist() == [2, 1]
    assert rep["groups_without_task"].tolist() == [0, 1]
    assert rep["tasks_allowing"].tolist() == [3, 3]
    running, workers, allowed = RM.task_report(groups, masks, 2)
    assert running.tolist() == [0, 1, 0, 0] and workers.tolist() == [0, 2, 0, 0]
    assert allowed.tolist() == [1, 1, 2, 2]
