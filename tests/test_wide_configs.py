"""CPU checks of protocol_amd.swarm.wide_config_swarm, the generator behind tests/test_gpu_config_width.py: its
configurations are valid for the product's host layer, every configuration index is named by a task and met by a
worker (the oracle says which), requirements reach the model table's third word, and the output is a function of the
seed.  No GPU."""
import numpy as np
import pytest

from oracle import oracle_ffi as orc
from protocol_amd import engine as E
from protocol_amd import host
from protocol_amd.swarm import MIXED_CONFIGS, WIDE_MODELS, make_swarm, wide_config_swarm

SIZES = [1, 2, 3, 4, 5, 24, 31, 32, 33, 63, 64]


@pytest.mark.parametrize("C", SIZES)
def test_configurations_are_valid_and_distinct(C):
    sw = wide_config_swarm(3, 200, 300, C)
    assert len(sw.configs) == C
    names = [c[0] for c in sw.configs]
    assert len(set(names)) == C and all(len(n.encode()) < orc.NAME_LEN for n in names)
    assert all(1 <= mn <= mx <= 16 for _n, mn, mx, _r in sw.configs)
    cfg_rows, _alts, req_models = host.pack_configs(sw.configs)
    assert all(len(m.encode()) < orc.MODEL_LEN for m in sw.model_names + req_models)
    full = (1 << C) - 1
    order = host.config_order(cfg_rows, full)
    assert sorted(order) == list(range(C))
    # the order over a part of the set is that part, in the same relative order (pm_host_config_order)
    part = full & 0xA5A5A5A5A5A5A5A5
    assert host.config_order(cfg_rows, part) == [c for c in order if (part >> c) & 1]
    # the oracle's tables take them as they are
    code, o_order = orc.sort_configs(orc.from_swarm(sw)[1])
    assert code == 0 and sorted(o_order.tolist()) == list(range(C))


@pytest.mark.parametrize("C", SIZES)
def test_every_index_is_named_and_met(C):
    sw = wide_config_swarm(5, 2 * C + 10, 4 * C + 7, C)
    nodes, cfgs, _tasks, _enabled = orc.from_swarm(sw)
    masks = orc.compat_masks(nodes, cfgs)
    healthy = (sw.status == 2) & sw.has_p2p
    met = int(np.bitwise_or.reduce(masks[healthy])) if healthy.any() else 0
    full = (1 << C) - 1
    assert met == full, hex(met ^ full)
    assert sw.enabled_mask() == full
    assert sw.topo.shape[1] == orc.MAX_TOPO and (sw.n_topo <= orc.MAX_TOPO).all()
    # the topology lists and the masks the host derives from them agree
    tm = sw.task_masks()
    for t in range(sw.T):
        names = {int(c) for c in sw.topo[t, :sw.n_topo[t]] if c >= 0}
        assert (int(tm[t]) == (1 << 64) - 1) if not sw.restricted[t] else int(tm[t]) == sum(1 << c for c in names)
        assert (sw.topo[t, sw.n_topo[t]:] == -2).all()
    assert (~sw.restricted).any() and (sw.restricted & (tm == 0)).any()  # unrestricted tasks and ghost-only ones


def test_model_classes_reach_the_third_word():
    sw = wide_config_swarm(7, 200, 500, 64)
    assert len(sw.model_names) == len(WIDE_MODELS) == 70 and len(set(sw.model_names)) == 70
    cfg_rows, _alts, req_models = host.pack_configs(sw.configs)
    words = (len(sw.model_names) + 31) // 32
    assert words == 3
    bits = host.build_model_table(req_models, sw.model_names).reshape(len(req_models), words)
    assert bits[:, 1].any() and bits[:, 2].any()
    # a requirement that selects a class >= 32 is met by a worker of that class (through the oracle's predicate)
    nodes, cfgs, _t, _e = orc.from_swarm(sw)
    masks = orc.compat_masks(nodes, cfgs)
    hi_cfgs = [i for i, (_n, _a, _b, r) in enumerate(sw.configs) if r and "zeta-k" in r]
    assert hi_cfgs
    hi_met = [i for i in hi_cfgs if (sw.gpu_model_id[(masks >> np.uint64(i)) & np.uint64(1) == 1] >= 32).any()]
    assert len(hi_met) >= len(hi_cfgs) // 2
    assert (sw.gpu_model_id >= 64).any()


def test_output_is_a_function_of_the_seed():
    def fields(sw):
        out = [sw.configs, sw.model_names]
        for k in ("address", "status", "gpu_count", "gpu_mem_mb", "gpu_model_id", "cpu_cores", "ram_mb", "storage_gb",
                  "lat", "lon", "created_at", "task_uid", "restricted", "n_topo", "topo"):
            out.append(getattr(sw, k).tolist())
        return out
    a, b = wide_config_swarm(11, 500, 700, 64), wide_config_swarm(11, 500, 700, 64)
    assert fields(a) == fields(b)
    c = wide_config_swarm(12, 500, 700, 64)
    assert fields(a) != fields(c)
    assert not np.array_equal(a.task_masks(), c.task_masks())
    # created_at descending (TaskStore::get_all_tasks order), uids distinct
    assert (np.diff(a.created_at) <= 0).all() and len(np.unique(a.task_uid)) == a.T
    with pytest.raises(ValueError):
        wide_config_swarm(1, 10, 10, 65)
    with pytest.raises(ValueError):
        wide_config_swarm(1, 10, 10, 0)


def test_make_swarm_is_untouched():
    """the committed scale / churn digests depend on make_swarm's output: the wide generator shares its streams' code
    but none of its tables"""
    sw = make_swarm(1, 50, 40)
    assert sw.configs == MIXED_CONFIGS and len(sw.model_names) == 12 and sw.topo.shape[1] == 3
    assert int(sw.task_masks()[0]) == 0x40400 and int(sw.address[0]) == 3150992677718134148
