"""pm_probe_configs / pm_config_overlap on the GPU against the numpy model of tests/probe_model.py: the edges of a wave, a
workgroup, the 64-bit masks and the transpose (W x P x C), every reason code through hand-made probes, every pool state
(before a tick, after one, status changes and dissolutions that have not gone up yet, partial and empty enabled masks), the
identities with the installed configurations probed themselves (pm_config_report, pm_compat_masks, pm_config_overlap), a second
engine that has the probes installed, every refusal with its buffers untouched, and a churn stream on two engines of which
one probes between all its calls."""
import ctypes as C

import numpy as np
import pytest

from protocol_amd import engine as E
from protocol_amd import host
from protocol_amd.churn import ChurnStream
from protocol_amd.swarm import baseline_config, make_swarm, wide_config_swarm

import probe_model as PM
import report_model as RM
from test_probe_model import INSTALLED, SPEC_MODELS, hand_rows, hand_table

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF


def load(sw):
    eng = E.Engine()
    cfg_rows, alt_rows, req_models = host.load_swarm(eng, sw)
    installed = (cfg_rows, alt_rows, host.build_model_table(req_models, sw.model_names))
    return eng, host.pack_workers(sw), installed


_POOL = []


def probe_pool():
    """85 probes: the hand-made requirements (test_probe_model.hand_rows), then 64 wide configurations of another seed"""
    if not _POOL:
        wide = [("w-" + n, mn, mx, req) for n, mn, mx, req in wide_config_swarm(99, 64, 64, 64).configs]
        _POOL.extend([(f"h{i}", 1 + i % 3, 2 + i % 3, r[0]) for i, r in enumerate(hand_rows())] + wide)
    return _POOL


def packed_probes(probes, model_names):
    cfg_rows, alt_rows, bits, n_rows, n_cls = host.pack_probes(probes, model_names)
    return (cfg_rows, alt_rows, bits), n_rows, n_cls


def check_probe(eng, cols, flags, enabled, installed, probes, model_names):
    """one pm_probe_configs call against the model.  The call comes FIRST: pm_get_groups, which the model's group_of comes
    from, compacts the engine's list (what is pending at the call stays pending for it)."""
    prb, n_rows, n_cls = packed_probes(probes, model_names)
    rows, overlap, mask = eng.probe_configs(prb[0], prb[1], prb[2], n_rows, n_cls)
    cc = eng.config_overlap()
    group_of = eng.get_groups()[0]
    w = dict(cols, flags=np.asarray(flags, dtype=np.uint32))
    want_rows, want_overlap, want_mask = PM.probe(w, group_of, enabled, installed, prb, n_cls)
    assert np.array_equal(rows, want_rows), (rows, want_rows)
    assert np.array_equal(overlap, want_overlap)
    assert np.array_equal(mask, want_mask)
    assert np.array_equal(cc, PM.config_overlap(w, group_of, installed, n_cls))
    return rows, overlap, mask, group_of


@pytest.mark.parametrize("C_", [1, 24, 64])
@pytest.mark.parametrize("W", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_shapes(W, C_):
    sw = wide_config_swarm(7 * C_ + 1, 200, W, C_)
    eng, cols, installed = load(sw)
    pool = probe_pool()
    for tick in (False, True):
        if tick:
            eng.tick()
        for P in (1, 2, 63, 64):
            # (P = 1: the probe of three alternatives, P = 2: the two model-row probes; else the first P of the pool)
            probes = {1: pool[19:20], 2: pool[10:12]}.get(P, pool[:P])
            check_probe(eng, cols, cols["flags"], sw.enabled_mask(), installed, probes, sw.model_names)
    eng.close()


def test_baseline_config_0():
    sw = baseline_config(0)
    eng, cols, installed = load(sw)
    pool = probe_pool()
    check_probe(eng, cols, cols["flags"], sw.enabled_mask(), installed, pool[:64], sw.model_names)
    eng.tick()
    rows, _, _, group_of = check_probe(eng, cols, cols["flags"], sw.enabled_mask(), installed, pool[:64], sw.model_names)
    assert (group_of >= 0).any() and (rows["idle_meets"] < rows["eligible_meets"]).any()  # idle != eligible
    eng.close()


def test_hand_made_probes_reach_every_code():
    cols, probes = hand_table(300)  # (five waves, two workgroups)
    cfg_rows, alt_rows, req_models = host.pack_configs(INSTALLED)
    bits = host.build_model_table(req_models, SPEC_MODELS)
    eng = E.Engine()
    eng.set_configs(cfg_rows, alt_rows)
    eng.set_model_table(bits, len(req_models), len(SPEC_MODELS))
    eng.upload_workers(cols)
    installed = (cfg_rows, alt_rows, bits)
    rows, overlap, mask, _ = check_probe(eng, cols, cols["flags"], (1 << 64) - 1, installed, probes, SPEC_MODELS)
    assert (rows["why"].sum(axis=0) > 0).all()  # every reason code is counted somewhere
    # worker i against probe i: the hand-stated code (mask bit <=> code 0)
    want = [r[8] for r in hand_rows()]
    assert [int((int(mask[i]) >> i) & 1) for i in range(len(want))] == [int(c == 0) for c in want]
    names = [p[3] for p in probes]
    assert None in names                                              # a probe without requirements
    p3 = names.index("gpu:count=8;gpu:count=4;gpu:memory_mb=100;gpu:count=1")  # three alternatives, the last one passes
    assert rows["eligible_meets"][p3] > 0
    pm_ = [i for i, n in enumerate(names) if n == "gpu:model=h100"]   # a model-row probe: class 1 passes, class 0 does not
    assert rows["eligible_meets"][pm_[0]] > 0 and rows["why"][pm_[0]][RM.GPU_MODEL] > 0
    # the enabled mask: partial, and 0 (nothing competes: exclusive == idle)
    for enabled in (0b0101, 0b1000, 0):
        eng.set_enabled_mask(enabled)
        r2, _, _, _ = check_probe(eng, cols, cols["flags"], enabled, installed, probes, SPEC_MODELS)
        if enabled == 0:
            assert np.array_equal(r2["idle_exclusive"], r2["idle_meets"]) and r2["idle_meets"].any()
    eng.close()


def test_pool_states():
    sw = make_swarm(3, 600, 3000)
    eng, cols, installed = load(sw)
    pool = probe_pool()
    probes = pool[:40]
    flags = cols["flags"].copy()
    enabled = sw.enabled_mask()
    state = lambda: check_probe(eng, cols, flags, enabled, installed, probes, sw.model_names)
    rows0, _, _, g0 = state()                                     # before any tick: idle == eligible
    assert (g0 < 0).all() and np.array_equal(rows0["idle_meets"], rows0["eligible_meets"])
    eng.tick()
    rows1, _, _, g1 = state()                                     # after a tick: idle != eligible
    assert (g1 >= 0).any() and (rows1["idle_meets"] < rows1["eligible_meets"]).any()
    assert np.array_equal(rows1["why"], rows0["why"])
    # status changes that have not gone up yet: grouped workers die (their groups dissolve), idle ones turn unhealthy
    grouped, idle = np.nonzero(g1 >= 0)[0], np.nonzero((g1 < 0) & ((flags & E.W_HEALTHY) != 0))[0]
    die, sick = grouped[::7][:20], idle[::5][:30]
    who = np.concatenate([die, sick])
    flags[who] &= np.uint32(~E.W_HEALTHY & 0xFFFFFFFF)
    eng.on_worker_status_many(who, flags[who], np.concatenate([np.ones(len(die)), np.zeros(len(sick))]).astype(np.uint32))
    rows2, _, _, g2 = state()
    assert (g2 >= 0).sum() < (g1 >= 0).sum() and rows2["why"].sum() < rows1["why"].sum()
    # a dissolution by id, not pushed yet
    _, groups, _ = eng.get_groups()
    assert eng.dissolve_group_by_id(int(groups[len(groups) // 2]["id"]))
    rows3, _, _, g3 = state()
    assert (g3 >= 0).sum() < (g2 >= 0).sum() and rows3["idle_meets"].sum() > rows2["idle_meets"].sum()
    # a partial enabled mask, then none
    for enabled in (0b101, 0):
        eng.set_enabled_mask(enabled)
        r, _, _, _ = state()
        if enabled == 0:
            assert np.array_equal(r["idle_exclusive"], r["idle_meets"])
    eng.set_enabled_mask(sw.enabled_mask())
    enabled = sw.enabled_mask()
    eng.tick()
    state()
    eng.close()


@pytest.mark.parametrize("which", ["wide64", "mixed"])
def test_probing_the_installed_configurations_themselves(which):
    sw = wide_config_swarm(11, 300, 1000, 64) if which == "wide64" else make_swarm(5, 500, 2500)
    eng, cols, installed = load(sw)
    n_cls = len(sw.model_names)
    _, _, req_models = host.pack_configs(sw.configs)
    for tick in (False, True):
        if tick:
            eng.tick()
        rows, overlap, mask = eng.probe_configs(installed[0], installed[1], installed[2], len(req_models), n_cls)
        rep = eng.config_report()
        assert np.array_equal(rows["why"], rep["why"])
        assert np.array_equal(rows["eligible_meets"], rep["eligible_meets"])
        assert np.array_equal(rows["idle_meets"], rep["idle_meets"])
        assert np.array_equal(mask, eng.compat_masks())
        cc = eng.config_overlap()
        assert np.array_equal(overlap, cc) and np.array_equal(cc, cc.T)
        assert np.array_equal(np.diagonal(cc), rep["idle_meets"])
        mins = installed[0]["min_group_size"]
        assert np.array_equal(rows["groups_max"], rows["idle_meets"] // mins)
        assert np.array_equal(rows["groups_exclusive"], rows["idle_exclusive"] // mins)
    eng.close()


def test_a_second_engine_with_the_probes_installed():
    sw = wide_config_swarm(21, 100, 1000, 24)
    eng, cols, installed = load(sw)
    eng.tick()
    probes = probe_pool()[:64]
    prb, n_rows, n_cls = packed_probes(probes, sw.model_names)
    _, _, mask = eng.probe_configs(prb[0], prb[1], prb[2], n_rows, n_cls, want_overlap=False)
    other = E.Engine()
    other.set_configs(prb[0], prb[1])
    other.set_model_table(prb[2], n_rows, n_cls)
    other.upload_workers(cols)
    assert np.array_equal(other.compat_masks(), mask)
    other.close()
    eng.close()


def test_refusals_leave_the_buffers_untouched():
    L = E.lib()
    sw = make_swarm(3, 200, 500)
    cfg_rows, alt_rows, req_models = host.pack_configs(sw.configs)
    bits = host.build_model_table(req_models, sw.model_names)
    n_cls, Cn = len(sw.model_names), len(cfg_rows)
    prb, n_rows, _ = packed_probes(probe_pool()[:12], sw.model_names)
    assert (prb[1]["flags"] & E.G_MODEL).any()
    rows = np.zeros(64, dtype=E.probe_row_dt)
    rows.view(np.uint8)[:] = 0xAB
    overlap = np.full(64 * 64, 0xABABABAB, dtype=np.uint32)
    mask = np.full(500, 0xABABABABABABABAB, dtype=np.uint64)
    cc = np.full(64 * 64, 0xABABABAB, dtype=np.uint32)
    n_out = C.c_uint32(77)

    def call(eng, cfg=prb[0], n=None, alts=prb[1], n_alts=None, b=prb[2], rows_n=n_rows, cls=n_cls, out=rows):
        return L.pm_probe_configs(eng._h, None if cfg is None else cfg.ctypes.data, len(cfg) if n is None else n,
                                  alts.ctypes.data if len(alts) else None, len(alts) if n_alts is None else n_alts,
                                  b.ctypes.data if b.size else None, rows_n, cls, None if out is None else out.ctypes.data,
                                  overlap.ctypes.data, mask.ctypes.data)

    def untouched():
        assert (rows.view(np.uint8) == 0xAB).all() and (overlap == 0xABABABAB).all() and (cc == 0xABABABAB).all()
        assert (mask == 0xABABABABABABABAB).all()

    eng = E.Engine()
    assert call(eng) == E.PM_ESTATE                                     # nothing uploaded
    assert L.pm_config_overlap(eng._h, cc.ctypes.data, cc.size, C.byref(n_out)) == E.PM_ESTATE
    eng.set_configs(cfg_rows, alt_rows)
    eng.set_model_table(bits, len(req_models), n_cls)
    assert call(eng) == E.PM_ESTATE                                     # no workers yet
    eng.upload_workers(host.pack_workers(sw))
    untouched()
    assert call(eng, n=0) == E.PM_OK                                    # no probes: nothing written
    untouched()
    many = np.zeros(65, dtype=E.config_row_dt)
    many["min_group_size"] = many["max_group_size"] = 1
    assert call(eng, cfg=many) == E.PM_EINVAL                           # more than PM_MAX_CONFIGS
    assert call(eng, cfg=None, n=3) == E.PM_EINVAL and call(eng, out=None) == E.PM_EINVAL   # NULL probes / rows
    bad = prb[0].copy()
    bad["min_group_size"][5] = 0
    assert call(eng, cfg=bad) == E.PM_EINVAL
    bad = prb[0].copy()
    bad["min_group_size"][2], bad["max_group_size"][2] = 3, 2
    assert call(eng, cfg=bad) == E.PM_EINVAL
    assert call(eng, n_alts=len(prb[1]) - 1) == E.PM_ERANGE             # an alternative range outside the table
    bad = prb[0].copy()
    bad["alt_begin"][1], bad["alt_count"][1] = 0xFFFFFFFF, 2            # (the sum must not wrap)
    assert call(eng, cfg=bad) == E.PM_ERANGE
    assert call(eng, cls=n_cls + 1) == E.PM_EINVAL and call(eng, cls=n_cls - 1) == E.PM_EINVAL   # a stale class count
    assert call(eng, rows_n=n_rows - 1) == E.PM_EINVAL                  # a model row outside the table
    assert call(eng, rows_n=0) == E.PM_EINVAL
    untouched()
    # the size query of pm_config_overlap: *n_cfgs always, nothing written below C * C
    assert L.pm_config_overlap(eng._h, None, 0, C.byref(n_out)) == E.PM_ERANGE and n_out.value == Cn
    n_out.value = 77
    assert L.pm_config_overlap(eng._h, cc.ctypes.data, Cn * Cn - 1, C.byref(n_out)) == E.PM_ERANGE and n_out.value == Cn
    untouched()
    assert L.pm_config_overlap(eng._h, cc.ctypes.data, Cn * Cn, None) == E.PM_OK
    assert (cc[Cn * Cn:] == 0xABABABAB).all() and not (cc[:Cn * Cn] == 0xABABABAB).all()
    cc[:] = 0xABABABAB
    # n_classes == 0 with a model alternative: an engine whose table has no classes
    e0 = E.Engine()
    nomodel = np.zeros(2, dtype=E.config_row_dt)
    nomodel["min_group_size"] = nomodel["max_group_size"] = 2
    e0.set_configs(nomodel, np.zeros(0, dtype=E.alt_row_dt))
    e0.upload_workers(host.pack_workers(sw))
    assert call(e0, cls=0) == E.PM_EINVAL
    assert call(e0, cfg=nomodel, alts=np.zeros(0, dtype=E.alt_row_dt), b=np.zeros(0, np.uint32), rows_n=0, cls=0) == E.PM_OK
    assert rows["why"][0].sum() == rows["why"][1].sum() > 0 and (overlap[:2] != 0xABABABAB).all()
    rows.view(np.uint8)[:] = 0xAB
    overlap[:] = 0xABABABAB
    mask[:] = 0xABABABABABABABAB
    e0.close()
    # inside a stepwise tick
    eng.upload_tasks(sw.task_masks(), sw.created_at, sw.task_uid)
    eng.set_enabled_mask(sw.enabled_mask())
    eng.dist_configure(0, 1)
    eng.dist_tick_begin()
    assert call(eng) == E.PM_ESTATE
    assert L.pm_config_overlap(eng._h, cc.ctypes.data, cc.size, C.byref(n_out)) == E.PM_ESTATE
    untouched()
    eng.dist_carve_wait()
    eng.dist_match_begin()
    eng.dist_tick_end()
    assert call(eng) == E.PM_OK and (mask != 0xABABABABABABABAB).all()
    assert (rows.view(np.uint8)[12 * 64:] == 0xAB).all() and (overlap[12 * Cn:] == 0xABABABAB).all()
    eng.close()


def _churn(with_probes):
    ticks = 6
    cs = ChurnStream(31, ticks, W0=2000, n_churn=60, n_new=150, T0=400)
    sw = cs.sw_all
    packed = host.pack_workers(sw)
    take = lambda idx: {k: np.ascontiguousarray(v[idx]) for k, v in packed.items()}
    cfg_rows, alt_rows, req_models = host.pack_configs(sw.configs)
    bits = host.build_model_table(req_models, sw.model_names)
    prb, n_rows, n_cls = packed_probes(probe_pool()[:30], sw.model_names)
    eng = E.Engine(group_id_seed=5)
    eng.set_configs(cfg_rows, alt_rows)
    eng.set_model_table(bits, len(req_models), n_cls)
    eng.upload_workers(take(np.arange(cs.W0)))
    eng.upload_tasks(cs.masks, cs.created, cs.uid)
    eng.set_enabled_mask(sw.enabled_mask())
    eng.enable_group_events()
    flags = packed["flags"].astype(np.int64).copy()
    n_probed = [0]

    def probe():
        if with_probes:
            eng.probe_configs(prb[0], prb[1], prb[2], n_rows, n_cls)
            eng.config_overlap()
            n_probed[0] += 1

    trace = []

    def snapshot(W, stats):
        group_of, groups, members = eng.get_groups()
        table = [(a.task, a.group_slot, a.group_index, a.group_size, a.next_worker, a.group_id)
                 for a in (eng.lookup(w) for w in range(W))]
        trace.append((stats["n_formed"], stats["n_groups"], group_of.tolist(), groups.tolist(), members.tolist(), table,
                      [(k, g, c, list(m)) for k, g, c, m in eng.drain_group_events()]))

    probe()
    snapshot(cs.W0, eng.tick())
    probe()
    for _ in range(ticks):
        leave, idx_new, new_tasks = cs.step()
        flags[leave] &= ~E.W_HEALTHY
        eng.on_worker_status_many(leave, flags[leave], np.ones(len(leave), dtype=np.uint32))
        probe()
        eng.append_workers(take(idx_new))
        probe()
        eng.tasks_insert_front(*new_tasks[:3])
        probe()
        stats = eng.tick()
        probe()
        snapshot(cs.W, stats)
    pushes = eng.debug_delta_pushes()
    eng.close()
    return trace, pushes, n_probed[0]


def test_probes_between_all_calls_change_nothing():
    plain, pushes_plain, _ = _churn(False)
    probed, pushes, n = _churn(True)
    assert n == 2 + 4 * 6
    assert len(plain) == len(probed) == 7
    for k, (a, b) in enumerate(zip(plain, probed)):
        assert a == b, f"tick {k}: the engine that probes differs"
    assert pushes == pushes_plain
    assert sum(t[0] for t in plain) > 0 and any(t[6] for t in plain[1:])
