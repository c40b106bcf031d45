"""The numpy model of the probe calls (tests/probe_model.py) against brute force: hand-made (requirement, worker) pairs that
reach every reason code, as probes over a 30-worker table with every worker state, counted pair by pair in plain loops."""
import numpy as np

from protocol_amd import engine as E
from protocol_amd import host

import probe_model as PM
import report_model as RM

SPEC_MODELS = ["NVIDIA A100 80GB", "NVIDIA H100 PCIe"]


def hand_rows():
    """(requirement, flags, count, mem, model class, cores, ram, storage, code): worker i against requirement i gives `code`;
    the cases of test_gpu_report.hand_rows, with a model row that matches (class 1) beside the one that does not (class 0)"""
    base = E.W_HAS_SPECS | E.W_HEALTHY | E.W_HAS_P2P
    G = E.W_HAS_GPU
    return [
        (None, E.W_HEALTHY | E.W_HAS_P2P, 0, 0, 0, 0, 0, 0, RM.OK),                  # no requirements, no specs
        ("ram_mb=1", E.W_HEALTHY | E.W_HAS_P2P, 0, 0, 0, 0, 0, 0, RM.NO_SPECS),
        ("cpu:cores=4", base | E.W_RAM, 0, 0, 0, 0, 10, 0, RM.CPU),                 # no cpu
        ("cpu:cores=4", base | E.W_HAS_CPU | E.W_CPU_CORES, 0, 0, 0, 2, 0, 0, RM.CPU),
        ("ram_mb=100", base | E.W_RAM, 0, 0, 0, 0, 10, 0, RM.RAM),
        ("storage_gb=100", base | E.W_STORAGE, 0, 0, 0, 0, 0, 10, RM.STORAGE),
        ("gpu:count=1", base | E.W_RAM, 0, 0, 0, 0, 10, 0, RM.GPU_NONE),
        ("gpu:count=2", base | G | E.W_GPU_COUNT, 1, 0, 0, 0, 0, 0, RM.GPU_COUNT),
        ("gpu:count=1", base | G | E.W_GPU_MEM, 0, 10, 0, 0, 0, 0, RM.GPU_COUNT),  # count None, required 1
        ("gpu:count=0", base | G | E.W_GPU_MEM, 0, 10, 0, 0, 0, 0, RM.OK),         # count None, required 0
        ("gpu:model=h100", base | G | E.W_GPU_COUNT | E.W_GPU_MODEL, 1, 0, 0, 0, 0, 0, RM.GPU_MODEL),
        ("gpu:model=h100", base | G | E.W_GPU_COUNT | E.W_GPU_MODEL, 1, 0, 1, 0, 0, 0, RM.OK),     # the model row matches
        ("gpu:memory_mb=100", base | G | E.W_GPU_COUNT | E.W_GPU_MEM, 1, 10, 0, 0, 0, 0, RM.GPU_MEM),
        ("gpu:memory_mb_max=5", base | G | E.W_GPU_COUNT | E.W_GPU_MEM, 1, 10, 0, 0, 0, 0, RM.GPU_MEM),
        ("gpu:total_memory_min=1", base | G | E.W_GPU_COUNT | E.W_GPU_MEM, 65536, 65536, 0, 0, 0, 0, RM.GPU_TOTAL),
        ("gpu:total_memory_max=0", base | G | E.W_GPU_COUNT | E.W_GPU_MEM, 65536, 65536, 0, 0, 0, 0, RM.OK),
        ("gpu:total_memory_max=15", base | G | E.W_GPU_COUNT | E.W_GPU_MEM, 2, 10, 0, 0, 0, 0, RM.GPU_TOTAL),
        ("gpu:count=8;gpu:count=1;gpu:memory_mb=100", base | G | E.W_GPU_COUNT | E.W_GPU_MEM, 1, 10, 0, 0, 0, 0,
         RM.GPU_MEM),                                                                # the largest code over alternatives
        ("gpu:count=1;gpu:model=h100;gpu:count=8", base | G | E.W_GPU_COUNT | E.W_GPU_MODEL, 1, 0, 0, 0, 0, 0,
         RM.GPU_MODEL),
        ("gpu:count=8;gpu:count=4;gpu:memory_mb=100;gpu:count=1", base | G | E.W_GPU_COUNT | E.W_GPU_MEM, 1, 10, 0, 0, 0, 0,
         RM.OK),                                                                     # three alternatives, the last one passes
        ("cpu:cores=4;ram_mb=100", base | E.W_HAS_CPU | E.W_CPU_CORES, 0, 0, 0, 8, 0, 0, RM.RAM),  # first failing clause
    ]


def hand_table(n_workers=30):
    """the hand rows' workers, repeated up to n_workers with their state varied (every third repeat unhealthy or without a p2p
    id, half of them located), and the hand requirements as probes named h0.."""
    rows = hand_rows()
    pick = [i % len(rows) for i in range(n_workers)]
    col = lambda k: np.array([rows[i][k] for i in pick], dtype=np.uint32)
    flags = col(1)
    for w in range(len(rows), n_workers):
        if w % 3 == 0:
            flags[w] &= np.uint32(~E.W_HEALTHY & 0xFFFFFFFF)
        if w % 3 == 1:
            flags[w] &= np.uint32(~E.W_HAS_P2P & 0xFFFFFFFF)
    flags[::2] |= np.uint32(E.W_HAS_LOC)
    n = n_workers
    cols = dict(flags=flags, gpu_count=col(2), gpu_mem_mb=col(3), gpu_model_class=col(4), cpu_cores=col(5), ram_mb=col(6),
                storage_gb=col(7), price=np.zeros(n, np.uint32), addr_rank=np.arange(n, dtype=np.uint32),
                lat=np.linspace(-60.0, 60.0, n), lon=np.linspace(-170.0, 170.0, n))
    probes = [(f"h{i}", 1 + i % 3, 2 + i % 3, r[0]) for i, r in enumerate(rows)]
    return cols, probes


INSTALLED = [("big", 2, 4, "gpu:count=1"), ("any", 1, 2, None), ("ram", 1, 3, "ram_mb=5"), ("h100", 2, 2, "gpu:model=h100")]


def packed(configs):
    cfg_rows, alt_rows, req_models = host.pack_configs(configs)
    return cfg_rows, alt_rows, host.build_model_table(req_models, SPEC_MODELS)


def test_hand_rows_reach_every_code_as_probes():
    rows = hand_rows()
    cols, probes = hand_table(len(rows))
    p = packed(probes)
    why = RM.why_codes(cols, p[0], p[1], p[2], len(SPEC_MODELS))
    want = [r[8] for r in rows]
    assert np.diagonal(why).tolist() == want
    assert set(want) == set(range(10))
    assert any(r[0] is None for r in rows)
    assert any(int(c["alt_count"]) == 3 and r[8] == RM.OK for c, r in zip(p[0], rows))  # a later alternative of three passes


def brute(cols, group_of, enabled, why_p, why_c, min_sizes):
    W, P = why_p.shape
    C = why_c.shape[1]
    rows = np.zeros(P, dtype=E.probe_row_dt)
    overlap = np.zeros((P, C), dtype=np.uint32)
    mask = [0] * W
    for w in range(W):
        f = int(cols["flags"][w])
        elig = bool(f & E.W_HEALTHY) and bool(f & E.W_HAS_P2P)
        idle = elig and group_of[w] < 0
        meets_enabled = any(why_c[w, c] == 0 and (enabled >> c) & 1 for c in range(C))
        for p in range(P):
            ok = why_p[w, p] == 0
            if ok:
                mask[w] |= 1 << p
            if elig:
                rows[p]["why"][why_p[w, p]] += 1
            if idle and ok:
                rows[p]["idle_meets"] += 1
                rows[p]["idle_located"] += bool(f & E.W_HAS_LOC)
                rows[p]["idle_exclusive"] += not meets_enabled
                for c in range(C):
                    overlap[p, c] += why_c[w, c] == 0
    for p in range(P):
        rows[p]["eligible_meets"] = rows[p]["why"][0]
        rows[p]["groups_max"] = rows[p]["idle_meets"] // min_sizes[p]
        rows[p]["groups_exclusive"] = rows[p]["idle_exclusive"] // min_sizes[p]
    return rows, overlap, np.array(mask, dtype=np.uint64)


def test_model_against_brute_force_on_30_workers():
    cols, probes = hand_table(30)
    group_of = np.full(30, -1)
    group_of[[0, 4, 9, 22]] = 0      # grouped rows: eligible, not idle
    group_of[[11, 25]] = 1
    inst, prb = packed(INSTALLED), packed(probes)
    n_cls = len(SPEC_MODELS)
    why_c = RM.why_codes(cols, inst[0], inst[1], inst[2], n_cls)
    why_p = RM.why_codes(cols, prb[0], prb[1], prb[2], n_cls)
    mins = [p[1] for p in probes]
    for enabled in (0b1111, 0b0101, 0):
        rows, overlap, mask = PM.probe(cols, group_of, enabled, inst, prb, n_cls)
        b_rows, b_overlap, b_mask = brute(cols, group_of, enabled, why_p, why_c, mins)
        assert np.array_equal(rows, b_rows), (rows, b_rows)
        assert np.array_equal(overlap, b_overlap) and np.array_equal(mask, b_mask)
        if enabled == 0:
            assert np.array_equal(rows["idle_exclusive"], rows["idle_meets"])
    rows, overlap, _ = PM.probe(cols, group_of, 0b1111, inst, prb, n_cls)
    assert (rows["idle_meets"] < rows["eligible_meets"]).any()      # idle != eligible
    assert (rows["idle_located"] < rows["idle_meets"]).any() and rows["idle_located"].any()
    assert (rows["idle_exclusive"] == 0).all()                      # "any" (no requirements) is enabled and meets everyone
    assert np.array_equal(overlap[:, 1], rows["idle_meets"])        # ... so its column is idle_meets
    # the C x C matrix: symmetric, the diagonal = the probes-of-themselves' idle_meets
    cc = PM.config_overlap(cols, group_of, inst, n_cls)
    self_rows, self_overlap, _ = PM.probe(cols, group_of, 0b1111, inst, inst, n_cls)
    assert np.array_equal(cc, cc.T) and np.array_equal(np.diagonal(cc), self_rows["idle_meets"])
    assert np.array_equal(cc, self_overlap)
