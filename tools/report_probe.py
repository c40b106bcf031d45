#!/usr/bin/env python3
"""What the diagnostics reports cost (pm_explain_workers over every row, pm_config_report, pm_task_report, the group
geography reports pm_group_spread / pm_config_spread, and the nearest-candidates query pm_nearest_workers for 1 and 256
queries at k = 64 and 256, with the bytes one query reads: 56 a worker row) at BASELINE
configs[1] and configs[2] after a cold match, and beside them a churn tick's ms_compat (BASELINE configs[4], the stream of
bench.py's `churn` sub-object).  Host wall clock per call, median of `reps` calls after one warm-up; prints one JSON line.
usage: python tools/report_probe.py [reps]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from protocol_amd import engine as E, host
from protocol_amd.churn import ChurnStream
from protocol_amd.swarm import baseline_config

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10


def timed(fn):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ts)), 3)


def nearest(eng, sw):
    """pm_nearest_workers: one query from the seed, one and 256 by index (origins and configurations spread over the table)"""
    C = len(sw.configs)
    q256 = [(i * sw.W // 256, i % C) for i in range(256)]
    q256 = np.array(q256, dtype=E.near_query_dt)
    seed = np.array([(E.NEAR_SEED, 0)], dtype=E.near_query_dt)
    r = dict(mb_read_per_query=round(56 * sw.W / 1e6, 2))
    for k in (64, 256):
        r[f"ms_seed_k{k}"] = timed(lambda: eng.nearest_workers(seed, E.NEAR_IDLE, k))
        for pool, tag in ((E.NEAR_IDLE, "idle"), (E.NEAR_ELIGIBLE, "eligible")):
            r[f"ms_q1_k{k}_{tag}"] = timed(lambda: eng.nearest_workers(q256[128:129], pool, k))
            r[f"ms_q256_k{k}_{tag}"] = timed(lambda: eng.nearest_workers(q256, pool, k))
    return r


out = {}
for cfg in (1, 2):
    sw = baseline_config(cfg, seed=1)
    eng = E.Engine()
    host.load_swarm(eng, sw)
    s = eng.tick()
    out[f"cfg{cfg}"] = dict(W=sw.W, T=sw.T, C=len(sw.configs), n_groups=s["n_groups"], ms_tick=round(s["ms_total"], 3),
                            ms_explain_all=timed(eng.explain_workers), ms_explain_one=timed(lambda: eng.explain_workers([0])),
                            ms_config_report=timed(eng.config_report), ms_task_report=timed(eng.task_report),
                            ms_group_spread=timed(eng.group_spread), ms_config_spread=timed(eng.config_spread),
                            nearest=nearest(eng, sw))
    eng.close()

# a churn tick's ms_compat, and the reports in the middle of the stream (status changes pending, the group list carrying
# tombstones): the state they are called in between a deployment's ticks
cs = ChurnStream(1, 8)
sw_all = cs.sw_all
packed = host.pack_workers(sw_all)
rows = lambda idx: {k: np.ascontiguousarray(v[idx]) for k, v in packed.items()}
eng = E.Engine()
cfg_rows, alt_rows, req_models = host.pack_configs(sw_all.configs)
eng.set_configs(cfg_rows, alt_rows)
eng.set_model_table(host.build_model_table(req_models, sw_all.model_names), len(req_models), len(sw_all.model_names))
eng.upload_workers(rows(np.arange(cs.W0)))
eng.upload_tasks(cs.masks, cs.created, cs.uid)
eng.set_enabled_mask(sw_all.enabled_mask())
eng.tick()
flags = packed["flags"].astype(np.int64)
compat, tick = [], []
for t in range(4):
    leave, idx_new, new_tasks = cs.step()
    eng.on_worker_status_many(leave, flags[leave] & ~E.W_HEALTHY, np.ones(len(leave), dtype=np.uint32))
    eng.append_workers(rows(idx_new))
    eng.tasks_insert_front(*new_tasks[:3])
    if t == 3:
        out["churn_pending"] = dict(W=cs.W, ms_explain_all=timed(eng.explain_workers), ms_config_report=timed(eng.config_report),
                                    ms_task_report=timed(eng.task_report), ms_group_spread=timed(eng.group_spread),
                                    ms_config_spread=timed(eng.config_spread))
    s = eng.tick()
    compat.append(s["ms_compat"])
    tick.append(s["ms_total"])
out["churn_tick"] = dict(ms_compat_median=round(float(np.median(compat)), 3), ms_total_median=round(float(np.median(tick)), 3))
eng.close()
print(json.dumps(out))
