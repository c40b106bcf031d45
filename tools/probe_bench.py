#!/usr/bin/env python3
"""What a probe costs: pm_probe_configs with P = 8, P = 24 and P = 64 probes (overlap and masks asked for), pm_config_overlap,
and — the yardstick, existing code — pm_config_report, on the same engines in the same run: BASELINE configs[1] (10,000 workers)
and configs[2] (100,000 workers) after a tick, and a 10,000-worker swarm with 24 configurations installed.  Host clock around
each call (each one ends in a stream synchronisation); the median of `reps` calls after two warm-up calls.  The probes are the
first P of 64 wide configurations (protocol_amd.swarm.wide_config_swarm: counts, models, memory bounds, cpu, ram, storage),
packed against the swarm's model names.
usage: python tools/probe_bench.py [reps]      (under rocprofv3 --kernel-trace --stats for the kernels' durations)"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from protocol_amd import engine as E, host
from protocol_amd.swarm import baseline_config, wide_config_swarm

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
pool = wide_config_swarm(99, 64, 64, 64).configs


def timed(call):
    for _ in range(2):
        call()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t)), float(np.min(t))


# (the third case has 24 configurations installed: P = 24 probes beside the report for as many configurations)
for name, make in (("configs[1]", lambda: baseline_config(1)), ("configs[2]", lambda: baseline_config(2)),
                   ("wide, C = 24", lambda: wide_config_swarm(5, 10000, 10000, 24))):
    sw = make()
    eng = E.Engine()
    host.load_swarm(eng, sw)
    eng.tick()
    print(f"{name}: W {sw.W}, T {sw.T}, C {len(sw.configs)} installed, after a tick; ms per call, median (min) of {reps}")
    med, lo = timed(eng.config_report)
    print(f"  pm_config_report                       {med:8.3f} ({lo:.3f})")
    med, lo = timed(eng.config_overlap)
    print(f"  pm_config_overlap                      {med:8.3f} ({lo:.3f})")
    for P in (8, 24, 64):
        cfg_rows, alt_rows, bits, n_rows, n_cls = host.pack_probes(pool[:P], sw.model_names)
        for what, kw in (("overlap + masks", {}), ("rows only", dict(want_overlap=False, want_mask=False))):
            med, lo = timed(lambda: eng.probe_configs(cfg_rows, alt_rows, bits, n_rows, n_cls, **kw))
            print(f"  pm_probe_configs P = {P:2d}, {what:15s} {med:8.3f} ({lo:.3f})")
    eng.close()
