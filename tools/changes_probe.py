#!/usr/bin/env python3
"""The assignment change feed at BASELINE configs[4] (the churn stream of bench.py's `churn` sub-object, protocol_amd/churn.py):
what a tick costs with the feed on and with it off, and what a drain costs at the rows a churn tick changes.

Switching the feed on is a resync (the next publish lists all 100k rows), so one engine cannot alternate between the two within
a stream.  Two engines in one process get the same stream instead, one with the feed on and one with it off; every tick is
timed on both (host clock around pm_tick, the stream idle before it), in alternating order.  The drain is timed as its two calls
(the size query, which makes the list on the device, and the copy-out), after the tick's timing.
usage: python tools/changes_probe.py [ticks]      (under rocprofv3 --kernel-trace --stats for the kernels' durations)"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from protocol_amd import engine as E, host
from protocol_amd.churn import ChurnStream

ticks = int(sys.argv[1]) if len(sys.argv) > 1 else 10
WARM = 2
cs = ChurnStream(1, WARM + ticks)
sw_all = cs.sw_all
packed = host.pack_workers(sw_all)
rows = lambda idx: {k: np.ascontiguousarray(v[idx]) for k, v in packed.items()}
flags = packed["flags"].astype(np.int64)
cfg_rows, alt_rows, req_models = host.pack_configs(sw_all.configs)


def engine(feed):
    eng = E.Engine()
    eng.set_configs(cfg_rows, alt_rows)
    eng.set_model_table(host.build_model_table(req_models, sw_all.model_names), len(req_models), len(sw_all.model_names))
    eng.upload_workers(rows(np.arange(cs.W0)))
    eng.upload_tasks(cs.masks, cs.created, cs.uid)
    eng.set_enabled_mask(sw_all.enabled_mask())
    if feed:
        eng.enable_assignment_changes()
    eng.tick()
    return eng


on, off = engine(True), engine(False)
w, what, resync = on.drain_assignment_changes()
print(f"cold match: W {cs.W0}, {len(w)} rows drained, resync {resync}")
t_on, t_off, t_drain, n_rows = [], [], [], []
for k in range(WARM + ticks):
    leave, idx_new, new_tasks = cs.step()
    for eng in (on, off):
        eng.on_worker_status_many(leave, flags[leave] & ~E.W_HEALTHY, np.ones(len(leave), dtype=np.uint32))
        eng.append_workers(rows(idx_new))
        eng.tasks_insert_front(*new_tasks[:3])
    ms = {}
    for eng in ((on, off) if k % 2 == 0 else (off, on)):
        t0 = time.perf_counter()
        eng.tick()
        ms[eng is on] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    w, what, resync = on.drain_assignment_changes()
    d = 1e3 * (time.perf_counter() - t0)
    assert np.all(np.diff(w.astype(np.int64)) > 0)
    # (a tick behind a rebuild of the task table's index space — this stream outgrows it every eighth tick — is a resync: it
    # lists every row; it is printed, and left out of the medians)
    if k >= WARM and not resync:
        t_on.append(ms[True]), t_off.append(ms[False]), t_drain.append(d), n_rows.append(len(w))
    print(f"tick {k}{' (warm-up)' if k < WARM else ''}{' RESYNC' if resync else ''}: W {cs.W}, feed on {ms[True]:.3f} ms, off {ms[False]:.3f} ms, drain {d:.3f} ms "
          f"for {len(w)} rows (group {int((what & 1 != 0).sum())}, ring {int((what & 2 != 0).sum())}, task {int((what & 4 != 0).sum())})")
med = lambda v: float(np.median(v))
print(f"ms per tick, median of {len(t_on)}: feed on {med(t_on):.3f}, feed off {med(t_off):.3f} (on - off {med(t_on) - med(t_off):+.3f})")
print(f"drain (size query + copy-out), median: {med(t_drain):.3f} ms per call pair at {int(med(n_rows))} rows")
# what assign_diff_kernel must move per publish: a row of d_table (32 B) and a remembered identity (32 B) read per worker, a task
# word (4 B) per grouped worker; an identity (32 B) and a `what` byte (read + write) per changed row; a bitmap word per 64 rows
W, n = cs.W, int(med(n_rows))
print(f"assign_diff_kernel bytes per publish at W {W}, {n} changed rows: {W * 68 + n * 34 + (W + 63) // 64 * 8:,}")
on.close(), off.close()
