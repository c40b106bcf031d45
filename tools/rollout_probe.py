#!/usr/bin/env python3
"""The rollout ledger on the host's clock at W worker rows (default 100,000), groups and claims from a real pm_tick over a seeded
swarm: a full-swarm ingest (every row reports), then each of the four reads.  Median, min and max of REPS calls after WARM
warm-ups; every engine call ends on a stream synchronise before it returns, so the host's clock sees the whole of it.  Beside each,
the same work as plain C++ on one host thread over the same columns (tools/rollout_host_loop.cpp), whose classes and per-task
table must equal the engine's.  The ratio is reported, not asserted.

Everything printed is also written to --out (default profiles/r26_rollout.txt).  --bench DIR appends the comparison of
`python bench.py --gpus 1 --steps 21 --warmup 3` on the parent commit's build and on this one (bench_<k>_parent.json /
bench_<k>_change.json, k = the order they ran in); --bench-only skips the GPU part.
usage: python tools/rollout_probe.py [W] [--out FILE] [--bench DIR] [--bench-only]"""
import argparse
import ctypes as C
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("W", nargs="?", type=int, default=100_000)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_rollout.txt"))
ap.add_argument("--bench", default=None)
ap.add_argument("--bench-only", action="store_true")
args = ap.parse_args()
W = args.W
LINES = []
WARM, REPS = 3, 15
med = lambda v: float(np.median(v))


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def bench_table(d):
    """ms_per_step and churn.ms_per_tick of every line, and where this commit's values lie in the parent's spread"""
    rows = []
    files = glob.glob(os.path.join(d, "bench_*_parent.json")) + glob.glob(os.path.join(d, "bench_*_change.json"))
    for f in sorted(files, key=lambda f: int(re.search(r"bench_(\d+)_", f).group(1))):
        j = json.loads([ln for ln in open(f) if ln.startswith("{")][-1])
        rows.append(("parent" if "parent" in os.path.basename(f) else "change", j["ms_per_step"], j["churn"]["ms_per_tick"]))
    say()
    say("== the feature unused (MEASURED): `python bench.py --gpus 1 --steps 21 --warmup 3` on the parent commit's build and on this one,")
    say("   alternating in one GPU session; bench.py never calls pm_rollout_*.  Order: " + " ".join(r[0][0] for r in rows) +
        " (p = parent, c = this commit)")
    for j, name in ((1, "ms_per_step"), (2, "churn.ms_per_tick")):
        say("  " + name)
        lo, hi = (f(r[j] for r in rows if r[0] == "parent") for f in (min, max))
        for w in ("parent", "change"):
            v = [r[j] for r in rows if r[0] == w]
            say("    %s  %s   median %.4f   min %.4f   max %.4f" % (w, " ".join("%.4f" % x for x in v), med(v), min(v), max(v)))
        m = med([r[j] for r in rows if r[0] == "change"])
        say("    the parent's spread is [%.4f, %.4f]: this commit's median %.4f lies %s"
            % (lo, hi, m, "inside" if lo <= m <= hi else "BELOW" if m < lo else "ABOVE"))


if args.bench_only:
    bench_table(args.bench)
    with open(args.out, "a") as f:
        f.write("\n".join(LINES) + "\n")
    sys.exit(0)

sys.path.insert(0, ROOT)
from protocol_amd import engine as E  # noqa: E402
from protocol_amd import host  # noqa: E402
from protocol_amd.swarm import make_swarm  # noqa: E402

so = os.path.join(tempfile.mkdtemp(), "libro_host.so")
subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                       os.path.join(ROOT, "tools", "rollout_host_loop.cpp"), "-o", so])
H = C.CDLL(so)
vp, u32 = C.c_void_p, C.c_uint32
H.ro_host_reset.argtypes = [u32]
H.ro_host_ingest.argtypes = [vp, u32]
H.ro_host_classify.argtypes = [vp, vp, vp, u32, vp, vp, vp]
H.ro_host_tasks.argtypes = [vp, vp, vp, vp, u32, vp, u32]
H.ro_host_tasks.restype = u32

rng = np.random.default_rng(26)
sw = make_swarm(7, 10_000, W)
eng = E.Engine(group_id_seed=1)
host.load_swarm(eng, sw)
eng.rollout_enable(True)
eng.tick()
group_of, groups, _ = eng.get_groups()
G = len(groups)
uids = np.asarray(sw.task_uid, dtype=np.uint64)
g_has = (groups["task"] != 0xFFFFFFFF).astype(np.uint8)
g_claim = uids[np.minimum(groups["task"], len(uids) - 1)].copy()
g_claim[g_has == 0] = 0
g_size = np.ascontiguousarray(groups["n_members"], dtype=np.uint32)
group_of = np.ascontiguousarray(group_of, dtype=np.int32)


def batch():
    """every row reports: three in four of a task-holding group's members its task (most of them RUNNING), the rest and the free
    workers some task of the list or an id no task carries"""
    r = np.zeros(W, dtype=E.ro_report_dt)
    r["worker"] = np.arange(W)
    has = (group_of >= 0) & (g_has[np.maximum(group_of, 0)] != 0)
    roll = rng.random(W)
    uid = rng.integers(1, 1 << 62, W, dtype=np.uint64)                       # (uint64 throughout: no id passes through a float)
    listed = roll < 0.95
    uid[listed] = uids[rng.integers(0, len(uids), W)][listed]
    own = has & (roll < 0.75)
    uid[own] = g_claim[np.maximum(group_of, 0)][own]
    r["uid"] = uid
    r["state"] = np.where(rng.random(W) < 0.8, E.TS_RUNNING, rng.integers(0, E.TS_N, W))
    return r


def timed(call, reps=REPS, warm=WARM):
    out = []
    for k in range(warm + reps):
        t0 = time.perf_counter()
        call()
        dt = (time.perf_counter() - t0) * 1e3
        if k >= warm:
            out.append(dt)
    return out


def line(name, gpu, host_ms, note=""):
    say("  %-36s engine median %8.3f ms  min %8.3f  max %8.3f   host loop %9.3f ms   ratio %6.1fx  %s"
        % (name, med(gpu), min(gpu), max(gpu), host_ms, host_ms / med(gpu), note))


say("== rollout ledger (MEASURED) at W = %d worker rows, %d groups of a real tick (%d hold a task), %d tasks; %d calls after %d warm-ups"
    % (W, G, int(g_has.sum()), len(uids), REPS, WARM))
batches = [batch() for _ in range(WARM + REPS)]
it = iter(batches)
t_ing = timed(lambda: eng.rollout_ingest(next(it)))
H.ro_host_reset(W)
t0 = time.perf_counter()
for b in batches:
    H.ro_host_ingest(b.ctypes.data, W)
host_ing = (time.perf_counter() - t0) * 1e3 / len(batches)
line("ingest, %d reports" % W, t_ing, host_ing, "(%.1f MB in)" % (W * 16 / 1e6))

cls = np.zeros(W, dtype=np.uint8)
g_cnt = np.zeros((max(G, 1), E.TS_N + 2), dtype=np.uint32)
by_class = np.zeros(E.RO_N, dtype=np.uint32)
h_cls = timed(lambda: H.ro_host_classify(group_of.ctypes.data, g_claim.ctypes.data, g_has.ctypes.data, G, cls.ctypes.data,
                                         g_cnt.ctypes.data, by_class.ctypes.data), reps=5, warm=1)
h_rows = np.zeros(W + G, dtype=E.ro_task_row_dt)
h_tasks = timed(lambda: H.ro_host_tasks(group_of.ctypes.data, g_claim.ctypes.data, g_has.ctypes.data, g_size.ctypes.data, G,
                                        h_rows.ctypes.data, len(h_rows)), reps=5, warm=1)
n_host = H.ro_host_tasks(group_of.ctypes.data, g_claim.ctypes.data, g_has.ctypes.data, g_size.ctypes.data, G, h_rows.ctypes.data, len(h_rows))

summary = eng.rollout_summary()
tasks, grows, workers = eng.rollout_tasks(), eng.rollout_groups(), eng.rollout_workers()
# the host loop holds the same ledger: its classes, group counters and per-task table are the engine's
assert summary["by_class"].tolist() == by_class.tolist() and workers["cls"].tolist() == cls.tolist(), "classes differ from the host loop's"
want = h_rows[:n_host].copy()
got = tasks.copy()
got["task"] = 0xFFFFFFFF
assert got.tobytes() == want.tobytes(), "the per-task table differs from the host loop's"
listed = np.nonzero(g_has)[0]
assert np.array_equal(np.column_stack([grows["same"], grows["other"], grows["silent"]]), g_cnt[listed]), "group counters differ"

line("summary (classify + sort + reduce)", timed(eng.rollout_summary), med(h_cls) + med(h_tasks), "(%d distinct ids)" % len(tasks))
line("tasks (%d rows of 64 B)" % len(tasks), timed(eng.rollout_tasks), med(h_cls) + med(h_tasks))
line("groups (%d rows of 64 B)" % len(grows), timed(eng.rollout_groups), med(h_cls))
line("workers, every class (%d rows of 24 B)" % len(workers), timed(eng.rollout_workers), med(h_cls), "(%.1f MB out)" % (len(workers) * 24 / 1e6))
lag = (1 << E.RO_OTHER) | (1 << E.RO_BEHIND) | (1 << E.RO_SILENT)
line("workers, OTHER | BEHIND | SILENT (%d)" % len(eng.rollout_workers(lag)), timed(lambda: eng.rollout_workers(lag)), med(h_cls))
say("  by_class (idle, stray, silent, other, behind, converged) = %s; groups converged %d of %d"
    % (summary["by_class"].tolist(), int(summary["groups_converged"]), int(summary["groups_with_task"])))
eng.close()

if args.bench:
    bench_table(args.bench)
with open(args.out, "w") as f:
    f.write("\n".join(LINES) + "\n")
