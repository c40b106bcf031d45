#!/usr/bin/env python3
"""The task directory on the host's clock at 100,000 tasks over 10,000 workers and 1,000,000 tasks over 100,000 workers (or the
T:W pairs given), groups and claims from a real pm_tick over a seeded swarm, a report on most grouped rows and on a few rows that
name a task nobody lists: the counters alone, a first and a middle page of 100 in each order, the starved filter, the full list.
p50, min and max of REPS calls after WARM warm-ups; every engine call ends on a stream synchronise before it returns, so the host's
clock sees the whole of it.  Beside each, what a host does today (tools/taskdir_host_loop.cpp): pm_task_report's three arrays and
pm_rollout_tasks fetched whole, a hash-map join on ids, classification, filter and sort on one thread — whose counters and window
must equal the engine's.  Every ratio is reported as measured, not asserted; below 1 the directory loses.

Everything printed is also written to --out (default profiles/r29_task_directory.txt).  --bench DIR appends the comparison of
`python bench.py --gpus 1 --steps 21 --warmup 3` on the parent commit's build and on this one (bench_<k>_parent.json /
bench_<k>_change.json, k = the order they ran in); --bench-only skips the GPU part.
usage: python tools/taskdir_probe.py [T:W ...] [--out FILE] [--bench DIR] [--bench-only]"""
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
ap.add_argument("sizes", nargs="*", default=["100000:10000", "1000000:100000"])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29_task_directory.txt"))
ap.add_argument("--bench", default=None)
ap.add_argument("--bench-only", action="store_true")
ap.add_argument("--reps", type=int, default=40)
args = ap.parse_args()
LINES = []
WARM, REPS = 5, args.reps
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
    say("   alternating in one GPU session; bench.py never calls pm_task_directory.  Order: " + " ".join(r[0][0] for r in rows) +
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
from protocol_amd import build as B  # noqa: E402
from protocol_amd import engine as E  # noqa: E402
from protocol_amd import host  # noqa: E402
from protocol_amd.swarm import make_swarm  # noqa: E402

E.lib()
so = os.path.join(tempfile.mkdtemp(), "libtdir_host.so")
subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                       os.path.join(ROOT, "tools", "taskdir_host_loop.cpp"), "-L", os.path.dirname(B.LIB_PATH), "-lpm_engine",
                       "-Wl,-rpath," + os.path.dirname(B.LIB_PATH), "-o", so])
H = C.CDLL(so)
vp, u32 = C.c_void_p, C.c_uint32
H.tdir_host_query.argtypes = [vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, u32, C.POINTER(u32)]
ALL = 7
ORDERS = ((E.TDIR_BY_LIST, "by list"), (E.TDIR_BY_OLDEST, "oldest first"), (E.TDIR_BY_WORKERS_DESC, "by workers"),
          (E.TDIR_BY_REPORTERS_DESC, "by reporters"))


def timed(call):
    out = []
    for k in range(WARM + REPS):
        t0 = time.perf_counter()
        call()
        dt = (time.perf_counter() - t0) * 1e3
        if k >= WARM:
            out.append(dt)
    return out


def probe(T, W):
    rng = np.random.default_rng(29)
    sw = make_swarm(7, T, W)
    eng = E.Engine(group_id_seed=1)
    host.load_swarm(eng, sw)
    eng.rollout_enable(True)
    eng.tick()
    group_of, groups, members = eng.get_groups()
    uid = np.ascontiguousarray(sw.task_uid, dtype=np.uint64)
    created = np.ascontiguousarray(sw.created_at, dtype=np.int64)
    masks = np.ascontiguousarray(sw.task_masks(), dtype=np.uint64)
    # nine grouped rows in ten report their group's claimed task, most of them RUNNING; one free row in ten reports a task nobody lists
    rows = np.flatnonzero((group_of >= 0) & (rng.random(W) < 0.9))
    rows = rows[groups["task"][group_of[rows]] != E.PM_NONE]
    reps = np.zeros(len(rows), dtype=E.ro_report_dt)
    reps["worker"] = rows
    reps["state"] = np.where(rng.random(len(rows)) < 0.9, E.TS_RUNNING, rng.integers(0, E.TS_N, len(rows)))
    reps["uid"] = uid[groups["task"][group_of[rows]]]
    eng.rollout_ingest(reps)
    free = np.flatnonzero((group_of < 0) & (rng.random(W) < 0.1))
    lost = np.zeros(len(free), dtype=E.ro_report_dt)
    lost["worker"], lost["state"], lost["uid"] = free, E.TS_RUNNING, 5 + (free % 97)
    eng.rollout_ingest(lost)

    q = np.zeros(1, dtype=E.tdir_query_dt)
    bufs = [(np.zeros(1, dtype=E.tdir_totals_dt), np.zeros(64, dtype=np.uint32), np.zeros(max(T, 1), dtype=E.tdir_row_dt)) for _ in range(2)]

    def fill(serve, order, offset, limit):
        q[0] = (0xFFFFFFFFFFFFFFFF, serve, ALL, 0, 0xFFFFFFFF, order, offset, limit, 0)

    def one_call(k=0):
        """ONE pm_task_directory into a buffer with room for every row, as a caller that pages does"""
        t, c, r = bufs[k]
        n = u32(0)
        E.check(E.lib().pm_task_directory(eng._h, q.ctypes.data, t.ctypes.data, c.ctypes.data, 64, r.ctypes.data, len(r), C.byref(n)))
        return n.value

    def host_query(k=1):
        t, c, r = bufs[k]
        n = u32(0)
        rc = H.tdir_host_query(eng._h, T, eng.C, uid.ctypes.data, created.ctypes.data, masks.ctypes.data, q.ctypes.data, t.ctypes.data,
                               c.ctypes.data, r.ctypes.data, len(r), C.byref(n))
        assert rc == 0, rc
        return n.value

    fill(ALL, E.TDIR_BY_LIST, 0, 0)
    one_call()
    t = bufs[0][0][0]
    say("== task directory (MEASURED) at T = %d tasks over W = %d worker rows, %d groups of a real tick, serve %s, rollout %s, %d orphan "
        "ids of %d rows; p50 of %d calls after %d warm-ups" % (T, W, len(groups), t["by_serve"].tolist(), t["by_rollout"].tolist(),
                                                             int(t["orphan_uids"]), int(t["orphan_reporters"]), REPS, WARM))
    shapes = [("counters only (limit 0)", ALL, E.TDIR_BY_LIST, 0, 0)]
    shapes += [("first page of 100, " + name, ALL, o, 0, 100) for o, name in ORDERS]
    shapes += [("page of 100 in the middle, " + name, ALL, o, T // 2, 100) for o, name in ORDERS]
    shapes += [("starved, first 100, by list", 1 << E.TKS_STARVED, E.TDIR_BY_LIST, 0, 100),
               ("starved, all, by list", 1 << E.TKS_STARVED, E.TDIR_BY_LIST, 0, 0xFFFFFFFF)]
    shapes += [("the full list, " + name, ALL, o, 0, 0xFFFFFFFF) for o, name in ORDERS]
    for name, serve, order, offset, limit in shapes:
        fill(serve, order, offset, limit)
        got, want = one_call(), host_query()
        # the host loop holds the same tables: its counters and its window are the engine's, byte for byte
        assert got == want, (name, got, want)
        assert bufs[0][0].tobytes() == bufs[1][0].tobytes() and bufs[0][1].tobytes() == bufs[1][1].tobytes(), name
        assert bufs[0][2][:got].tobytes() == bufs[1][2][:got].tobytes(), name
        gpu = timed(one_call)
        cpu = timed(host_query)
        say("  %-42s %8d tasks   engine p50 %9.3f ms  min %9.3f  max %9.3f   host loop p50 %9.3f ms   ratio %6.2fx  (%.2f MB out)"
            % (name, got, med(gpu), min(gpu), max(gpu), med(cpu), med(cpu) / med(gpu), got * 88 / 1e6))
    # where a call's time goes with the ledger on: the same counters-only query with the ledger off has no id join
    fill(ALL, E.TDIR_BY_LIST, 0, 0)
    on = med(timed(one_call))
    eng.rollout_enable(False)
    off = med(timed(one_call))
    say("  counters only: %.3f ms with the rollout ledger on, %.3f ms with it off — the difference is the ledger's per-task table, the "
        "upload of the live ids and the eight passes of the id join" % (on, off))
    eng.close()


for size in args.sizes:
    T, W = (int(x) for x in size.split(":"))
    probe(T, W)
    say()
if args.bench:
    bench_table(args.bench)
with open(args.out, "w") as f:
    f.write("\n".join(LINES) + "\n")
