#!/usr/bin/env python3
"""The node directory on the host's clock at 10,000 and 100,000 worker rows (or the sizes given), groups and claims from a real
pm_tick over a seeded swarm, statuses drawn over all eight, a report on every second row: the counters alone, the first page of
100 by row and by address, a page in the middle, the full list.  p50, min and max of REPS calls after WARM warm-ups; every engine
call ends on a stream synchronise before it returns, so the host's clock sees the whole of it.  Beside each, what a host does today
(tools/directory_host_loop.cpp): pm_liveness_get over every row, pm_get_groups, pm_rollout_get over every row, a std::stable_sort,
the join and the page cut on one thread — whose rows must equal the engine's.  The ratio is reported, not asserted.

Everything printed is also written to --out (default profiles/r27_directory.txt).  --bench DIR appends the comparison of
`python bench.py --gpus 1 --steps 21 --warmup 3` on the parent commit's build and on this one (bench_<k>_parent.json /
bench_<k>_change.json, k = the order they ran in); --bench-only skips the GPU part.
usage: python tools/directory_probe.py [W ...] [--out FILE] [--bench DIR] [--bench-only]"""
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
ap.add_argument("W", nargs="*", type=int, default=[10_000, 100_000])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_directory.txt"))
ap.add_argument("--bench", default=None)
ap.add_argument("--bench-only", action="store_true")
args = ap.parse_args()
LINES = []
WARM, REPS = 20, 200
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
    say("   alternating in one GPU session; bench.py never calls pm_directory.  Order: " + " ".join(r[0][0] for r in rows) +
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
so = os.path.join(tempfile.mkdtemp(), "libdir_host.so")
subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                       os.path.join(ROOT, "tools", "directory_host_loop.cpp"), "-L", os.path.dirname(B.LIB_PATH), "-lpm_engine",
                       "-Wl,-rpath," + os.path.dirname(B.LIB_PATH), "-o", so])
H = C.CDLL(so)
vp, u32 = C.c_void_p, C.c_uint32
H.dir_host_query.argtypes = [vp, u32, vp, u32, u32, u32, u32, C.POINTER(u32), vp, vp, u32, C.POINTER(u32)]
ALL = (1 << E.NS_N) - 1
NOT_DEAD = ALL & ~(1 << E.NS_DEAD)


def timed(call):
    out = []
    for k in range(WARM + REPS):
        t0 = time.perf_counter()
        call()
        dt = (time.perf_counter() - t0) * 1e3
        if k >= WARM:
            out.append(dt)
    return out


def probe(W):
    rng = np.random.default_rng(27)
    sw = make_swarm(7, 10_000, W)
    eng = E.Engine(group_id_seed=1)
    host.load_swarm(eng, sw)
    eng.liveness_enable(True)
    eng.rollout_enable(True)
    eng.tick()
    # most nodes Healthy, the rest over the seven other statuses, as a pool looks between two sweeps
    statuses = np.where(rng.random(W) < 0.7, E.NS_HEALTHY, rng.integers(0, E.NS_N, W)).astype(np.uint8)
    eng.liveness_set(np.arange(W, dtype=np.uint32), statuses, rng.integers(0, 9, W).astype(np.uint32))
    reps = np.zeros(W // 2, dtype=E.ro_report_dt)
    reps["worker"] = np.arange(0, W - 1, 2)[:W // 2]
    reps["state"] = rng.integers(0, E.TS_N, W // 2)
    reps["uid"] = np.asarray(sw.task_uid, dtype=np.uint64)[rng.integers(0, len(sw.task_uid), W // 2)]
    eng.rollout_ingest(reps)
    ranks = np.ascontiguousarray(sw.addr_rank(), dtype=np.uint32)
    group_of, groups, _ = eng.get_groups()
    buf = np.zeros(W, dtype=E.dir_row_dt)

    def host_query(mask, order, offset, limit):
        total, n, counts = u32(0), u32(0), np.zeros(E.NS_N, dtype=np.uint32)
        rc = H.dir_host_query(eng._h, W, ranks.ctypes.data, mask, order, offset, limit, C.byref(total), counts.ctypes.data,
                              buf.ctypes.data, W, C.byref(n))
        assert rc == 0, rc
        return total.value, counts, buf[:n.value]

    out = np.zeros(W, dtype=E.dir_row_dt)
    q = np.zeros(1, dtype=E.dir_query_dt)

    def one_call(mask, order, offset, limit):
        """ONE pm_directory into a buffer with room for every row, as a caller that pages does (no size query in front)"""
        q[0] = (mask, E.DIR_ANY, order, offset, limit)
        total, n, counts = u32(0), u32(0), np.zeros(E.NS_N, dtype=np.uint32)
        E.check(E.lib().pm_directory(eng._h, q.ctypes.data, C.byref(total), counts.ctypes.data, out.ctypes.data, W, C.byref(n)))
        return n.value

    say("== node directory (MEASURED) at W = %d worker rows, %d groups of a real tick, %d grouped rows, statuses %s; p50 of %d calls "
        "after %d warm-ups" % (W, len(groups), int((group_of >= 0).sum()), np.bincount(statuses, minlength=E.NS_N).tolist(), REPS, WARM))
    total = eng.directory(NOT_DEAD, limit=0)[0]
    shapes = [("counters only (limit 0)", ALL, E.DIR_BY_ROW, 0, 0),
              ("first page of 100, by row", NOT_DEAD, E.DIR_BY_ROW, 0, 100),
              ("first page of 100, by address", NOT_DEAD, E.DIR_BY_ADDRESS, 0, 100),
              ("page of 100 in the middle, by row", NOT_DEAD, E.DIR_BY_ROW, total // 2, 100),
              ("page of 100 in the middle, by address", NOT_DEAD, E.DIR_BY_ADDRESS, total // 2, 100),
              ("the full list, by row", ALL, E.DIR_BY_ROW, 0, 0xFFFFFFFF),
              ("the full list, by address", ALL, E.DIR_BY_ADDRESS, 0, 0xFFFFFFFF)]
    for name, mask, order, offset, limit in shapes:
        lim = None if limit == 0xFFFFFFFF else limit
        got = eng.directory(mask, E.DIR_ANY, order, offset, lim)
        want = host_query(mask, order, offset, limit)
        # the host loop holds the same tables: its window is the engine's, byte for byte
        assert got[0] == want[0] and got[1].tolist() == want[1].tolist() and got[2].tobytes() == want[2].tobytes(), name
        gpu = timed(lambda: one_call(mask, order, offset, limit))
        cpu = timed(lambda: host_query(mask, order, offset, limit))
        say("  %-40s %6d rows   engine p50 %8.3f ms  min %8.3f  max %8.3f   host loop p50 %8.3f ms   ratio %6.2fx  (%.2f MB out)"
            % (name, len(got[2]), med(gpu), min(gpu), max(gpu), med(cpu), med(cpu) / med(gpu), len(got[2]) * 48 / 1e6))
    eng.close()


for W in args.W:
    probe(W)
    say()
if args.bench:
    bench_table(args.bench)
with open(args.out, "w") as f:
    f.write("\n".join(LINES) + "\n")
