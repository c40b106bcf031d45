#!/usr/bin/env python3
"""The group directory on the host's clock at 10,000 and 100,000 worker rows (or the sizes given), groups and claims from a real
pm_tick over a seeded swarm, most members Healthy and the rest over the seven other statuses, a report on most rows: the
counters alone, a first and a middle page of 100 in each order, the degraded filter, the full list.  p50, min and max of REPS
calls after WARM warm-ups; every engine call ends on a stream synchronise before it returns, so the host's clock sees the whole
of it.  Beside each, what a host does today (tools/groupdir_host_loop.cpp): pm_get_groups with every member, pm_liveness_get
over every row, pm_rollout_groups, the join, a sort of the id texts, the page cut on one thread — whose window must equal the
engine's.  The ratio is reported, not asserted.

Everything printed is also written to --out (default profiles/r28_group_directory.txt).  --bench DIR appends the comparison of
`python bench.py --gpus 1 --steps 21 --warmup 3` on the parent commit's build and on this one (bench_<k>_parent.json /
bench_<k>_change.json, k = the order they ran in); --bench-only skips the GPU part.
usage: python tools/groupdir_probe.py [W ...] [--out FILE] [--bench DIR] [--bench-only]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28_group_directory.txt"))
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
    say("   alternating in one GPU session; bench.py never calls pm_group_directory.  Order: " + " ".join(r[0][0] for r in rows) +
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
so = os.path.join(tempfile.mkdtemp(), "libgdir_host.so")
subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                       os.path.join(ROOT, "tools", "groupdir_host_loop.cpp"), "-L", os.path.dirname(B.LIB_PATH), "-lpm_engine",
                       "-Wl,-rpath," + os.path.dirname(B.LIB_PATH), "-o", so])
H = C.CDLL(so)
vp, u32 = C.c_void_p, C.c_uint32
H.gdir_host_query.argtypes = [vp, u32, u32, vp, vp, vp, vp, u32, C.POINTER(u32), vp, u32, C.POINTER(u32)]
ALL = 7
DEGRADED = (1 << E.GH_LOST) | (1 << E.GH_DEGRADED)
ORDERS = ((E.GDIR_BY_SLOT, "by slot"), (E.GDIR_BY_ID_TEXT, "by id text"), (E.GDIR_BY_SIZE_DESC, "by size"))


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
    rng = np.random.default_rng(28)
    sw = make_swarm(7, 10_000, W)
    eng = E.Engine(group_id_seed=1)
    host.load_swarm(eng, sw)
    eng.liveness_enable(True)
    eng.rollout_enable(True)
    eng.tick()
    # most nodes Healthy, the rest over the seven other statuses, as a pool looks between two sweeps
    statuses = np.where(rng.random(W) < 0.9, E.NS_HEALTHY, rng.integers(0, E.NS_N, W)).astype(np.uint8)
    eng.liveness_set(np.arange(W, dtype=np.uint32), statuses, np.zeros(W, dtype=np.uint32))
    group_of, groups, members = eng.get_groups()
    G, M = len(groups), len(members)
    # nine rows in ten report their group's claimed task, most of them RUNNING
    uid_of_task = np.asarray(sw.task_uid, dtype=np.uint64)
    rows = np.flatnonzero((group_of >= 0) & (rng.random(W) < 0.9))
    rows = rows[groups["task"][group_of[rows]] != E.PM_NONE]
    reps = np.zeros(len(rows), dtype=E.ro_report_dt)
    reps["worker"] = rows
    reps["state"] = np.where(rng.random(len(rows)) < 0.9, E.TS_RUNNING, rng.integers(0, E.TS_N, len(rows)))
    reps["uid"] = uid_of_task[groups["task"][group_of[rows]]]
    eng.rollout_ingest(reps)

    q = np.zeros(1, dtype=E.gdir_query_dt)
    bufs = [(np.zeros(1, dtype=E.gdir_totals_dt), np.zeros(64, dtype=np.uint32), np.zeros(max(G, 1), dtype=E.gdir_row_dt),
             np.zeros(max(M, 1), dtype=np.uint32)) for _ in range(2)]

    def fill(health, order, offset, limit):
        q[0] = (0xFFFFFFFFFFFFFFFF, E.GDIR_ANY, 0, 0xFFFFFFFF, health, ALL, order, offset, limit)

    def one_call(k=0):
        """ONE pm_group_directory into buffers with room for every row and member, as a caller that pages does"""
        t, c, r, m = bufs[k]
        n, nm = u32(0), u32(0)
        E.check(E.lib().pm_group_directory(eng._h, q.ctypes.data, t.ctypes.data, c.ctypes.data, 64, r.ctypes.data, len(r), C.byref(n),
                                           m.ctypes.data, len(m), C.byref(nm)))
        return n.value, nm.value

    def host_query(k=1):
        t, c, r, m = bufs[k]
        n, nm = u32(0), u32(0)
        rc = H.gdir_host_query(eng._h, W, eng.C, q.ctypes.data, t.ctypes.data, c.ctypes.data, r.ctypes.data, len(r), C.byref(n),
                               m.ctypes.data, len(m), C.byref(nm))
        assert rc == 0, rc
        return n.value, nm.value

    fill(ALL, E.GDIR_BY_SLOT, 0, 0)
    one_call()
    t = bufs[0][0][0]
    say("== group directory (MEASURED) at W = %d worker rows, %d groups of a real tick with %d members, health %s, rollout %s; "
        "p50 of %d calls after %d warm-ups" % (W, G, M, t["by_health"].tolist(), t["by_rollout"].tolist(), REPS, WARM))
    shapes = [("counters only (limit 0)", ALL, E.GDIR_BY_SLOT, 0, 0)]
    shapes += [("first page of 100, " + name, ALL, o, 0, 100) for o, name in ORDERS]
    shapes += [("page of 100 in the middle, " + name, ALL, o, G // 2, 100) for o, name in ORDERS]
    shapes += [("lost or degraded, first 100, by id text", DEGRADED, E.GDIR_BY_ID_TEXT, 0, 100),
               ("lost or degraded, all, by id text", DEGRADED, E.GDIR_BY_ID_TEXT, 0, 0xFFFFFFFF)]
    shapes += [("the full list, " + name, ALL, o, 0, 0xFFFFFFFF) for o, name in ORDERS]
    for name, health, order, offset, limit in shapes:
        fill(health, order, offset, limit)
        got, want = one_call(), host_query()
        # the host loop holds the same tables: its counters and its window are the engine's, byte for byte
        assert got == want, (name, got, want)
        assert bufs[0][0].tobytes() == bufs[1][0].tobytes() and bufs[0][1].tobytes() == bufs[1][1].tobytes(), name
        assert bufs[0][2][:got[0]].tobytes() == bufs[1][2][:got[0]].tobytes(), name
        assert bufs[0][3][:got[1]].tobytes() == bufs[1][3][:got[1]].tobytes(), name
        gpu = timed(one_call)
        cpu = timed(host_query)
        say("  %-42s %6d groups   engine p50 %8.3f ms  min %8.3f  max %8.3f   host loop p50 %8.3f ms   ratio %6.2fx  (%.2f MB out)"
            % (name, got[0], med(gpu), min(gpu), max(gpu), med(cpu), med(cpu) / med(gpu), (got[0] * 80 + got[1] * 4) / 1e6))
    eng.close()


for W in args.W:
    probe(W)
    say()
if args.bench:
    bench_table(args.bench)
with open(args.out, "w") as f:
    f.write("\n".join(LINES) + "\n")
