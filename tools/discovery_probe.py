#!/usr/bin/env python3
"""pm_discovery_sync on the host's clock at W table rows (default 100,000), three shapes: (a) the usual pass — every node
listed, endpoints almost all distinct, 1 % new rows, 1 % demoted; (b) 1,000 new rows on a table that shares 100 endpoints;
(c) the worst case — half the list Healthy on ONE endpoint, half new on the same.  Median, min and max of 50 calls after 5
warm-ups (between two calls the ledger is put back with pm_liveness_set, outside the timing), the bytes a call moves, and
beside each shape one run of the reference-shaped D x W loop as plain C++ on one host thread (tools/discovery_host_loop.cpp,
integer ids instead of strings: it flatters the reference), whose counts and final statuses must equal the engine's.

Everything printed is also written to --out (default profiles/r19_discovery.txt).  --bench DIR appends the comparison of
`python bench.py --gpus 1 --steps 21 --warmup 3` on the parent commit's build and on this one (bench_<k>_parent.json /
bench_<k>_change.json, k = the order they ran in); --bench-only skips the GPU part and appends a further session.
usage: python tools/discovery_probe.py [W] [--out FILE] [--bench DIR] [--bench-only]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_discovery.txt"))
ap.add_argument("--bench", default=None)
ap.add_argument("--bench-only", action="store_true")
args = ap.parse_args()
W = args.W
LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


WARM, REPS = 5, 50
NOW = 1_760_000_000_000
med = lambda v: float(np.median(v))


def bench_table(d):
    """ms_per_step and churn.ms_per_tick of every line, and where this commit's values lie in the parent's spread"""
    rows = []
    files = glob.glob(os.path.join(d, "bench_*_parent.json")) + glob.glob(os.path.join(d, "bench_*_change.json"))
    for f in sorted(files, key=lambda f: int(re.search(r"bench_(\d+)_", f).group(1))):
        j = json.loads([ln for ln in open(f) if ln.startswith("{")][-1])
        rows.append(("parent" if "parent" in os.path.basename(f) else "change", j["ms_per_step"], j["churn"]["ms_per_tick"],
                     j["churn"]["split_ms_p50"]))
    say()
    say("== the feature unused: `python bench.py --gpus 1 --steps 21 --warmup 3` on the parent commit's build and on this one, alternating")
    say("   in one GPU session; bench.py never calls pm_discovery_sync.  Order: " + " ".join(r[0][0] for r in rows) + " (p = parent, c = this commit)")
    for j, name in ((1, "ms_per_step"), (2, "churn.ms_per_tick")):
        say("  " + name)
        lo, hi = (f(r[j] for r in rows if r[0] == "parent") for f in (min, max))
        for w in ("parent", "change"):
            v = [r[j] for r in rows if r[0] == w]
            say("    %s  %s   median %.4f   min %.4f   max %.4f" % (w, " ".join("%.4f" % x for x in v), med(v), min(v), max(v)))
        m = med([r[j] for r in rows if r[0] == "change"])
        say("    the parent's spread is [%.4f, %.4f]: this commit's median %.4f lies %s" % (lo, hi, m, "inside" if lo <= m <= hi else "BELOW" if m < lo else "ABOVE"))
    say("  churn phases (p50 of a run's six ticks; ms_per_tick is status + append + tasks + match), per run")
    for w in ("parent", "change"):
        for k in ("status_ms", "append_ms", "tasks_ms", "match_ms"):
            say("    %s  %-7s %s" % (w, k[:-3], " ".join("%.3f" % r[3][k] for r in rows if r[0] == w)))


if args.bench_only:
    bench_table(args.bench)
    with open(args.out, "a") as f:
        f.write("\n".join(LINES) + "\n")
    sys.exit(0)

sys.path.insert(0, ROOT)
from protocol_amd import engine as E

tmp = tempfile.mkdtemp()
so = os.path.join(tmp, "disc_host_loop.so")
subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                       os.path.join(ROOT, "tools", "discovery_host_loop.cpp"), "-o", so])
HOST = C.CDLL(so)
HOST.disc_host_pass.restype = C.c_uint32
HOST.disc_host_pass.argtypes = [C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
OK = E.DF_VALIDATED | E.DF_WHITELISTED | E.DF_ACTIVE


def shape_a():
    """every node listed in a seeded order, its own endpoint each; 1 % demoted (inactive, no stamp); 1 % new rows, half of them
    on a listed node's endpoint"""
    rng = np.random.default_rng(1)
    n_new = max(W // 100, 1)
    status = np.full(W, E.NS_HEALTHY, dtype=np.uint8)
    ep = np.arange(W, dtype=np.uint32)
    rows = np.zeros(W + n_new, dtype=E.disc_row_dt)
    rows["row"][:W] = rows["endpoint"][:W] = rows["endpoint_after"][:W] = np.arange(W)
    rows["flags"] = OK
    demoted = rng.choice(W, size=n_new, replace=False)
    rows["flags"][demoted] = E.DF_VALIDATED | E.DF_WHITELISTED
    rows["row"][W:] = E.DISC_NEW
    rows["endpoint"][W:] = np.where(np.arange(n_new) % 2 == 0, W + np.arange(n_new), rng.choice(W, size=n_new))
    rows = rows[rng.permutation(len(rows))]
    return "(a) the usual pass", status, ep, W + n_new, 1, rows


def shape_b():
    status = np.full(W, E.NS_HEALTHY, dtype=np.uint8)
    ep = (np.arange(W) % 100).astype(np.uint32)
    rows = np.zeros(1000, dtype=E.disc_row_dt)
    rows["row"] = E.DISC_NEW
    rows["endpoint"] = np.arange(1000) % 100
    rows["flags"] = OK
    return "(b) 1,000 new rows on a table that shares 100 endpoints", status, ep, 100, W // 100 + 1, rows


def shape_c():
    """the table's first half Healthy on endpoint 0 and listed (every tenth demoted), as many new rows on endpoint 0 between
    them; the other half of the table unlisted on endpoints of its own"""
    rng = np.random.default_rng(3)
    half = W // 2
    status = np.full(W, E.NS_HEALTHY, dtype=np.uint8)
    ep = np.arange(W, dtype=np.uint32)
    ep[:half] = 0
    rows = np.zeros(2 * half, dtype=E.disc_row_dt)
    rows["row"][:half] = np.arange(half)
    rows["flags"] = OK
    rows["flags"][:half:10] = E.DF_VALIDATED | E.DF_WHITELISTED
    rows["row"][half:] = E.DISC_NEW
    rows = rows[rng.permutation(len(rows))]
    return "(c) the worst case: half the list Healthy on one endpoint, half new on the same", status, ep, W, half - half // 20, rows


def run(name, status, ep, n_ep, max_same, rows):
    D = len(rows)
    eng = E.Engine()
    one = np.ones(W, dtype=np.uint32)
    eng.upload_workers(dict(flags=np.where(status == E.NS_HEALTHY, E.W_HEALTHY, 0).astype(np.uint32) | 1, gpu_count=one, gpu_mem_mb=one,
                            gpu_model_class=0 * one, cpu_cores=one, ram_mb=one, storage_gb=one, lat=np.zeros(W), lon=np.zeros(W)))
    eng.liveness_enable(True, 3)
    idx = np.arange(W)
    ms = []
    for k in range(WARM + REPS):
        eng.liveness_set(idx, status)
        t0 = time.perf_counter()
        out, total = eng.discovery_sync(NOW, ep, n_ep, int(max_same), rows)
        dt = 1e3 * (time.perf_counter() - t0)
        if k >= WARM:
            ms.append(dt)
    fin = np.zeros(D, dtype=np.uint8)
    cnt = np.zeros(D, dtype=np.uint32)
    r = np.ascontiguousarray(rows)
    t0 = time.perf_counter()
    host_total = HOST.disc_host_pass(NOW, W, status.ctypes.data, ep.ctypes.data, int(max_same), r.ctypes.data, D, fin.ctypes.data, cnt.ctypes.data)
    host_ms = 1e3 * (time.perf_counter() - t0)
    assert host_total == total and np.array_equal(cnt, out["healthy_same_endpoint"]) and np.array_equal(fin, out["final_status"]), name
    new = rows["row"] == E.DISC_NEW
    say(f"{name}: W {W}, D {D} ({int(new.sum())} new), {n_ep} endpoint ids, max {int(max_same)}")
    say(f"    pm_discovery_sync apply=0: median {med(ms):.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}) of {REPS} after {WARM} warm-ups; "
        f"{total} updates, {int((out['ops'] & E.DO_ADMIT != 0).sum())} admitted, {int((out['ops'] & E.DO_SKIP != 0).sum())} skipped, "
        f"largest count {int(cnt.max())}")
    say(f"    bytes moved: host to device {D * 32 + W * 4:,} (rows, endpoint column), device to host {D * 16:,} (results)")
    say(f"    the sequential D x W loop, plain C++, one host thread, one run: {host_ms:.1f} ms ({host_ms / med(ms):.0f} x); "
        f"counts, final statuses and the number of updates equal the engine's")
    eng.close()


say("The discovery sync (pm_discovery.inc), one MI355X.  Written by tools/discovery_probe.py (tools/gpu_run.sh step `discovery`).")
say()
say("== host clock around pm_discovery_sync (the call ends in a stream synchronisation); no threshold was set for these times")
for shape in (shape_a, shape_b, shape_c):
    run(*shape())
say("(c): about 100,000 rows that each ask a segment of about 95,000 events; a decide thread walks a segment of more than 64 events")
say("with its wave, 64 events a step.  (c) was measured with that cooperative walk only: a thread walking alone would issue 64 times")
say("as many loads — whether (c) needs the walk to end inside the probe's time limit was not measured.")

if args.bench:
    bench_table(args.bench)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(LINES) + "\n")
