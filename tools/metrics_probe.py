#!/usr/bin/env python3
"""The metrics ledger on the host's clock at W worker rows (default 100,000) with E series a row (default 8): an ingest of W
REPLACE beats x E entries onto a ledger of the same size, the totals cold (right behind an ingest) and cached, and the full
listing with its join.  Median, min and max of REPS calls after WARM warm-ups, and beside each one run of the same call as plain
C++ on one host thread (tools/metrics_host_loop.cpp: an unordered_map per node; it flatters the reference, which pays a Redis
round trip per field), whose totals must equal the engine's.  The ratio is reported, not asserted.

Everything printed is also written to --out (default profiles/r20_metrics.txt).  --bench DIR appends the comparison of
`python bench.py --gpus 1 --steps 21 --warmup 3` on the parent commit's build and on this one (bench_<k>_parent.json /
bench_<k>_change.json, k = the order they ran in); --bench-only skips the GPU part.
usage: python tools/metrics_probe.py [W] [E] [--out FILE] [--bench DIR] [--bench-only]"""
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
ap.add_argument("E", nargs="?", type=int, default=8)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_metrics.txt"))
ap.add_argument("--bench", default=None)
ap.add_argument("--bench-only", action="store_true")
args = ap.parse_args()
W, NE = args.W, args.E
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
    say("== the feature unused: `python bench.py --gpus 1 --steps 21 --warmup 3` on the parent commit's build and on this one, alternating")
    say("   in one GPU session; bench.py never calls pm_metrics_*.  Order: " + " ".join(r[0][0] for r in rows) + " (p = parent, c = this commit)")
    for j, name in ((1, "ms_per_step"), (2, "churn.ms_per_tick")):
        say("  " + name)
        lo, hi = (f(r[j] for r in rows if r[0] == "parent") for f in (min, max))
        for w in ("parent", "change"):
            v = [r[j] for r in rows if r[0] == w]
            say("    %s  %s   median %.4f   min %.4f   max %.4f" % (w, " ".join("%.4f" % x for x in v), med(v), min(v), max(v)))
        m = med([r[j] for r in rows if r[0] == "change"])
        say("    the parent's spread is [%.4f, %.4f]: this commit's median %.4f lies %s" % (lo, hi, m, "inside" if lo <= m <= hi else "BELOW" if m < lo else "ABOVE"))


if args.bench_only:
    bench_table(args.bench)
    with open(args.out, "a") as f:
        f.write("\n".join(LINES) + "\n")
    sys.exit(0)

sys.path.insert(0, ROOT)
from protocol_amd import engine as E  # noqa: E402

so = os.path.join(tempfile.mkdtemp(), "libmx_host.so")
subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                       os.path.join(ROOT, "tools", "metrics_host_loop.cpp"), "-o", so])
H = C.CDLL(so)
vp, u32 = C.c_void_p, C.c_uint32
H.mx_host_reset.argtypes = [u32]
H.mx_host_ingest.argtypes = [vp, u32, vp]
H.mx_host_totals.argtypes = [vp, vp, u32]
H.mx_host_rows.argtypes = [vp, vp, vp, vp]
H.mx_host_rows.restype = u32

rng = np.random.default_rng(20)
S = 4 * NE                                  # series in use: every row holds NE of them
z = np.zeros(W, dtype=np.uint32)
eng = E.Engine()
eng.upload_workers(dict(flags=np.full(W, E.W_HEALTHY | E.W_HAS_P2P, dtype=np.uint32), gpu_count=z, gpu_mem_mb=z, gpu_model_class=z,
                        cpu_cores=z, ram_mb=z, storage_gb=z, price=z, lat=np.zeros(W), lon=np.zeros(W)))
eng.metrics_enable(True)


def batch():
    """W REPLACE beats in row order, NE distinct series each (a sliding window, so about three in four survive a beat)"""
    beats = np.zeros(W, dtype=E.mx_beat_dt)
    beats["row"] = np.arange(W)
    beats["kind"] = E.MXB_REPLACE
    beats["first"] = np.arange(W, dtype=np.uint32) * NE
    beats["n"] = NE
    ent = np.zeros(W * NE, dtype=E.mx_entry_dt)
    start = rng.integers(0, S, size=W)
    ent["series"] = ((start[:, None] + np.arange(NE)[None, :]) % S).reshape(-1)
    ent["flags"] = (ent["series"] % 4 == 0).astype(np.uint32)
    ent["value"] = rng.normal(size=W * NE) * 100.0
    return beats, ent


def timed(call, reps=REPS, warm=WARM, before=None):
    out = []
    for k in range(warm + reps):
        if before:
            before()
        t0 = time.perf_counter()
        call()
        dt = (time.perf_counter() - t0) * 1e3
        if k >= warm:
            out.append(dt)
    return out


def line(name, gpu, host_ms, note=""):
    say("  %-34s engine median %8.3f ms  min %8.3f  max %8.3f   host loop %9.3f ms   ratio %6.1fx  %s"
        % (name, med(gpu), min(gpu), max(gpu), host_ms, host_ms / med(gpu), note))


say("== metrics ledger at W = %d worker rows, %d series a row (%d entries), %d series in use; %d calls after %d warm-ups"
    % (W, NE, W * NE, S, REPS, WARM))
batches = [batch() for _ in range(WARM + REPS + 2)]
eng.metrics_ingest(batches[-1][0], batches[-1][1], S)              # the standing ledger
H.mx_host_reset(W)
H.mx_host_ingest(batches[-1][0].ctypes.data, W, batches[-1][1].ctypes.data)
it = iter(batches)


def one_ingest():
    b, e = next(it)
    eng.metrics_ingest(b, e, S)


t_ing = timed(one_ingest)
t0 = time.perf_counter()
for b, e in batches[:WARM + REPS]:
    H.mx_host_ingest(b.ctypes.data, W, e.ctypes.data)
host_ing = (time.perf_counter() - t0) * 1e3 / (WARM + REPS)
line("ingest, %d REPLACE beats x %d" % (W, NE), t_ing, host_ing, "(%.1f MB in)" % ((W * 16 + W * NE * 16) / 1e6))

# the totals: cold = the first call behind an ingest (a one-row ingest in front of every call), cached = the second
touch_b = np.array([(0, E.MXB_MERGE, 0, 1)], dtype=E.mx_beat_dt)


def touch():
    eng.metrics_ingest(touch_b, np.array([(0, 0, float(rng.normal()))], dtype=E.mx_entry_dt), S)


t_touch = timed(touch)
t_cold = timed(eng.metrics_totals, before=touch)
t_hot = timed(eng.metrics_totals)
hs, hc = np.zeros(S), np.zeros(S, dtype=np.uint32)
t0 = time.perf_counter()
H.mx_host_totals(hs.ctypes.data, hc.ctypes.data, S)
host_tot = (time.perf_counter() - t0) * 1e3
line("totals, cold (%d entries)" % (W * NE), t_cold, host_tot)
line("totals, cached", t_hot, host_tot)
say("  (a one-row ingest, which copies the other rows: median %.3f ms)" % med(t_touch))
# the host loop holds the same ledger but for row 0's touched value: counts equal, sums equal to rounding (its order is the map's)
gs, gc = eng.metrics_totals()
assert gc.tolist() == hc.tolist(), "counts differ from the host loop's"
assert np.allclose(gs, hs, rtol=1e-9, atol=1e3), "sums differ from the host loop's"

rows = eng.metrics_rows()
t_rows = timed(eng.metrics_rows, reps=5, warm=1)
out = np.zeros(len(rows), dtype=E.mx_row_dt)
gof, gid, gcfg = np.full(W, -1, dtype=np.int32), np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint32)
t0 = time.perf_counter()
n = H.mx_host_rows(gof.ctypes.data, gid.ctypes.data, gcfg.ctypes.data, out.ctypes.data)
host_rows = (time.perf_counter() - t0) * 1e3
assert n == len(rows)
line("full listing (%d rows of 32 B)" % len(rows), t_rows, host_rows, "(%.1f MB out; includes the numpy buffer)" % (len(rows) * 32 / 1e6))
eng.close()

if args.bench:
    bench_table(args.bench)
with open(args.out, "w") as f:
    f.write("\n".join(LINES) + "\n")
