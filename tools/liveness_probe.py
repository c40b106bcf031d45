#!/usr/bin/env python3
"""pm_liveness_sweep on the host's clock at W worker rows (default 100,000) with 1 % of the rows silent: the median of 50
sweeps after 5 warm-ups, reporting (apply = 0) and applying (apply = 1) on a carved swarm, and the bytes a sweep moves.

Every timed sweep meets the same state: between two sweeps the silent rows are put back to Healthy with pm_liveness_set (and,
for the applying engine, their flags with pm_on_worker_status_many), outside the timing.  With the default threshold (3) a
silent Healthy row turns Unhealthy: 1 % of the rows are listed and no group dissolves.  A last section times the sweep in
which those rows die (threshold 1, their second silent interval): every death dissolves a group.

Everything printed is also written to --out (default profiles/r18_liveness.txt).  --bench DIR appends the liveness-off
comparison: DIR holds the result lines of `python bench.py --gpus 1 --steps 21 --warmup 3` run on the parent commit's build and
on this one, alternating in one GPU session, as bench_<k>_parent.json / bench_<k>_change.json (k = the order they ran in;
other files there are ignored).  --bench-only skips the sweep (no GPU needed) and APPENDS the comparison of a further session.
usage: python tools/liveness_probe.py [W] [--out FILE] [--bench DIR] [--bench-only]"""
import argparse
import glob
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("W", nargs="?", type=int, default=100_000)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_liveness.txt"))
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
                     j["churn"]["split_ms_p50"], j["churn"]["groups"]))
    say()
    say("== liveness off: `python bench.py --gpus 1 --steps 21 --warmup 3` on the parent commit's build and on this one, alternating in")
    say("   one GPU session; bench.py never calls a liveness function.  Order: " + " ".join(r[0][0] for r in rows) + " (p = parent, c = this commit)")
    for j, name in ((1, "ms_per_step"), (2, "churn.ms_per_tick")):
        say("  " + name)
        lo, hi = (f(r[j] for r in rows if r[0] == "parent") for f in (min, max))
        for w in ("parent", "change"):
            v = [r[j] for r in rows if r[0] == w]
            say("    %s  %s   median %.4f   min %.4f   max %.4f" % (w, " ".join("%.4f" % x for x in v), med(v), min(v), max(v)))
        inside = [lo <= r[j] <= hi for r in rows if r[0] == "change"]
        say("    the parent's spread is [%.4f, %.4f]: %d of %d of this commit's values lie inside" % (lo, hi, sum(inside), len(inside)))
    say("  churn phases (p50 of a run's six ticks), median over the runs")
    for w in ("parent", "change"):
        say("    " + w + "  " + "  ".join("%s %.4f" % (k[:-3], med([r[3][k] for r in rows if r[0] == w])) for k in rows[0][3] if k != "publish_ms"))
    say("  groups " + str(sorted({r[4] for r in rows})))
    others = len(glob.glob(os.path.join(d, "bench_*.json"))) - len(files)
    if others:
        say("  (%d runs of other builds stood between these in the same session and are left out)" % others)



if args.bench_only:
    bench_table(args.bench)
    with open(args.out, "a") as f:
        f.write("\n".join(LINES) + "\n")
    sys.exit(0)

sys.path.insert(0, ROOT)
from protocol_amd import engine as E, host
from protocol_amd.swarm import make_swarm

sw = make_swarm(1, max(W // 10, 1), W)
packed = host.pack_workers(sw)
flags = packed["flags"].astype(np.uint32)
healthy = np.nonzero(flags & E.W_HEALTHY)[0]
rng = np.random.default_rng(1)
silent = np.sort(rng.choice(healthy, size=max(W // 100, 1), replace=False))
beats = np.full(W, NOW - 1000, dtype=np.uint64)
beats[silent] = 0
pool = np.full((W + 63) // 64, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)


def engine(m):
    eng = E.Engine()
    host.load_swarm(eng, sw)
    eng.tick()
    eng.liveness_enable(True, m)
    # (rows that are not Healthy start Discovered: one sweep with every one of them beating settles them, so that the timed
    # sweeps list the silent rows only)
    n, _ = eng.liveness_sweep(NOW, np.full(W, NOW, dtype=np.uint64), None, apply=True)
    eng.tick()
    return eng, n


def restore(eng, apply):
    eng.liveness_set(silent, np.full(len(silent), E.NS_HEALTHY, dtype=np.uint8))
    if apply:
        eng.on_worker_status_many(silent, flags[silent] | np.uint32(E.W_HEALTHY))


def timed(eng, apply, with_pool):
    ms, n_last = [], 0
    for k in range(WARM + REPS):
        t0 = time.perf_counter()
        n_last, census = eng.liveness_sweep(NOW + k, beats, pool if with_pool else None, apply=apply)
        dt = 1e3 * (time.perf_counter() - t0)
        assert n_last == len(silent) and int(census.sum()) == W
        if k >= WARM:
            ms.append(dt)
        restore(eng, apply)
    return med(ms), min(ms), max(ms), n_last


say("The liveness sweep (pm_liveness.inc), one MI355X.  Written by tools/liveness_probe.py (tools/gpu_run.sh step `liveness`).")
say()
say("== the sweep: host clock around pm_liveness_sweep (the call ends in a stream synchronisation), BASELINE configs[1]'s swarm")
say("   after a tick, 1 % of the Healthy rows silent")
eng, settled = engine(3)
say(f"W {W}, {len(healthy)} Healthy rows, {len(silent)} silent (1 %), {settled} rows settled by the first sweep; "
      f"groups {len(eng.get_groups()[1])}")
for apply in (False, True):
    for with_pool in (False, True):
        m, lo, hi, n = timed(eng, apply, with_pool)
        say(f"pm_liveness_sweep apply={int(apply)} in_pool_bits={'given' if with_pool else 'NULL'}: median {m:.3f} ms "
              f"(min {lo:.3f}, max {hi:.3f}) of {REPS} after {WARM} warm-ups, {n} rows listed")
t0 = time.perf_counter()
rows = eng.liveness_transitions()
say(f"pm_liveness_transitions (size query + copy-out) of {len(rows)} rows: {1e3 * (time.perf_counter() - t0):.3f} ms")
words = (W + 63) // 64
n = len(silent)
say(f"bytes per sweep at W {W}, {n} listed: host to device {W * 8:,} (beat column) + {words * 8:,} (pool bits, when given); "
      f"sweep kernel reads {W * 13 + words * 8:,} (beat, status, counter, pool words) and writes about {n * 6 + words * 8:,} "
      f"(changed statuses and counters, old-status bytes, the bitmap); scan and expansion read {words * 12 + n * 6:,} and write "
      f"{words * 4 + n * 12:,}; device to host 36 (count, census) + {n * 12:,} (the rows: apply, or pm_liveness_transitions)")
eng.close()

# the sweep in which the silent rows die: threshold 1, their second silent interval
eng, _ = engine(1)
ms, dissolved = [], []
for k in range(5):
    eng.liveness_sweep(NOW + 10 * k, beats, None, apply=True)                # Healthy -> Unhealthy
    before = len(eng.get_groups()[1])
    t0 = time.perf_counter()
    n, _ = eng.liveness_sweep(NOW + 10 * k + 1, beats, None, apply=True)     # Unhealthy -> Dead: the groups dissolve
    ms.append(1e3 * (time.perf_counter() - t0))
    dissolved.append(before - len(eng.get_groups()[1]))
    assert n == len(silent)
    restore(eng, True)
    eng.tick()
say(f"pm_liveness_sweep apply=1, {len(silent)} deaths dissolving {int(med(dissolved))} groups: median {med(ms):.3f} ms of 5")
eng.close()


if args.bench:
    bench_table(args.bench)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(LINES) + "\n")
