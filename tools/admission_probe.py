#!/usr/bin/env python3
"""The request gate's admission on one MI355X, timed on the host clock around each C ABI call (every call waits for its stream,
so the clock sees the whole of it, copies included): pm_admit_requests beside pm_verify_requests on the same batch of n = 1,000 /
10,000 requests, over standing nonce sets of 0 / 100,000 / 1,000,000 entries — what admission adds to the gate, which recovery
dominates, and how that grows with the standing set (one flag pass, one scan and one copy pass over it; never a sort) — and
pm_liveness_sweep_beats(NULL) beside pm_liveness_sweep at W = 100,000 (the first uploads nothing of size W).

The requests are 128 signatures by 128 signers the big-integer model made (tests/secp256k1_model.py), repeated to n with fresh
nonces: under a hundred a row, and the windows are put back before every call, so that every request reaches the nonce set and
is stored.  The standing set is filled the same way, 10,000 a call.  Warm-up calls first; medians with min and max.

Everything printed is also written to --out (default profiles/r33_admission.txt).  --bench DIR appends the comparison of
`bench.py --gpus 1` lines of the parent commit's build and of this one (bench_<k>_parent.json / bench_<k>_change.json, k = the
order they ran in); --bench-only skips the GPU part.
usage: python tools/admission_probe.py [n ...] [--sets N ...] [--book W] [--out FILE] [--bench DIR] [--bench-only] [--steps N]"""
import argparse
import glob
import hashlib
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("sizes", nargs="*", default=["1000", "10000"])
ap.add_argument("--sets", nargs="*", type=int, default=[0, 100000, 1000000])
ap.add_argument("--book", type=int, default=100000)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r33_admission.txt"))
ap.add_argument("--bench", default=None)
ap.add_argument("--bench-only", action="store_true")
ap.add_argument("--steps", type=int, default=7)
args = ap.parse_args()
LINES = []
WARM, STEPS = 2, args.steps
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
    say("   alternating in one GPU session; bench.py never calls admission.  Order: " + " ".join(r[0][0] for r in rows) +
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


def finish():
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a" if args.bench_only else "w") as f:  # (a table replaces the file; --bench-only adds to one)
        f.write("\n".join(LINES) + "\n")


if args.bench_only:
    bench_table(args.bench)
    finish()
    sys.exit(0)

sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import secp256k1_model as M  # noqa: E402
from protocol_amd import engine as E  # noqa: E402
from protocol_amd.addresses import make_addresses  # noqa: E402

ON = E.W_HEALTHY | E.W_HAS_P2P
SIGNERS = 128
FILL = 10000
NOW = 1_700_000_000_000


def cols(n):
    z = np.zeros(n, dtype=np.uint32)
    return dict(flags=np.full(n, ON, dtype=np.uint32), gpu_count=z, gpu_mem_mb=z, gpu_model_class=z, cpu_cores=z, ram_mb=z, storage_gb=z,
                price=z, lat=np.zeros(n), lon=np.zeros(n))


def clock(call):
    t0 = time.perf_counter()
    call()
    return 1e3 * (time.perf_counter() - t0)


def row(name, v, n):
    v = v[WARM:]
    say("    %-52s median %9.3f ms   min %9.3f   max %9.3f   %8.3f us a request   (%d calls)"
        % (name, med(v), min(v), max(v), 1e3 * med(v) / n, len(v)))
    return med(v)


keys = [int.from_bytes(hashlib.sha256(b"admission probe signer %d" % i).digest(), "big") % (M.N - 1) + 1 for i in range(SIGNERS)]
addr = [M.address_of_key(k) for k in keys]
pool = []
for k in range(SIGNERS):
    msg = b'/heartbeat{"address":"0x%s"}' % addr[k].hex().encode()
    pool.append((msg, M.sig65(*M.sign(keys[k], M.eip191(msg))), addr[k]))

W = args.book
eng = E.Engine(device=0)
eng.upload_workers(cols(W))
eng.enable_addresses(True)
book = make_addresses(3, W, "uniform")
where = np.linspace(0, W - 1, SIGNERS).astype(np.uint32)
for k, w in enumerate(where):
    book[w] = np.frombuffer(addr[k], dtype=np.uint8)
eng.set_addresses(0, book)
eng.liveness_enable(True)
ZERO64, ZERO32 = np.zeros(SIGNERS, dtype=np.uint64), np.zeros(SIGNERS, dtype=np.uint32)
serial = [0]


def batch(n):
    """n heartbeats, signer i % 128, every nonce new -> (pm_verify_requests' arrays, pm_admit_requests' arrays)"""
    msgs = [pool[i % SIGNERS][0] for i in range(n)]
    off = np.zeros(n + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
    sigs = np.frombuffer(b"".join(pool[i % SIGNERS][1] for i in range(n)), dtype=np.uint8).reshape(-1, 65)
    claimed = np.frombuffer(b"".join(pool[i % SIGNERS][2] for i in range(n)), dtype=np.uint8).reshape(-1, 20)
    gate = (np.frombuffer(b"".join(msgs), dtype=np.uint8), off, sigs, claimed, None)
    nonces = b"".join(b"probe-nonce-%012d" % (serial[0] + i) for i in range(n))  # 24 bytes each
    serial[0] += n
    noff = (24 * np.arange(n + 1)).astype(np.uint32)
    flags = np.full(n, E.RQ_FLAG_BEAT, dtype=np.uint8)
    ts = np.full(n, NOW // 1000, dtype=np.uint64)
    return gate, gate[:4] + (flags, ts, np.frombuffer(nonces, dtype=np.uint8), noff)


def admit(packed):
    eng.admission_rate_set(where, ZERO64, ZERO32)  # (not timed: the windows start over, every request reaches the nonce set)
    return clock(lambda: eng.admit_requests(packed, NOW))


say("== admission behind the request gate (MEASURED on one MI355X, host clock around each call; %d warm-up calls, then %d measured; the"
    % (WARM, STEPS))
say("   book holds %d rows, %d of them the signers'; every measured request is admitted and its nonce stored)" % (W, SIGNERS))
added = {}
for N in args.sets:
    eng.enable_admission(True)
    while eng.admission_nonces(NOW)[1] < N:
        _g, a = batch(min(FILL, N - eng.admission_nonces(NOW)[1]))
        admit(a)
    say("  standing set: %d nonces" % eng.admission_nonces(NOW)[1])
    for size in args.sizes:
        n = int(size)
        g, _a = batch(n)
        tv = [clock(lambda: eng.verify_requests(g)) for _ in range(WARM + STEPS)]
        ta = []
        for _ in range(WARM + STEPS):
            _g, a = batch(n)
            ta.append(admit(a))
        say("   n = %d" % n)
        b = row("pm_verify_requests", tv, n)
        c = row("pm_admit_requests", ta, n)
        added[(N, n)] = c - b
        say("      admission adds %.3f ms to the gate's %.3f ms; the set holds %d nonces now" % (c - b, b, eng.admission_nonces(NOW)[1]))
say("  what admission adds, by standing set (ms):")
for size in args.sizes:
    say("    n = %-6d " % int(size) + "   ".join("N = %d: %.3f" % (N, added[(N, int(size))]) for N in args.sets))

# the sweep from the device's column
eng.enable_admission(True)
rng = np.random.default_rng(4)
col = (NOW - rng.integers(0, 400_000, W)).astype(np.uint64)
eng.beats_set(np.arange(W, dtype=np.uint32), col)
a = [clock(lambda: eng.liveness_sweep(NOW, col)) for _ in range(WARM + STEPS)]
b = [clock(lambda: eng.liveness_sweep_beats(NOW)) for _ in range(WARM + STEPS)]
say("  the sweep at W = %d (apply = 0):" % W)
row("pm_liveness_sweep (uploads W x 8 bytes)", a, W)
row("pm_liveness_sweep_beats(NULL)", b, W)
eng.close()
if args.bench:
    bench_table(args.bench)
finish()
