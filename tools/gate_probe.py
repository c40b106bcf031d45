#!/usr/bin/env python3
"""The request gate on one MI355X, timed on the host clock around each C ABI call (every call waits for its stream, so the clock
sees the whole of it, copies included): pm_ecrecover_many and pm_verify_requests at n = 1,000 / 10,000 / 100,000 over an address
book of 100,000 rows, the address index cold (a row rewritten before the call: the index is sorted again) and warm; beside them
pm_host_ecrecover on one host thread — this project's plain C++ (pm_host.cpp), NOT k256: nobody has measured what the reference
pays per beat.  The signatures are 64 the big-integer model made (tests/secp256k1_model.py), repeated to n: a lane's work does not
depend on its neighbour's.  Warm-up calls first; medians with min and max.

Everything printed is also written to --out (default profiles/r32_request_gate.txt).  --bench DIR appends the comparison of
`bench.py --gpus 1` lines of the parent commit's build and of this one (bench_<k>_parent.json / bench_<k>_change.json, k = the
order they ran in); --bench-only skips the GPU part.
usage: python tools/gate_probe.py [n ...] [--book W] [--out FILE] [--bench DIR] [--bench-only] [--steps N]"""
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
ap.add_argument("sizes", nargs="*", default=["1000", "10000", "100000"])
ap.add_argument("--book", type=int, default=100000)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r32_request_gate.txt"))
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
    say("   alternating in one GPU session; bench.py never calls the gate.  Order: " + " ".join(r[0][0] for r in rows) +
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
POOL = 64


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


# 64 requests by 8 signers, as the middleware sees a heartbeat: path + JSON of about 100 bytes
keys = [int.from_bytes(hashlib.sha256(b"probe signer %d" % i).digest(), "big") % (M.N - 1) + 1 for i in range(8)]
addr = [M.address_of_key(k) for k in keys]
pool = []
for i in range(POOL):
    k = i % len(keys)
    msg = b'/heartbeat{"address":"0x%s","nonce":"probe-nonce-%07d"}' % (addr[k].hex().encode(), i)
    h = M.eip191(msg)
    pool.append((msg, h, M.sig65(*M.sign(keys[k], h)), addr[k]))

W = args.book
eng = E.Engine(device=0)
eng.upload_workers(cols(W))
eng.enable_addresses(True)
book = make_addresses(3, W, "uniform")
where = np.linspace(0, W - 1, len(keys)).astype(np.int64)
for k, w in enumerate(where):
    book[w] = np.frombuffer(addr[k], dtype=np.uint8)
eng.set_addresses(0, book)
eng.liveness_enable(True)

say("== the request gate (MEASURED on one MI355X, host clock around each call; %d warm-up calls, then %d measured; the book holds %d rows)"
    % (WARM, STEPS, W))
host_n = 200
hs = [clock(lambda i=i: E.host_ecrecover(pool[i % POOL][1], pool[i % POOL][2])) for i in range(host_n)]
say("  pm_host_ecrecover, one host thread, %d recoveries: median %.3f ms each (this project's plain C++, not k256; the reference is unmeasured)"
    % (host_n, med(hs)))
for size in args.sizes:
    n = int(size)
    say("  n = %d" % n)
    reps = (n + POOL - 1) // POOL
    hashes = np.frombuffer(b"".join(p[1] for p in pool) * reps, dtype=np.uint8).reshape(-1, 32)[:n]
    sigs = np.frombuffer(b"".join(p[2] for p in pool) * reps, dtype=np.uint8).reshape(-1, 65)[:n]
    t = [clock(lambda: eng.ecrecover_many(hashes, sigs)) for _ in range(WARM + STEPS)]
    a = row("pm_ecrecover_many", t, n)
    say("      against the host thread: %.1f recoveries in the time of one" % (med(hs) / (a / n)))
    ok, got = eng.ecrecover_many(hashes, sigs)
    say("      every address is the signer's: %s" % bool(ok.all() and all(got[i].tobytes() == pool[i % POOL][3] for i in range(0, n, max(n // 97, 1)))))
    msgs = [pool[i % POOL][0] for i in range(n)]
    off = np.zeros(n + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
    packed = (np.frombuffer(b"".join(msgs), dtype=np.uint8), off, np.ascontiguousarray(sigs),
              np.frombuffer(b"".join(pool[i % POOL][3] for i in range(n)), dtype=np.uint8).reshape(-1, 20), None)
    warm = [clock(lambda: eng.verify_requests(packed)) for _ in range(WARM + STEPS)]
    cold = []
    for _ in range(WARM + STEPS):
        eng.set_addresses(1, book[1:2])   # the same bytes again: the book's epoch moves, the index is built again
        cold.append(clock(lambda: eng.verify_requests(packed)))
    b = row("pm_verify_requests, the index warm", warm, n)
    c = row("pm_verify_requests, the index cold", cold, n)
    say("      the index of %d rows costs %.3f ms" % (W, c - b))
    v, counts = eng.verify_requests(packed)
    say("      every request is OK at its signer's row: %s   census %s"
        % (bool((v["code"] == E.RQ_OK).all() and all(int(v["row"][i]) == int(where[(i % POOL) % len(keys)]) for i in range(0, n, max(n // 97, 1)))),
           counts.tolist()))
eng.close()
say()
say("  (no window or table for G was tried: the ladder is the plain interleaved double-and-add over {G, R, G + R})")
if args.bench:
    bench_table(args.bench)
finish()
