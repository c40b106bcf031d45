#!/usr/bin/env python3
"""The address book on one MI355X, timed on the host clock around each C ABI call (every call waits for its stream, so the clock
sees the whole of it): at W = 10,000 / 100,000 / 1,000,000 rows with 1 % appended a step — pm_addresses_set of the new rows,
pm_addresses_rank on uniform addresses (the one-word sort) and on a shared-prefix swarm (the all-words sort), pm_addresses_text of
a page of 100 rows, pm_invite_digests of 1,000 and 10,000 rows.  Beside the set + rank pair, what the plugin does today
(tools/address_host_loop.cpp): an EIP-55 text per new address, an insert into the sorted text vector, the ranks of all W rows
rebuilt, the whole column through pm_set_addr_ranks.  Warm-up steps first; medians with min and max.

Everything printed is also written to --out (default profiles/r30_address_book.txt).  --bench DIR appends the comparison of
`bench.py --gpus 1` lines of the parent commit's build and of this one (bench_<k>_parent.json / bench_<k>_change.json, k = the
order they ran in); --bench-only skips the GPU part.
usage: python tools/address_probe.py [W ...] [--out FILE] [--bench DIR] [--bench-only] [--steps N]"""
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
ap.add_argument("sizes", nargs="*", default=["10000", "100000", "1000000"])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30_address_book.txt"))
ap.add_argument("--bench", default=None)
ap.add_argument("--bench-only", action="store_true")
ap.add_argument("--steps", type=int, default=8)
args = ap.parse_args()
LINES = []
WARM, STEPS = 3, args.steps
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
    say("   alternating in one GPU session; bench.py never enables the address book.  Order: " + " ".join(r[0][0] for r in rows) +
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
from protocol_amd import build as B  # noqa: E402
from protocol_amd import engine as E  # noqa: E402
from protocol_amd.addresses import make_addresses  # noqa: E402

E.lib()
so = os.path.join(tempfile.mkdtemp(), "libaddr_host.so")
subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                       os.path.join(ROOT, "tools", "address_host_loop.cpp"), "-L", os.path.dirname(B.LIB_PATH), "-lpm_engine",
                       "-Wl,-rpath," + os.path.dirname(B.LIB_PATH), "-o", so])
H = C.CDLL(so)
vp, u32 = C.c_void_p, C.c_uint32
H.addr_host_append.argtypes = [vp, vp, u32]
H.addr_host_load.argtypes = [vp, vp, u32]
H.addr_host_ranks.restype = C.POINTER(u32)
ON = E.W_HEALTHY | E.W_HAS_P2P


def cols(n):
    z = np.zeros(n, dtype=np.uint32)
    return dict(flags=np.full(n, ON, dtype=np.uint32), gpu_count=z, gpu_mem_mb=z, gpu_model_class=z, cpu_cores=z, ram_mb=z, storage_gb=z,
                price=z, lat=np.zeros(n), lon=np.zeros(n))


def clock(call):
    t0 = time.perf_counter()
    call()
    return 1e3 * (time.perf_counter() - t0)


def row(name, v):
    v = v[WARM:]
    say("    %-58s median %9.4f ms   min %9.4f   max %9.4f   (%d steps)" % (name, med(v), min(v), max(v), len(v)))
    return med(v)


def churn(W, variant):
    """W rows loaded, then STEPS + WARM steps of W / 100 appended rows: the device path and the host loop, each on its own engine"""
    step = max(W // 100, 1)
    total = W + (WARM + STEPS) * step
    addrs = make_addresses(7, total, variant)
    dev, hst = E.Engine(device=0), E.Engine(device=0)
    for eng in (dev, hst):
        eng.upload_workers(cols(W))
    dev.enable_addresses(True)
    t_load_dev = clock(lambda: (dev.set_addresses(0, addrs[:W]), dev.rank_addresses(want=False)))
    first = np.ascontiguousarray(addrs[:W])
    t_load_host = clock(lambda: E.check(H.addr_host_load(hst._h, first.ctypes.data, W)))
    say("  %s addresses, W = %d, %d appended a step" % (variant, W, step))
    say("    the first load (set + rank of W rows | texts, one sort, the column):   device %.3f ms   host %.3f ms" % (t_load_dev, t_load_host))
    t_set, t_rank, t_host = [], [], []
    for s in range(WARM + STEPS):
        lo = W + s * step
        new = np.ascontiguousarray(addrs[lo:lo + step])
        dev.append_workers(cols(step))
        hst.append_workers(cols(step))
        t_set.append(clock(lambda: dev.set_addresses(lo, new)))
        t_rank.append(clock(lambda: dev.rank_addresses(want=False)))
        t_host.append(clock(lambda: E.check(H.addr_host_append(hst._h, new.ctypes.data, step))))
    sorts = dev.debug_address_sorts()
    a = row("pm_addresses_set of the new rows", t_set)
    b = row("pm_addresses_rank (%s)" % ("one-word sort" if not sorts["deep"] else "all-words sort" if not sorts["shallow"] else "BOTH PATHS"), t_rank)
    c = row("host loop: EIP-55 + sorted insert + re-rank + pm_set_addr_ranks", t_host)
    say("    set + rank %.4f ms against the host loop's %.4f ms: %.2fx" % (a + b, c, c / (a + b)))
    got = dev.rank_addresses()
    want = np.ctypeslib.as_array(H.addr_host_ranks(), shape=(total,))
    say("    the two paths' ranks agree: %s" % bool(np.array_equal(got, want)))
    hst.close()
    return dev, total


say("== the address book (MEASURED on one MI355X, host clock around each call; %d warm-up steps, then %d measured)" % (WARM, STEPS))
for size in args.sizes:
    W = int(size)
    dev, total = churn(W, "uniform")
    page = np.arange(total // 2, total // 2 + 100, dtype=np.uint32)
    row("pm_addresses_text of a page of 100 rows", [clock(lambda: dev.address_texts(page)) for _ in range(WARM + STEPS)])
    rng = np.random.default_rng(1)
    for n in (1000, 10000):
        rows = rng.integers(0, total, size=n).astype(np.uint32)
        nonces = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        exp = np.full(n, 1_760_000_000, dtype=np.uint64)
        row("pm_invite_digests of %d rows" % n, [clock(lambda: dev.invite_digests(1, 2, rows, nonces, exp)) for _ in range(WARM + STEPS)])
    dev.close()
    dev, _ = churn(W, "prefix20")
    dev.close()
    say()
if args.bench:
    bench_table(args.bench)
finish()
