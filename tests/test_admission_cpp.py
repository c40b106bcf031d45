"""The request gate's admission without a GPU: GpuMatchPlugin::enable_admission / admit_requests with their C face, and
sweep_statuses' switch to pm_liveness_sweep_beats, against a mock (tests/cpp/admission_test.cpp + tests/cpp/mock_admission.cpp, a
stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer; the signatures come from the big-integer model,
written to a file the program reads), and the new names agreeing across the header, protocol_amd.engine, the Rust twin's extern
block and both libraries' dynamic symbol tables."""
import hashlib
import os
import re
import shutil
import subprocess

import pytest

import secp256k1_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = [os.path.join(ROOT, "include"), os.path.join(ROOT, "protocol_amd", "plugin"), os.path.join(ROOT, "protocol_amd", "csrc")]
PLUGIN = os.path.join(ROOT, "protocol_amd", "plugin")
SRC = [os.path.join(ROOT, "tests", "cpp", f) for f in ("admission_test.cpp", "mock_admission.cpp", "mock_gate.cpp", "mock_addresses.cpp",
                                                       "mock_directory.cpp", "mock_liveness.cpp", "mock_engine.cpp")] + \
      [os.path.join(PLUGIN, f) for f in ("gpu_match_plugin.cpp", "gpu_match_addresses.cpp", "gpu_match_directory.cpp", "gpu_match_gate.cpp",
                                         "gpu_match_liveness.cpp", "gpu_match_admission.cpp", "pm_plugin_c.cpp", "pm_plugin_addresses_c.cpp",
                                         "pm_plugin_gate_c.cpp", "pm_plugin_admission_c.cpp")] + \
      [os.path.join(ROOT, "protocol_amd", "csrc", "pm_host.cpp")]
ENGINE = {"pm_admission_enable": 2, "pm_admit_requests": 13, "pm_admission_rate_get": 5, "pm_admission_rate_set": 5,
          "pm_admission_nonces": 4, "pm_beats_get": 4, "pm_beats_set": 4, "pm_liveness_sweep_beats": 7}
SHIM = ("pm_admission_enable", "pm_admit_requests", "pm_liveness_sweep_beats")  # what the plugin twins call


def _case_file(path):
    keys = [int.from_bytes(hashlib.sha256(b"admission cpp signer %d" % i).digest(), "big") % (M.N - 1) + 1 for i in range(4)]
    with open(path, "w") as f:
        for k, key in enumerate(keys):
            addr = M.address_of_key(key)
            for m in range(12):
                msg = b'/heartbeat{"n":%d}' % m
                f.write(f"signed {k} {addr.hex()} {M.sig65(*M.sign(key, M.eip191(msg))).hex()} {msg.decode()}\n")


def test_the_admission_twin_against_the_mock_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe, cases = str(tmp_path / "admission_test"), str(tmp_path / "cases.txt")
    _case_file(cases)
    base = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *[f"-I{d}" for d in INC], *SRC, "-lpthread", "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    r = subprocess.run(base[:1] + san + base[1:], capture_output=True, text=True)
    if r.returncode != 0:  # (a toolchain without the sanitizer runtimes: the plain build still runs every check)
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    out = subprocess.run([exe, cases], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "4 tests, 0 failed checks" in out.stdout, out.stdout + out.stderr[-4000:]


def _arity(args: str) -> int:
    return len([a for a in args.split(",") if a.strip()])


def test_the_new_names_agree_everywhere():
    from protocol_amd import build as B
    from protocol_amd import engine as E
    hdr = open(os.path.join(ROOT, "include", "pm_engine.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    rs = open(os.path.join(ROOT, "rust", "gpu_match_plugin.rs")).read()
    ext = rs[rs.index('extern "C" {'):rs.index("\n}\n", rs.index('extern "C" {'))]
    body = rs[rs.index("\n}\n", rs.index('extern "C" {')):]
    eng = subprocess.run(["nm", "-D", B.build()], capture_output=True, text=True, check=True).stdout
    plug = subprocess.run(["nm", "-D", "-C", B.build_plugin()], capture_output=True, text=True, check=True).stdout
    for name, arity in ENGINE.items():
        h = re.search(r"int32_t " + name + r"\(([^;]*)\);", plain)
        assert h and _arity(h.group(1)) == arity, name
        assert name in E.EXPORTS
        assert re.search(r"\bT " + name + r"\b", eng), f"libpm_engine.so does not define {name}"
    for name in SHIM:
        r = re.search(r"fn " + name + r"\(([^;]*)\) -> i32;", ext)
        assert r and _arity(r.group(1)) == ENGINE[name], name
        assert re.search(r"\b" + name + r"\b", body), f"the Rust plugin body does not use {name}"
        assert re.search(r"\bU " + name + r"\b", plug), f"libpm_plugin.so does not import {name}"
    pmx = open(os.path.join(PLUGIN, "pm_plugin_c.h")).read()
    for name in ("pmx_enable_admission", "pmx_admit_requests"):
        assert re.search(r"int32_t " + name + r"\(", pmx) and re.search(r"\bT " + name + r"\b", plug), name
    hpp = open(os.path.join(PLUGIN, "gpu_match_plugin.hpp")).read()
    for name in ("enable_admission", "admit_requests"):
        assert re.search(r"pub fn " + name + r"\(", body), f"the Rust twin has no {name}"
        assert re.search(r"\b" + name + r"\(", hpp), f"the C++ twin has no {name}"
    # the codes and flags are the header's on every side
    for name, val in (("RATE_LIMITED", 8), ("EXPIRED", 9), ("BAD_NONCE", 10), ("REPLAY", 11), ("NO_NONCE", 12)):
        assert re.search(r"PM_RQ_%s = %d\b" % (name, val), plain) and getattr(E, "RQ_" + name) == val
        assert re.search(r"pub const RQ_%s: u32 = %d;" % (name, val), rs), name
    assert re.search(r"PM_AD_N_CODES = 13\b", plain) and E.AD_N_CODES == 13 and re.search(r"pub const AD_N_CODES: usize = 13;", rs)
    for name, val in (("NO_TIMESTAMP", 2), ("NO_NONCE", 4), ("BEAT", 8)):
        assert re.search(r"#define PM_RQ_FLAG_%s %du\b" % (name, val), hdr) and getattr(E, "RQ_FLAG_" + name) == val
        assert re.search(r"pub const RQ_FLAG_%s: u8 = %d;" % (name, val), rs), name
    # the plugin's older files stay linkable against mocks without the new exports
    for f in ("gpu_match_plugin.cpp", "pm_plugin_c.cpp", "gpu_match_liveness.cpp", "gpu_match_gate.cpp"):
        assert not re.search(r"\bpm_(admi\w+|beats_\w+|liveness_sweep_beats)\s*\(", open(os.path.join(PLUGIN, f)).read()), f
    assert {"gpu_match_admission.cpp", "pm_plugin_admission_c.cpp"} <= set(B.PLUGIN_SOURCES)
    assert {"pm_admission.inc", "pm_engine_admission.inc"} <= set(B.HEADERS)
    assert re.search(r"#define PM_ABI_VERSION 3\b", hdr)
    kernels = open(os.path.join(B.CSRC, "pm_kernels.hip")).read()
    assert kernels.index('"pm_secp256k1.inc"') < kernels.index('"pm_admission.inc"') < kernels.index('"pm_launch.inc"')
    # the debug header's hook is a macro over pm_admission_enable, not a call of its own
    dbg = open(os.path.join(ROOT, "include", "pm_engine_debug.h")).read()
    assert re.search(r"#define PM_AD_DEBUG_PREFIX_BITS\(k\) \(1u \| \(\(uint32_t\)\(k\) << 8\)\)", dbg) and E.ad_debug_prefix_bits(4) == 1 | 4 << 8
