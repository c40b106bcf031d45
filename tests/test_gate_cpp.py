"""The request gate without a GPU: pm_host_ecrecover on the named cases, and GpuMatchPlugin::verify_requests with its C face
against a mock (tests/cpp/gate_test.cpp + tests/cpp/mock_gate.cpp, a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer; the cases and the signatures come from the big-integer model, written to a file the program reads),
and the new names agreeing across the header, protocol_amd.engine, the Rust twin's extern block and both libraries' dynamic
symbol tables."""
import hashlib
import os
import re
import shutil
import subprocess

import pytest

import gate_cases as GC
import secp256k1_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = [os.path.join(ROOT, "include"), os.path.join(ROOT, "protocol_amd", "plugin"), os.path.join(ROOT, "protocol_amd", "csrc")]
PLUGIN = os.path.join(ROOT, "protocol_amd", "plugin")
SRC = [os.path.join(ROOT, "tests", "cpp", f) for f in ("gate_test.cpp", "mock_gate.cpp", "mock_addresses.cpp", "mock_directory.cpp",
                                                       "mock_engine.cpp")] + \
      [os.path.join(PLUGIN, f) for f in ("gpu_match_plugin.cpp", "gpu_match_addresses.cpp", "gpu_match_directory.cpp", "gpu_match_gate.cpp",
                                         "pm_plugin_c.cpp", "pm_plugin_addresses_c.cpp", "pm_plugin_gate_c.cpp")] + \
      [os.path.join(ROOT, "protocol_amd", "csrc", "pm_host.cpp")]
ENGINE = {"pm_ecrecover_many": 7, "pm_verify_requests": 9, "pm_host_ecrecover": 3}


def _case_file(path):
    keys = [int.from_bytes(hashlib.sha256(b"gate cpp signer %d" % i).digest(), "big") % (M.N - 1) + 1 for i in range(4)]
    with open(path, "w") as f:
        for name, (z, sig) in GC.named().items():
            ok, addr, _ = GC.expected(z, sig)
            f.write(f"case {name} {z.hex()} {sig.hex()} {ok} {addr.hex()}\n")
        for k, key in enumerate(keys):
            addr = M.address_of_key(key)
            for m in range(12):
                msg = b'/heartbeat{"n":%d}' % m
                f.write(f"signed {k} {addr.hex()} {M.sig65(*M.sign(key, M.eip191(msg))).hex()} {msg.decode()}\n")


def test_the_gate_twin_against_the_mock_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe, cases = str(tmp_path / "gate_test"), str(tmp_path / "cases.txt")
    _case_file(cases)
    base = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *[f"-I{d}" for d in INC], *SRC, "-lpthread", "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    r = subprocess.run(base[:1] + san + base[1:], capture_output=True, text=True)
    if r.returncode != 0:  # (a toolchain without the sanitizer runtimes: the plain build still runs every check)
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    out = subprocess.run([exe, cases], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "5 tests, 0 failed checks" in out.stdout, out.stdout + out.stderr[-4000:]


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
        r = re.search(r"fn " + name + r"\(([^;]*)\) -> i32;", ext)
        assert h and r and _arity(h.group(1)) == _arity(r.group(1)) == arity, name
        assert name in E.EXPORTS
        assert re.search(r"\bT " + name + r"\b", eng), f"libpm_engine.so does not define {name}"
    assert re.search(r"\bpm_verify_requests\s*\(", body), "the Rust plugin body does not call pm_verify_requests"
    assert re.search(r"\bU pm_verify_requests\b", plug), "libpm_plugin.so does not import pm_verify_requests"
    pmx = open(os.path.join(PLUGIN, "pm_plugin_c.h")).read()
    assert re.search(r"int32_t pmx_verify_requests\(", pmx) and re.search(r"\bT pmx_verify_requests\b", plug)
    hpp = open(os.path.join(PLUGIN, "gpu_match_plugin.hpp")).read()
    assert re.search(r"pub fn verify_requests\(", body), "the Rust twin has no verify_requests"
    assert re.search(r"\bverify_requests\(", hpp), "the C++ twin has no verify_requests"
    # the verdict's layout is the header's on both sides
    c_fields = re.findall(r"typedef struct pm_rq_verdict \{(.*?)\} pm_rq_verdict;", plain, flags=re.S)[0]
    assert [d.split()[-1].split("[")[0] for d in c_fields.split(";") if d.strip()] == ["code", "row", "status", "_pad", "address"]
    rs_fields = re.search(r"pub struct pm_rq_verdict\s*\{(.*?)\n\}", rs, flags=re.S).group(1)
    assert re.findall(r"pub (\w+)\s*:\s*([^,\n]+)", rs_fields) == [("code", "u32"), ("row", "u32"), ("status", "u8"), ("_pad", "[u8; 3]"),
                                                                    ("address", "[u8; 20]")]
    assert E.RQ_VERDICT.itemsize == 32 and E.RQ_VERDICT.fields["address"][1] == 12
    # gpu_match_plugin.cpp stays linkable against a mock without the new exports
    main = open(os.path.join(PLUGIN, "gpu_match_plugin.cpp")).read() + open(os.path.join(PLUGIN, "pm_plugin_c.cpp")).read()
    assert not re.search(r"\bpm_(verify_requests|ecrecover_many)\s*\(", main)
    assert {"gpu_match_gate.cpp", "pm_plugin_gate_c.cpp"} <= set(B.PLUGIN_SOURCES)
    assert {"pm_secp256k1.inc", "pm_engine_gate.inc"} <= set(B.HEADERS)
    assert re.search(r"#define PM_ABI_VERSION 3\b", hdr)
    kernels = open(os.path.join(B.CSRC, "pm_kernels.hip")).read()
    assert kernels.index('"pm_keccak.inc"') < kernels.index('"pm_secp256k1.inc"')
