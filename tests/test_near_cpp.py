"""The nearest-candidates call without a GPU: GpuMatchPlugin::nearest_nodes and its C face pmx_nearest_nodes against the mock
engine (tests/cpp/near_test.cpp + tests/cpp/mock_near.cpp, a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer), and the new export agreeing across the header, protocol_amd.engine.EXPORTS, the Rust twin's
extern block and both libraries' dynamic symbol tables."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = [os.path.join(ROOT, "include"), os.path.join(ROOT, "protocol_amd", "plugin"), os.path.join(ROOT, "protocol_amd", "csrc")]
PLUGIN = os.path.join(ROOT, "protocol_amd", "plugin")
SRC = [os.path.join(ROOT, "tests", "cpp", "near_test.cpp"), os.path.join(ROOT, "tests", "cpp", "mock_near.cpp"),
       os.path.join(ROOT, "tests", "cpp", "mock_engine.cpp"), os.path.join(PLUGIN, "gpu_match_plugin.cpp"),
       os.path.join(PLUGIN, "gpu_match_near.cpp"), os.path.join(PLUGIN, "pm_plugin_c.cpp"),
       os.path.join(PLUGIN, "pm_plugin_near_c.cpp"), os.path.join(ROOT, "protocol_amd", "csrc", "pm_host.cpp")]


def test_nearest_nodes_against_the_mock_engine_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "near_test")
    base = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *[f"-I{d}" for d in INC], *SRC, "-lpthread", "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    r = subprocess.run(base[:1] + san + base[1:], capture_output=True, text=True)
    if r.returncode != 0:  # (a toolchain without the sanitizer runtimes: the plain build still runs every check)
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "3 tests, 0 failed checks" in out.stdout, out.stdout + out.stderr[-4000:]


def _arity(args: str) -> int:
    return len([a for a in args.split(",") if a.strip()])


def test_the_new_export_agrees_everywhere():
    from protocol_amd import build as B
    from protocol_amd import engine as E
    hdr = open(os.path.join(ROOT, "include", "pm_engine.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    rs = open(os.path.join(ROOT, "rust", "gpu_match_plugin.rs")).read()
    ext = rs[rs.index('extern "C" {'):rs.index("\n}\n", rs.index('extern "C" {'))]
    body = rs[rs.index("\n}\n", rs.index('extern "C" {')):]
    name = "pm_nearest_workers"
    h = re.search(r"int32_t " + name + r"\(([^;]*)\);", plain)
    r = re.search(r"fn " + name + r"\(([^;]*)\) -> i32;", ext)
    assert h and r and _arity(h.group(1)) == _arity(r.group(1)) == 8
    assert name in E.EXPORTS and re.search(r"\b" + name + r"\s*\(", body), "the Rust plugin body does not call it"
    for struct, dt in (("pm_near_query", E.near_query_dt), ("pm_near_row", E.near_row_dt)):
        c_struct = plain[plain.index("typedef struct " + struct + " {"):plain.index("} " + struct + ";")]
        fields = [f.strip() for decl in re.findall(r"uint32_t ([^;]+);", c_struct) for f in decl.split(",")]
        assert list(dt.names) == fields and dt.itemsize == 4 * len(fields), (struct, fields)
        r_struct = rs[rs.index("pub struct " + struct + " {"):]
        assert re.findall(r"pub (\w+): u32", r_struct[:r_struct.index("}")]) == fields, struct
    assert "enum { PM_NEAR_IDLE = 0," in hdr and "PM_NEAR_ELIGIBLE = 1 }" in hdr and (E.NEAR_IDLE, E.NEAR_ELIGIBLE) == (0, 1)
    assert "#define PM_NEAR_SEED 0xFFFFFFFEu" in hdr and E.NEAR_SEED == 0xFFFFFFFE and "NEAR_SEED: u32 = 0xFFFF_FFFE" in rs
    assert "#define PM_NEAR_MAX_K 256u" in hdr and E.NEAR_MAX_K == 256 and "NEAR_MAX_K: u32 = 256" in rs
    assert "#define PM_NEAR_MAX_QUERIES 65535u" in hdr and E.NEAR_MAX_QUERIES == 65535
    eng = subprocess.run(["nm", "-D", B.build()], capture_output=True, text=True, check=True).stdout
    plug = subprocess.run(["nm", "-D", "-C", B.build_plugin()], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T " + name + r"$", eng, flags=re.M) and re.search(r"^\s+U " + name + r"$", plug, flags=re.M)
    for sym in ("orchestrator::GpuMatchPlugin::nearest_nodes", "pmx_nearest_nodes"):
        assert re.search(r" T " + re.escape(sym), plug), sym
    assert "#define PM_ABI_VERSION 3" in hdr and "pm_nearest_workers (nearest candidates)" in hdr
    c_face = open(os.path.join(PLUGIN, "pm_plugin_c.h")).read()
    assert re.search(r"int32_t pmx_nearest_nodes\(", c_face) and re.search(r"pub fn nearest_nodes\(&self", rs)
