"""The group geography calls without a GPU: GpuMatchPlugin::group_spread / configuration_spread / force_regroup against the mock
engine (tests/cpp/spread_test.cpp + tests/cpp/mock_spread.cpp, a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer), and the three new exports agreeing across the header, protocol_amd.engine.EXPORTS, the Rust twin's
extern block and both libraries' dynamic symbol tables."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = [os.path.join(ROOT, "include"), os.path.join(ROOT, "protocol_amd", "plugin"), os.path.join(ROOT, "protocol_amd", "csrc")]
SRC = [os.path.join(ROOT, "tests", "cpp", "spread_test.cpp"), os.path.join(ROOT, "tests", "cpp", "mock_spread.cpp"),
       os.path.join(ROOT, "tests", "cpp", "mock_engine.cpp"), os.path.join(ROOT, "protocol_amd", "plugin", "gpu_match_plugin.cpp"),
       os.path.join(ROOT, "protocol_amd", "plugin", "gpu_match_spread.cpp"), os.path.join(ROOT, "protocol_amd", "csrc", "pm_host.cpp")]
NEW = ("pm_group_spread", "pm_config_spread", "pm_force_regroup")


def test_spread_against_the_mock_engine_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "spread_test")
    base = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *[f"-I{d}" for d in INC], *SRC, "-lpthread", "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    r = subprocess.run(base[:1] + san + base[1:], capture_output=True, text=True)
    if r.returncode != 0:  # (a toolchain without the sanitizer runtimes: the plain build still runs every check)
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "4 tests, 0 failed checks" in out.stdout, out.stdout + out.stderr[-4000:]


def _arity(decl: str) -> int:
    args = decl[decl.index("(") + 1:decl.rindex(")")]
    return len([a for a in args.split(",") if a.strip()])


def test_the_new_exports_agree_everywhere():
    from protocol_amd import build as B
    from protocol_amd import engine as E
    hdr = open(os.path.join(ROOT, "include", "pm_engine.h")).read()
    rs = open(os.path.join(ROOT, "rust", "gpu_match_plugin.rs")).read()
    ext = rs[rs.index('extern "C" {'):rs.index("\n}\n", rs.index('extern "C" {'))]
    body = rs[rs.index("\n}\n", rs.index('extern "C" {')):]
    for name in NEW:
        h = re.search(r"int32_t " + name + r"\(([^;]*)\);", hdr)
        assert h, name
        r = re.search(r"fn " + name + r"\(([^;]*)\) -> i32;", ext)
        assert r, name
        assert _arity("(" + h.group(1) + ")") == _arity("(" + r.group(1) + ")"), name
        assert name in E.EXPORTS, name
        assert re.search(r"\b" + name + r"\s*\(", body), f"the Rust plugin body does not call {name}"
    # the row structs: the header's fields in order, in C, numpy and Rust, and their sizes
    for struct, dt, size in (("pm_group_spread_row", E.group_spread_dt, 48), ("pm_config_spread_row", E.config_spread_dt, 64)):
        c_struct = hdr[hdr.index("typedef struct " + struct + " {"):hdr.index("} " + struct + ";")]
        c_struct = re.sub(r"/\*.*?\*/", "", c_struct, flags=re.S)
        fields = [f.strip().split("[")[0] for decl in re.findall(r"(?:uint32_t|uint64_t|double) ([^;]+);", c_struct)
                  for f in decl.split(",")]
        assert list(dt.names) == fields and dt.itemsize == size, (struct, fields)
        r_struct = rs[rs.index("pub struct " + struct + " {"):]
        r_struct = r_struct[:r_struct.index("}")]
        assert re.findall(r"pub (\w+):", r_struct) == fields, struct
    assert "hist: [u32; 5]" in rs and E.SPREAD_BUCKETS == 5 and "#define PM_SPREAD_BUCKETS 5" in hdr
    edges = re.search(r"PM_SPREAD_EDGES_KM\[PM_SPREAD_BUCKETS - 1\] = \{([^}]*)\}", hdr).group(1)
    assert tuple(float(x) for x in edges.split(",")) == E.SPREAD_EDGES_KM
    assert (E.REGROUP_ALL, E.REGROUP_DIAMETER, E.REGROUP_LONGEST_HOP) == (0, 1, 2)
    assert "PM_REGROUP_ALL = 0, PM_REGROUP_DIAMETER = 1, PM_REGROUP_LONGEST_HOP = 2" in hdr
    eng = subprocess.run(["nm", "-D", B.build()], capture_output=True, text=True, check=True).stdout
    plug = subprocess.run(["nm", "-D", "-C", B.build_plugin()], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r" T " + name + r"$", eng, flags=re.M), name
        assert re.search(r"^\s+U " + name + r"$", plug, flags=re.M), name
    for sym in ("orchestrator::GpuMatchPlugin::group_spread", "orchestrator::GpuMatchPlugin::configuration_spread",
                "orchestrator::GpuMatchPlugin::force_regroup", "pmx_group_spread", "pmx_configuration_spread", "pmx_force_regroup"):
        assert re.search(r" T " + re.escape(sym), plug), sym
    assert "#define PM_ABI_VERSION 3" in hdr and "pm_group_spread /" in hdr
