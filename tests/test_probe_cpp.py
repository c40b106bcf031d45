"""The probe calls without a GPU: GpuMatchPlugin::probe_configurations / configuration_overlap and their C face against the
mock engine (tests/cpp/probe_test.cpp + tests/cpp/mock_probe.cpp, a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer), and the two new exports agreeing across the header, protocol_amd.engine.EXPORTS, the Rust twin's
extern block and body, the struct's fields, both libraries' dynamic symbol tables and the C face."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = [os.path.join(ROOT, "include"), os.path.join(ROOT, "protocol_amd", "plugin"), os.path.join(ROOT, "protocol_amd", "csrc")]
PLUGIN = os.path.join(ROOT, "protocol_amd", "plugin")
SRC = [os.path.join(ROOT, "tests", "cpp", "probe_test.cpp"), os.path.join(ROOT, "tests", "cpp", "mock_probe.cpp"),
       os.path.join(ROOT, "tests", "cpp", "mock_engine.cpp"), os.path.join(PLUGIN, "gpu_match_plugin.cpp"),
       os.path.join(PLUGIN, "gpu_match_probe.cpp"), os.path.join(PLUGIN, "pm_plugin_c.cpp"),
       os.path.join(PLUGIN, "pm_plugin_probe_c.cpp"), os.path.join(ROOT, "protocol_amd", "csrc", "pm_host.cpp")]


def test_probe_methods_against_the_mock_engine_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "probe_test")
    base = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *[f"-I{d}" for d in INC], *SRC, "-lpthread", "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    r = subprocess.run(base[:1] + san + base[1:], capture_output=True, text=True)
    if r.returncode != 0:  # (a toolchain without the sanitizer runtimes: the plain build still runs every check)
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "4 tests, 0 failed checks" in out.stdout, out.stdout + out.stderr[-4000:]


def _arity(args: str) -> int:
    return len([a for a in re.sub(r"/\*.*?\*/", "", args, flags=re.S).split(",") if a.strip()])


def test_the_new_exports_agree_everywhere():
    from protocol_amd import build as B
    from protocol_amd import engine as E
    hdr = open(os.path.join(ROOT, "include", "pm_engine.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    rs = open(os.path.join(ROOT, "rust", "gpu_match_plugin.rs")).read()
    ext = rs[rs.index('extern "C" {'):rs.index("\n}\n", rs.index('extern "C" {'))]
    body = rs[rs.index("\n}\n", rs.index('extern "C" {')):]
    for name, arity in (("pm_probe_configs", 11), ("pm_config_overlap", 4)):
        h = re.search(r"int32_t " + name + r"\(([^;]*)\);", plain)
        r = re.search(r"fn " + name + r"\(([^;]*)\) -> i32;", ext)
        assert h and r and _arity(h.group(1)) == _arity(r.group(1)) == arity, name
        assert name in E.EXPORTS and re.search(r"\b" + name + r"\s*\(", body), name + ": the Rust plugin body does not call it"
        assert len(getattr(E.lib(), name).argtypes) == arity
    # the struct: the header's fields, the numpy record and the Rust #[repr(C)] struct, in order
    c_struct = plain[plain.index("typedef struct pm_probe_row {"):plain.index("} pm_probe_row;")]
    fields = [f.strip() for decl in re.findall(r"uint32_t ([^;]+);", c_struct) for f in decl.split(",")]
    assert fields[0] == "why[PM_WHY_N]" and "PM_WHY_N = 10" in hdr
    fields[0] = "why"
    assert list(E.probe_row_dt.names) == fields and E.probe_row_dt.itemsize == 4 * (len(fields) - 1 + 10)
    assert E.probe_row_dt["why"].shape == (10,)
    r_struct = rs[rs.index("pub struct pm_probe_row {"):]
    r_struct = r_struct[:r_struct.index("}")]
    assert re.findall(r"pub (\w+): (?:u32|\[u32; 10\])", r_struct) == fields and "pub why: [u32; 10]" in r_struct
    eng = subprocess.run(["nm", "-D", B.build()], capture_output=True, text=True, check=True).stdout
    plug = subprocess.run(["nm", "-D", "-C", B.build_plugin()], capture_output=True, text=True, check=True).stdout
    for name in ("pm_probe_configs", "pm_config_overlap"):
        assert re.search(r" T " + name + r"$", eng, flags=re.M) and re.search(r"^\s+U " + name + r"$", plug, flags=re.M), name
    for sym in ("orchestrator::GpuMatchPlugin::probe_configurations", "orchestrator::GpuMatchPlugin::configuration_overlap",
                "pmx_probe_configurations", "pmx_configuration_overlap"):
        assert re.search(r" T " + re.escape(sym), plug), sym
    assert "#define PM_ABI_VERSION 3" in hdr and "pm_probe_configs / pm_config_overlap (probes and configuration overlap)" in hdr
    c_face = open(os.path.join(PLUGIN, "pm_plugin_c.h")).read()
    assert re.search(r"int32_t pmx_probe_configurations\(", c_face) and re.search(r"int32_t pmx_configuration_overlap\(", c_face)
    assert re.search(r"pub fn probe_configurations\(&self", rs) and re.search(r"pub fn configuration_overlap\(&self", rs)
