"""The diagnostics reports without a GPU: GpuMatchPlugin::explain_node / configuration_report / task_report against the mock
engine (tests/cpp/report_test.cpp + tests/cpp/mock_report.cpp, under AddressSanitizer and UndefinedBehaviorSanitizer), and the
three new exports agreeing across the header, protocol_amd.engine.EXPORTS, the Rust twin's extern block and both libraries'
dynamic symbol tables."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = [os.path.join(ROOT, "include"), os.path.join(ROOT, "protocol_amd", "plugin"), os.path.join(ROOT, "protocol_amd", "csrc")]
SRC = [os.path.join(ROOT, "tests", "cpp", "report_test.cpp"), os.path.join(ROOT, "tests", "cpp", "mock_report.cpp"),
       os.path.join(ROOT, "tests", "cpp", "mock_engine.cpp"), os.path.join(ROOT, "protocol_amd", "plugin", "gpu_match_plugin.cpp"),
       os.path.join(ROOT, "protocol_amd", "plugin", "gpu_match_report.cpp"), os.path.join(ROOT, "protocol_amd", "csrc", "pm_host.cpp")]
NEW = ("pm_explain_workers", "pm_config_report", "pm_task_report")


def test_reports_against_the_mock_engine_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "report_test")
    base = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *[f"-I{d}" for d in INC], *SRC, "-lpthread", "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    r = subprocess.run(base[:1] + san + base[1:], capture_output=True, text=True)
    if r.returncode != 0:  # (a toolchain without the sanitizer runtimes: the plain build still runs every check)
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "3 tests, 0 failed checks" in out.stdout, out.stdout + out.stderr[-4000:]


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
    # the row struct: seventeen u32 in the header's order, in C, numpy and Rust
    fields = ["enabled", "eligible_meets", "idle_meets", "why", "groups", "members", "groups_without_task", "tasks_allowing"]
    assert list(E.config_report_dt.names) == fields and E.config_report_dt.itemsize == 17 * 4
    c_struct = hdr[hdr.index("typedef struct pm_config_report_row {"):hdr.index("} pm_config_report_row;")]
    assert re.findall(r"uint32_t (\w+)", c_struct) == fields
    r_struct = rs[rs.index("pub struct pm_config_report_row {"):]
    r_struct = r_struct[:r_struct.index("}")]
    assert re.findall(r"pub (\w+):", r_struct) == fields and "why: [u32; 10]" in r_struct
    eng = subprocess.run(["nm", "-D", B.build()], capture_output=True, text=True, check=True).stdout
    plug = subprocess.run(["nm", "-D", "-C", B.build_plugin()], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r" T " + name + r"$", eng, flags=re.M), name
        assert re.search(r"^\s+U " + name + r"$", plug, flags=re.M), name
    for sym in ("orchestrator::GpuMatchPlugin::explain_node", "orchestrator::GpuMatchPlugin::configuration_report",
                "orchestrator::GpuMatchPlugin::task_report", "pmx_explain_node", "pmx_configuration_report", "pmx_task_report"):
        assert re.search(r" T " + re.escape(sym), plug), sym
    assert "#define PM_ABI_VERSION 3" in hdr and "pm_explain_workers /" in hdr
