"""Restart and switch-over without a GPU: GpuMatchPlugin::restore_groups against the mock engine (tests/cpp/restore_test.cpp
+ tests/cpp/mock_adopt.cpp, under AddressSanitizer and UndefinedBehaviorSanitizer), and the two new exports agreeing across
the header, protocol_amd.engine.EXPORTS, the Rust twin's extern block and both libraries' dynamic symbol tables."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = [os.path.join(ROOT, "include"), os.path.join(ROOT, "protocol_amd", "plugin"), os.path.join(ROOT, "protocol_amd", "csrc")]
SRC = [os.path.join(ROOT, "tests", "cpp", "restore_test.cpp"), os.path.join(ROOT, "tests", "cpp", "mock_adopt.cpp"),
       os.path.join(ROOT, "tests", "cpp", "mock_engine.cpp"), os.path.join(ROOT, "protocol_amd", "plugin", "gpu_match_plugin.cpp"),
       os.path.join(ROOT, "protocol_amd", "plugin", "gpu_match_restore.cpp"), os.path.join(ROOT, "protocol_amd", "csrc", "pm_host.cpp")]
NEW = ("pm_adopt_groups", "pm_group_id_state")


def test_restore_groups_against_the_mock_engine_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "restore_test")
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
    assert "u64) -> i32" in re.search(r"fn pm_adopt_groups\([^;]*;", ext).group(0)
    assert "state: *mut u64" in re.search(r"fn pm_group_id_state\([^;]*;", ext).group(0)
    eng = subprocess.run(["nm", "-D", B.build()], capture_output=True, text=True, check=True).stdout
    plug = subprocess.run(["nm", "-D", "-C", B.build_plugin()], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r" T " + name + r"$", eng, flags=re.M), name
        assert re.search(r"^\s+U " + name + r"$", plug, flags=re.M), name
    for sym in ("orchestrator::GpuMatchPlugin::restore_groups", "orchestrator::GpuMatchPlugin::group_tasks",
                "orchestrator::GpuMatchPlugin::group_id_state() const", "pmx_restore_groups", "pmx_group_tasks",
                "pmx_group_id_state", "pmx_take_restore_report"):
        assert re.search(r" T " + re.escape(sym), plug), sym
    # the ABI version stays 3: the two calls are compatible additions, and the header's history says so
    assert "#define PM_ABI_VERSION 3" in hdr and "pm_adopt_groups / pm_group_id_state" in hdr
