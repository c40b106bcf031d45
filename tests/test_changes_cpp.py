"""The assignment change feed without a GPU: GpuMatchPlugin::changed_nodes and its C face pmx_changed_nodes against a scripted
mock (tests/cpp/changes_test.cpp + tests/cpp/mock_changes.cpp, a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer), and the two new exports agreeing across the header, protocol_amd.engine.EXPORTS, the Rust twin's
extern block and both libraries' dynamic symbol tables."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = [os.path.join(ROOT, "include"), os.path.join(ROOT, "protocol_amd", "plugin"), os.path.join(ROOT, "protocol_amd", "csrc")]
PLUGIN = os.path.join(ROOT, "protocol_amd", "plugin")
SRC = [os.path.join(ROOT, "tests", "cpp", "changes_test.cpp"), os.path.join(ROOT, "tests", "cpp", "mock_changes.cpp"),
       os.path.join(ROOT, "tests", "cpp", "mock_engine.cpp"), os.path.join(PLUGIN, "gpu_match_plugin.cpp"),
       os.path.join(PLUGIN, "gpu_match_changes.cpp"), os.path.join(PLUGIN, "pm_plugin_c.cpp"),
       os.path.join(PLUGIN, "pm_plugin_changes_c.cpp"), os.path.join(ROOT, "protocol_amd", "csrc", "pm_host.cpp")]


def test_changed_nodes_against_the_scripted_mock_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "changes_test")
    base = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *[f"-I{d}" for d in INC], *SRC, "-lpthread", "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    r = subprocess.run(base[:1] + san + base[1:], capture_output=True, text=True)
    if r.returncode != 0:  # (a toolchain without the sanitizer runtimes: the plain build still runs every check)
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "4 tests, 0 failed checks" in out.stdout, out.stdout + out.stderr[-4000:]


def _arity(args: str) -> int:
    return len([a for a in args.split(",") if a.strip()])


def test_the_new_exports_agree_everywhere():
    from protocol_amd import build as B
    from protocol_amd import engine as E
    hdr = open(os.path.join(ROOT, "include", "pm_engine.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    rs = open(os.path.join(ROOT, "rust", "gpu_match_plugin.rs")).read()
    ext = rs[rs.index('extern "C" {'):rs.index("\n}\n", rs.index('extern "C" {'))]
    body = rs[rs.index("\n}\n", rs.index('extern "C" {')):]
    for name, arity in (("pm_enable_assignment_changes", 2), ("pm_drain_assignment_changes", 5)):
        h = re.search(r"int32_t " + name + r"\(([^;]*)\);", plain)
        r = re.search(r"fn " + name + r"\(([^;]*)\) -> i32;", ext)
        assert h and r and _arity(h.group(1)) == _arity(r.group(1)) == arity, name
        assert name in E.EXPORTS and re.search(r"\b" + name + r"\s*\(", body), name + ": the Rust plugin body does not call it"
    c_struct = plain[plain.index("typedef struct pm_change_row {"):plain.index("} pm_change_row;")]
    fields = [f.strip() for decl in re.findall(r"uint32_t ([^;]+);", c_struct) for f in decl.split(",")]
    assert list(E.change_row_dt.names) == fields == ["worker", "what"] and E.change_row_dt.itemsize == 4 * len(fields)
    r_struct = rs[rs.index("pub struct pm_change_row {"):]
    assert re.findall(r"pub (\w+): u32", r_struct[:r_struct.index("}")]) == fields
    assert "enum { PM_CHG_GROUP = 1, PM_CHG_RING = 2, PM_CHG_TASK = 4 };" in hdr
    assert (E.CHG_GROUP, E.CHG_RING, E.CHG_TASK) == (1, 2, 4)
    for const, val in (("CHG_GROUP", 1), ("CHG_RING", 2), ("CHG_TASK", 4), ("CHANGES_RESYNC", 1)):
        assert f"pub const {const}: u32 = {val};" in rs, const
    assert "#define PM_CHANGES_RESYNC 1u" in hdr and E.CHANGES_RESYNC == 1
    eng = subprocess.run(["nm", "-D", B.build()], capture_output=True, text=True, check=True).stdout
    plug = subprocess.run(["nm", "-D", "-C", B.build_plugin()], capture_output=True, text=True, check=True).stdout
    for name in ("pm_enable_assignment_changes", "pm_drain_assignment_changes"):
        assert re.search(r" T " + name + r"$", eng, flags=re.M) and re.search(r"^\s+U " + name + r"$", plug, flags=re.M), name
    for sym in ("orchestrator::GpuMatchPlugin::enable_change_feed", "orchestrator::GpuMatchPlugin::changed_nodes",
                "pmx_enable_change_feed", "pmx_changed_nodes"):
        assert re.search(r" T " + re.escape(sym), plug), sym
    assert "#define PM_ABI_VERSION 3" in hdr
    assert "pm_enable_assignment_changes / pm_drain_assignment_changes (assignment change feed)" in hdr
    c_face = open(os.path.join(PLUGIN, "pm_plugin_c.h")).read()
    assert re.search(r"int32_t pmx_enable_change_feed\(", c_face) and re.search(r"int32_t pmx_changed_nodes\(", c_face)
    assert re.search(r"pub fn changed_nodes\(&self", rs) and re.search(r"pub fn enable_change_feed\(&self", rs)
    # the plugin's main file stays linkable against a mock engine that has not these exports
    main_src = open(os.path.join(PLUGIN, "gpu_match_plugin.cpp")).read()
    assert "assignment_changes" not in main_src and "changed_nodes" not in main_src and "enable_change_feed" not in main_src
