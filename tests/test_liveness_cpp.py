"""The liveness sweep's plugin side without a GPU: GpuMatchPlugin::enable_liveness / beat / sweep_statuses and their C face
against a mock (tests/cpp/liveness_test.cpp + tests/cpp/mock_liveness.cpp, a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer: beats from several threads race the sweep and the node sync), and the five new exports agreeing
across the header, protocol_amd.engine.EXPORTS, the Rust twin's extern block and both libraries' dynamic symbol tables."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = [os.path.join(ROOT, "include"), os.path.join(ROOT, "protocol_amd", "plugin"), os.path.join(ROOT, "protocol_amd", "csrc")]
PLUGIN = os.path.join(ROOT, "protocol_amd", "plugin")
SRC = [os.path.join(ROOT, "tests", "cpp", "liveness_test.cpp"), os.path.join(ROOT, "tests", "cpp", "mock_liveness.cpp"),
       os.path.join(ROOT, "tests", "cpp", "mock_engine.cpp"), os.path.join(PLUGIN, "gpu_match_plugin.cpp"),
       os.path.join(PLUGIN, "gpu_match_liveness.cpp"), os.path.join(PLUGIN, "pm_plugin_c.cpp"),
       os.path.join(PLUGIN, "pm_plugin_liveness_c.cpp"), os.path.join(ROOT, "protocol_amd", "csrc", "pm_host.cpp")]
NAMES = {"pm_liveness_enable": 3, "pm_liveness_set": 5, "pm_liveness_get": 5, "pm_liveness_sweep": 7, "pm_liveness_transitions": 4}


def test_sweep_statuses_against_the_mock_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "liveness_test")
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
    for name, arity in NAMES.items():
        h = re.search(r"int32_t " + name + r"\(([^;]*)\);", plain)
        r = re.search(r"fn " + name + r"\(([^;]*)\) -> i32;", ext)
        assert h and r and _arity(h.group(1)) == _arity(r.group(1)) == arity, name
        assert name in E.EXPORTS and re.search(r"\b" + name + r"\s*\(", body), name + ": the Rust plugin body does not call it"
    # pm_live_row: the header, numpy and the repr(C) twin
    c_struct = plain[plain.index("typedef struct pm_live_row {"):plain.index("} pm_live_row;")]
    fields = [(t, f.strip()) for t, decl in re.findall(r"(uint\d+_t) ([^;]+);", c_struct) for f in decl.split(",")]
    assert fields == [("uint32_t", "worker"), ("uint8_t", "old_status"), ("uint8_t", "new_status"), ("uint16_t", "_pad"),
                      ("uint32_t", "counter")]
    assert list(E.live_row_dt.names) == [f for _, f in fields] and E.live_row_dt.itemsize == 12
    assert [E.live_row_dt.fields[f][1] for _, f in fields] == [0, 4, 5, 6, 8]
    r_struct = rs[rs.index("pub struct pm_live_row {"):]
    r_struct = r_struct[:r_struct.index("}")]
    assert re.findall(r"pub (\w+): (\w+)", r_struct) == [(f, "u" + t[4:-2]) for t, f in fields]
    assert "#[repr(C)]" in rs[rs.index("pub struct pm_live_row {") - 60:rs.index("pub struct pm_live_row {")]
    # the statuses, in NodeStatus' order, and the two constants
    enum = re.search(r"enum \{ (PM_NS_DISCOVERED[^}]*)\};", plain).group(1)
    values = {k.strip(): int(v) for k, v in (kv.split("=") for kv in enum.split(","))}
    assert values == {"PM_NS_DISCOVERED": 0, "PM_NS_WAITING": 1, "PM_NS_HEALTHY": 2, "PM_NS_UNHEALTHY": 3, "PM_NS_DEAD": 4,
                      "PM_NS_EJECTED": 5, "PM_NS_BANNED": 6, "PM_NS_LOWBALANCE": 7, "PM_NS_N": 8}
    for k, v in values.items():
        assert getattr(E, k[3:]) == v and f"pub const {k[3:]}: u8 = {v};" in rs, k
    assert "#define PM_LIVE_TTL_MS 90000u" in hdr and "#define PM_LIVE_GIVE_UP 360u" in hdr
    assert (E.LIVE_TTL_MS, E.LIVE_GIVE_UP) == (90000, 360)
    assert "pub const LIVE_TTL_MS: u32 = 90000;" in rs and "pub const LIVE_GIVE_UP: u32 = 360;" in rs
    eng = subprocess.run(["nm", "-D", B.build()], capture_output=True, text=True, check=True).stdout
    plug = subprocess.run(["nm", "-D", "-C", B.build_plugin()], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(r" T " + name + r"$", eng, flags=re.M) and re.search(r"^\s+U " + name + r"$", plug, flags=re.M), name
    for sym in ("orchestrator::GpuMatchPlugin::enable_liveness", "orchestrator::GpuMatchPlugin::beat",
                "orchestrator::GpuMatchPlugin::sweep_statuses", "pmx_enable_liveness", "pmx_beat", "pmx_sweep_statuses"):
        assert re.search(r" T " + re.escape(sym), plug), sym
    assert "#define PM_ABI_VERSION 3" in hdr
    c_face = open(os.path.join(PLUGIN, "pm_plugin_c.h")).read()
    for name in ("pmx_enable_liveness", "pmx_beat", "pmx_sweep_statuses"):
        assert re.search(r"int32_t " + name + r"\(", c_face), name
    for method in ("enable_liveness", "beat", "sweep_statuses"):
        assert re.search(r"pub fn " + method + r"\(&self", rs), method
    # the plugin's main file stays linkable against a mock engine that has not these exports
    main_src = open(os.path.join(PLUGIN, "gpu_match_plugin.cpp")).read()
    assert "pm_liveness_" not in main_src
    # no kernel of the sweep is inline assembly, and the scan is the change feed's own
    kernels = open(os.path.join(ROOT, "protocol_amd", "csrc", "pm_liveness.inc")).read()
    assert "asm" not in kernels and "change_scan_kernel" in kernels and kernels.count("__global__") == 5
