"""The discovery sync's plugin side without a GPU: GpuMatchPlugin::set_endpoint / sync_discovery and their C face against a mock
(tests/cpp/discovery_test.cpp + tests/cpp/mock_discovery.cpp, a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer: the sync races beats, status changes, the sweep and the node sync), and the new export agreeing
across the header, protocol_amd.engine.EXPORTS, the Rust twin's extern block and both libraries' dynamic symbol tables."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = [os.path.join(ROOT, "include"), os.path.join(ROOT, "protocol_amd", "plugin"), os.path.join(ROOT, "protocol_amd", "csrc")]
PLUGIN = os.path.join(ROOT, "protocol_amd", "plugin")
SRC = [os.path.join(ROOT, "tests", "cpp", f) for f in ("discovery_test.cpp", "mock_discovery.cpp", "mock_liveness.cpp", "mock_engine.cpp")] + \
      [os.path.join(PLUGIN, f) for f in ("gpu_match_plugin.cpp", "gpu_match_liveness.cpp", "gpu_match_discovery.cpp", "pm_plugin_c.cpp",
                                         "pm_plugin_liveness_c.cpp", "pm_plugin_discovery_c.cpp")] + \
      [os.path.join(ROOT, "protocol_amd", "csrc", "pm_host.cpp")]


def test_sync_discovery_against_the_mock_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "discovery_test")
    base = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *[f"-I{d}" for d in INC], *SRC, "-lpthread", "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    r = subprocess.run(base[:1] + san + base[1:], capture_output=True, text=True)
    if r.returncode != 0:  # (a toolchain without the sanitizer runtimes: the plain build still runs every check)
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "5 tests, 0 failed checks" in out.stdout, out.stdout + out.stderr[-4000:]


def _arity(args: str) -> int:
    return len([a for a in args.split(",") if a.strip()])


def _c_fields(plain, name):
    body = plain[plain.index("typedef struct %s {" % name):plain.index("} %s;" % name)]
    return [(t, f.strip()) for t, decl in re.findall(r"(uint\d+_t) ([^;]+);", body) for f in decl.split(",")]


def test_the_new_export_agrees_everywhere():
    from protocol_amd import build as B
    from protocol_amd import engine as E
    hdr = open(os.path.join(ROOT, "include", "pm_engine.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    rs = open(os.path.join(ROOT, "rust", "gpu_match_plugin.rs")).read()
    ext = rs[rs.index('extern "C" {'):rs.index("\n}\n", rs.index('extern "C" {'))]
    body = rs[rs.index("\n}\n", rs.index('extern "C" {')):]
    name = "pm_discovery_sync"
    h = re.search(r"int32_t " + name + r"\(([^;]*)\);", plain)
    r = re.search(r"fn " + name + r"\(([^;]*)\) -> i32;", ext)
    assert h and r and _arity(h.group(1)) == _arity(r.group(1)) == 10
    assert name in E.EXPORTS and re.search(r"\b" + name + r"\s*\(", body), "the Rust plugin body does not call it"
    # the two structs: the header, numpy and the repr(C) twins
    rows = _c_fields(plain, "pm_disc_row")
    assert rows == [("uint32_t", "row"), ("uint32_t", "endpoint"), ("uint32_t", "endpoint_after"), ("uint32_t", "flags"),
                    ("uint64_t", "last_change_ms"), ("uint64_t", "last_updated_ms")]
    assert list(E.disc_row_dt.names) == [f for _, f in rows] and E.disc_row_dt.itemsize == 32
    assert [E.disc_row_dt.fields[f][1] for _, f in rows] == [0, 4, 8, 12, 16, 24]
    res = _c_fields(plain, "pm_disc_result")
    assert res == [("uint32_t", "healthy_same_endpoint"), ("uint8_t", "old_status"), ("uint8_t", "final_status"), ("uint8_t", "n_updates"),
                   ("uint8_t", "ops"), ("uint8_t", "upd_old[3]"), ("uint8_t", "upd_new[3]"), ("uint16_t", "_pad")]
    assert list(E.disc_result_dt.names) == [f.split("[")[0] for _, f in res] and E.disc_result_dt.itemsize == 16
    assert [E.disc_result_dt.fields[f.split("[")[0]][1] for _, f in res] == [0, 4, 5, 6, 7, 8, 11, 14]
    for struct, fields in (("pm_disc_row", rows), ("pm_disc_result", res)):
        at = rs.index("pub struct %s {" % struct)
        r_struct = rs[at:rs.index("}", at)]
        want = [(f.split("[")[0], ("[u8; 3]" if "[3]" in f else "u" + t[4:-2])) for t, f in fields]
        assert re.findall(r"pub (\w+): (\[u8; 3\]|\w+)", r_struct) == want, struct
        assert "#[repr(C)]" in rs[at - 60:at]
    # the constants
    for k, v in (("PM_DISC_NEW", "0xFFFFFFFFu"), ("PM_EP_NONE", "0xFFFFFFFFu"), ("PM_DISC_GRACE_MS", "300000u")):
        assert re.search(r"#define %s %s\b" % (k, v), hdr), k
    assert (E.DISC_NEW, E.EP_NONE, E.DISC_GRACE_MS) == (0xFFFFFFFF, 0xFFFFFFFF, 300000)
    assert "pub const DISC_NEW: u32 = 0xFFFF_FFFF;" in rs and "pub const EP_NONE: u32 = 0xFFFF_FFFF;" in rs
    assert "pub const DISC_GRACE_MS: u32 = 300000;" in rs
    for prefix, first in (("PM_DF_", "PM_DF_VALIDATED"), ("PM_DO_", "PM_DO_ADMIT")):
        enum = re.search(r"enum \{ (" + first + r"[^}]*)\};", plain).group(1)
        values = {k.strip(): int(v) for k, v in (kv.split("=") for kv in enum.split(","))}
        assert sorted(values.values()) == [1, 2, 4, 8, 16, 32]
        for k, v in values.items():
            assert getattr(E, k[3:]) == v and f"pub const {k[3:]}: u32 = {v};" in rs, k
    eng = subprocess.run(["nm", "-D", B.build()], capture_output=True, text=True, check=True).stdout
    plug = subprocess.run(["nm", "-D", "-C", B.build_plugin()], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T " + name + r"$", eng, flags=re.M) and re.search(r"^\s+U " + name + r"$", plug, flags=re.M)
    for sym in ("orchestrator::GpuMatchPlugin::sync_discovery", "orchestrator::GpuMatchPlugin::set_endpoint", "pmx_sync_discovery",
                "pmx_set_endpoint"):
        assert re.search(r" T " + re.escape(sym), plug), sym
    c_face = open(os.path.join(PLUGIN, "pm_plugin_c.h")).read()
    for fn in ("pmx_sync_discovery", "pmx_set_endpoint"):
        assert re.search(r"int32_t " + fn + r"\(", c_face), fn
    for method in ("sync_discovery", "set_endpoint"):
        assert re.search(r"pub fn " + method + r"\(&self", rs), method
    # the plugin's main file stays linkable against a mock engine that has not the export
    assert "pm_discovery_sync" not in open(os.path.join(PLUGIN, "gpu_match_plugin.cpp")).read()
    # one statement of the row rule, used by the count, the scatter and the decision; no inline assembly
    kernels = open(os.path.join(ROOT, "protocol_amd", "csrc", "pm_discovery.inc")).read()
    assert "asm" not in kernels and kernels.count("__global__") == 5
    assert len(re.findall(r"\bDiscStep disc_rule\(", kernels)) == 1 and len(re.findall(r"= disc_rule\(", kernels)) == 2
