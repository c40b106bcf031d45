"""The metrics ledger's plugin side without a GPU: GpuMatchPlugin's metrics methods and their C face against a mock
(tests/cpp/metrics_test.cpp + tests/cpp/mock_metrics.cpp, a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer: the interner, the queue and the one ingest a flush sends, the roll-ups, the reference's own tests,
writers racing a reader), and the new exports agreeing across the header, protocol_amd.engine.EXPORTS, the Rust twin's extern
block and both libraries' dynamic symbol tables."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = [os.path.join(ROOT, "include"), os.path.join(ROOT, "protocol_amd", "plugin"), os.path.join(ROOT, "protocol_amd", "csrc")]
PLUGIN = os.path.join(ROOT, "protocol_amd", "plugin")
SRC = [os.path.join(ROOT, "tests", "cpp", f) for f in ("metrics_test.cpp", "mock_metrics.cpp", "mock_engine.cpp")] + \
      [os.path.join(PLUGIN, f) for f in ("gpu_match_plugin.cpp", "gpu_match_metrics.cpp", "pm_plugin_c.cpp", "pm_plugin_metrics_c.cpp")] + \
      [os.path.join(ROOT, "protocol_amd", "csrc", "pm_host.cpp")]
NAMES = ["pm_metrics_enable", "pm_metrics_ingest", "pm_metrics_totals", "pm_metrics_rows"]


def test_the_metrics_twin_against_the_mock_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "metrics_test")
    base = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *[f"-I{d}" for d in INC], *SRC, "-lpthread", "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    r = subprocess.run(base[:1] + san + base[1:], capture_output=True, text=True)
    if r.returncode != 0:  # (a toolchain without the sanitizer runtimes: the plain build still runs every check)
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "6 tests, 0 failed checks" in out.stdout, out.stdout + out.stderr[-4000:]


def _arity(args: str) -> int:
    return len([a for a in args.split(",") if a.strip()])


def _c_fields(plain, name):
    body = plain[plain.index("typedef struct %s {" % name):plain.index("} %s;" % name)]
    return [(t, f.strip()) for t, decl in re.findall(r"(uint\d+_t|double) ([^;]+);", body) for f in decl.split(",")]


def test_the_new_exports_agree_everywhere():
    from protocol_amd import build as B
    from protocol_amd import engine as E
    hdr = open(os.path.join(ROOT, "include", "pm_engine.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    rs = open(os.path.join(ROOT, "rust", "gpu_match_plugin.rs")).read()
    ext = rs[rs.index('extern "C" {'):rs.index("\n}\n", rs.index('extern "C" {'))]
    body = rs[rs.index("\n}\n", rs.index('extern "C" {')):]
    eng = subprocess.run(["nm", "-D", B.build()], capture_output=True, text=True, check=True).stdout
    plug = subprocess.run(["nm", "-D", "-C", B.build_plugin()], capture_output=True, text=True, check=True).stdout
    for name, arity in zip(NAMES, (2, 6, 5, 6)):
        h = re.search(r"int32_t " + name + r"\(([^;]*)\);", plain)
        r = re.search(r"fn " + name + r"\(([^;]*)\) -> i32;", ext)
        assert h and r and _arity(h.group(1)) == _arity(r.group(1)) == arity, name
        assert name in E.EXPORTS and re.search(r"\b" + name + r"\s*\(", body), f"the Rust plugin body does not call {name}"
        assert re.search(r" T " + name + r"$", eng, flags=re.M) and re.search(r"^\s+U " + name + r"$", plug, flags=re.M), name
        # the plugin's main file stays linkable against a mock engine that has not the export
        assert name not in open(os.path.join(PLUGIN, "gpu_match_plugin.cpp")).read()
    # the three structs: the header, numpy and the repr(C) twins
    want = {"pm_mx_beat": ([("uint32_t", "row"), ("uint32_t", "kind"), ("uint32_t", "first"), ("uint32_t", "n")], [0, 4, 8, 12], 16, E.mx_beat_dt),
            "pm_mx_entry": ([("uint32_t", "series"), ("uint32_t", "flags"), ("double", "value")], [0, 4, 8], 16, E.mx_entry_dt),
            "pm_mx_row": ([("uint32_t", "row"), ("uint32_t", "series"), ("double", "value"), ("uint64_t", "group_id"), ("uint32_t", "config"),
                           ("uint32_t", "_pad")], [0, 4, 8, 16, 24, 28], 32, E.mx_row_dt)}
    for struct, (fields, offsets, size, dt) in want.items():
        assert _c_fields(plain, struct) == fields, struct
        assert list(dt.names) == [f for _, f in fields] and dt.itemsize == size
        assert [dt.fields[f][1] for _, f in fields] == offsets
        at = rs.index("pub struct %s {" % struct)
        r_struct = rs[at:rs.index("}", at)]
        assert re.findall(r"pub (\w+): (\w+)", r_struct) == [(f, "f64" if t == "double" else "u" + t[4:-2]) for t, f in fields], struct
        assert "#[repr(C)]" in rs[at - 60:at]
    # the constants
    assert re.search(r"#define PM_MX_MANUAL 0xFFFFFFFFu\b", hdr) and re.search(r"#define PM_MX_ROW_MAX 1024u\b", hdr)
    assert (E.MX_MANUAL, E.MX_ROW_MAX) == (0xFFFFFFFF, 1024) and E.MX_ROW_MAX >= 1024
    assert "pub const MX_MANUAL: u32 = 0xFFFF_FFFF;" in rs and "pub const MX_ROW_MAX: u32 = 1024;" in rs
    kinds = re.search(r"enum \{ (PM_MXB_REPLACE[^}]*)\};", plain).group(1)
    values = {k.strip(): int(v) for k, v in (kv.split("=") for kv in kinds.split(","))}
    assert values == {"PM_MXB_REPLACE": 0, "PM_MXB_MERGE": 1, "PM_MXB_DELETE": 2}
    for k, v in list(values.items()) + [("PM_MXF_MAX", 1)]:
        assert getattr(E, k[3:]) == v and f"pub const {k[3:]}: u32 = {v};" in rs, k
    assert re.search(r"enum \{ PM_MXF_MAX = 1 \};", plain)
    # both twins carry the surface, the C face declares what it defines
    methods = ("enable_metrics", "beat_metrics", "store_metrics", "store_manual_metric", "delete_metric", "clear_metrics", "flush_metrics",
               "aggregate_metrics_for_all_tasks", "aggregate_metrics_for_task", "metrics_for_node", "all_metrics", "synced_metrics")
    for method in methods:
        assert re.search(r" T orchestrator::GpuMatchPlugin::" + method + r"(\[abi:cxx11\])?\(", plug), method
        assert re.search(r"pub fn " + method + r"\(&self", rs), method
    c_face = open(os.path.join(PLUGIN, "pm_plugin_c.h")).read()
    for fn in ("pmx_enable_metrics", "pmx_beat_metrics", "pmx_store_metrics", "pmx_store_manual_metric", "pmx_delete_metric",
               "pmx_clear_metrics", "pmx_flush_metrics", "pmx_aggregate_metrics", "pmx_metrics_for_node", "pmx_synced_metrics"):
        assert re.search(r"int32_t " + fn + r"\(", c_face) and re.search(r" T " + fn + r"$", plug, flags=re.M), fn
    # no floating-point atomics in the kernels (the totals are deterministic), no inline assembly
    kernels = open(os.path.join(ROOT, "protocol_amd", "csrc", "pm_metrics.inc")).read()
    code = re.sub(r"//[^\n]*", "", kernels)
    assert "asm" not in code and not re.search(r"atomicAdd\([^;]*(double|float|sum|val)", code)
    assert ABI_STAYS_3(hdr)


def ABI_STAYS_3(hdr):
    return re.search(r"#define PM_ABI_VERSION 3\b", hdr) is not None
