"""The task directory's plugin side without a GPU: GpuMatchPlugin's task directory methods and their C face against a mock
(tests/cpp/taskdir_test.cpp + tests/cpp/mock_taskdir.cpp, a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer: the query each method sends, paging, the "present only" rule of the statistics, the "unknown" name,
the texts and their sizing), and the new names agreeing across the header, protocol_amd.engine.EXPORTS, the Rust twin's extern
block, both libraries' dynamic symbol tables and the struct layouts."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = [os.path.join(ROOT, "include"), os.path.join(ROOT, "protocol_amd", "plugin"), os.path.join(ROOT, "protocol_amd", "csrc")]
PLUGIN = os.path.join(ROOT, "protocol_amd", "plugin")
SRC = [os.path.join(ROOT, "tests", "cpp", f) for f in ("taskdir_test.cpp", "mock_taskdir.cpp", "mock_directory.cpp", "mock_groupdir.cpp",
                                                        "mock_rollout.cpp", "mock_engine.cpp")] + \
      [os.path.join(PLUGIN, f) for f in ("gpu_match_plugin.cpp", "gpu_match_taskdir.cpp", "gpu_match_directory.cpp", "gpu_match_groupdir.cpp",
                                         "gpu_match_rollout.cpp", "pm_plugin_c.cpp", "pm_plugin_taskdir_c.cpp")] + \
      [os.path.join(ROOT, "protocol_amd", "csrc", "pm_host.cpp")]
PMX = ["pmx_list_tasks", "pmx_task_counts", "pmx_starved_tasks", "pmx_orchestrator_statistics"]
METHODS = ("list_tasks", "task_counts", "starved_tasks", "orchestrator_statistics")


def test_the_task_directory_twin_against_the_mock_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "taskdir_test")
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
    h = re.search(r"int32_t pm_task_directory\(([^;]*)\);", plain)
    r = re.search(r"fn pm_task_directory\(([^;]*)\) -> i32;", ext)
    assert h and r and _arity(h.group(1)) == _arity(r.group(1)) == 8
    assert "pm_task_directory" in E.EXPORTS
    assert re.search(r"\bpm_task_directory\s*\(", body), "the Rust plugin body does not call pm_task_directory"
    assert re.search(r"\bT pm_task_directory\b", eng), "libpm_engine.so does not define pm_task_directory"
    assert re.search(r"\bU pm_task_directory\b", plug), "libpm_plugin.so does not import pm_task_directory"
    pmx = open(os.path.join(PLUGIN, "pm_plugin_c.h")).read()
    for name in PMX:
        assert re.search(r"int32_t " + name + r"\(", pmx) and re.search(r"\bT " + name + r"\b", plug), name
    hpp = open(os.path.join(PLUGIN, "gpu_match_plugin.hpp")).read()
    for name in METHODS:
        assert re.search(r"pub fn " + name + r"\(", body), f"the Rust twin has no {name}"
        assert re.search(r"\b" + name + r"\(", hpp), f"the C++ twin has no {name}"
    # gpu_match_plugin.cpp stays linkable against a mock without the new export
    main = open(os.path.join(PLUGIN, "gpu_match_plugin.cpp")).read() + open(os.path.join(PLUGIN, "pm_plugin_c.cpp")).read()
    assert "pm_task_directory" not in main
    assert {"gpu_match_taskdir.cpp", "pm_plugin_taskdir_c.cpp"} <= set(B.PLUGIN_SOURCES)
    assert {"pm_taskdir.inc", "pm_engine_taskdir.inc"} <= set(B.HEADERS)
    assert re.search(r"#define PM_ABI_VERSION 3\b", hdr)


def test_the_struct_layouts_agree_in_c_numpy_and_rust():
    from protocol_amd import engine as E
    hdr = open(os.path.join(ROOT, "include", "pm_engine.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    rs = open(os.path.join(ROOT, "rust", "gpu_match_plugin.rs")).read()
    c_size = {"uint8_t": 1, "uint16_t": 2, "uint32_t": 4, "uint64_t": 8, "int64_t": 8}
    r_size = {"u8": 1, "u16": 2, "u32": 4, "u64": 8, "i64": 8}
    dims = {"PM_TS_N": 8, "PM_TKS_N": 3, "PM_TKR_N": 3}
    assert re.search(r"PM_TS_N = 8\b", plain) and re.search(r"PM_TKS_N = 3\b", plain) and re.search(r"PM_TKR_N = 3\b", plain)
    for name, dt, size in (("pm_tdir_query", E.tdir_query_dt, 40), ("pm_tdir_totals", E.tdir_totals_dt, 56),
                           ("pm_tdir_row", E.tdir_row_dt, 88)):
        body = plain[plain.index("typedef struct %s {" % name):plain.index("} %s;" % name)]
        c_fields = []                                       # (name, element size, elements)
        for t, decl in re.findall(r"(u?int\d+_t) ([^;]+);", body):
            for f in decl.split(","):
                m = re.match(r"\s*(\w+)(?:\[(\w+)\])?\s*$", f)
                c_fields.append((m.group(1), c_size[t], dims[m.group(2)] if m.group(2) else 1))
        at = rs.index("pub struct %s {" % name)
        assert "#[repr(C)]" in rs[rs.rindex("\n\n", 0, at):at], name
        r_fields = []
        for f, t in re.findall(r"pub (\w+): ([^,\n]+),", rs[at:rs.index("}", at)]):
            m = re.match(r"\[(u\d+); (\d+)\]$", t)
            r_fields.append((f, r_size[m.group(1)], int(m.group(2))) if m else (f, r_size[t], 1))
        np_fields = []
        for n in dt.names:
            sub = dt.fields[n][0]
            np_fields.append((n, sub.base.itemsize, int(sub.shape[0]) if sub.shape else 1))
        assert c_fields == np_fields == r_fields, (name, c_fields, np_fields, r_fields)
        # natural alignment without holes: every field sits at the sum of the sizes in front of it, on a multiple of its size
        offsets = [sum(s * k for _, s, k in np_fields[:i]) for i in range(len(np_fields))]
        assert [dt.fields[n][1] for n in dt.names] == offsets and all(o % s == 0 for o, (_, s, _) in zip(offsets, np_fields))
        assert dt.itemsize == size == sum(s * k for _, s, k in np_fields)
    assert E.tdir_row_dt.itemsize % 8 == 0
    assert E.tdir_row_dt.fields["created_at"][0] == "<i8" and re.search(r"pub created_at: i64,", rs) and "int64_t created_at;" in plain
    src = open(os.path.join(ROOT, "protocol_amd", "csrc", "pm_engine_taskdir.inc")).read()
    assert "static_assert(sizeof(pm_tdir_row) == 88" in src
    consts = dict(re.findall(r"pub const ((?:TDIR|TKS|TKR)_\w+): u32 = (\d+);", rs))
    for prefix, names in (("TDIR", ("BY_LIST", "BY_OLDEST", "BY_WORKERS_DESC", "BY_REPORTERS_DESC")),
                          ("TKS", ("RUNNING", "WAITING", "STARVED", "N")), ("TKR", ("UNHELD", "CONVERGED", "ROLLING", "N"))):
        for k, name in enumerate(names):
            full = prefix + "_" + name
            assert int(consts[full]) == k == getattr(E, full) and re.search(r"PM_%s = %d\b" % (full, k), plain), full
    assert int(consts["TKR_NONE"]) == 255 == E.TKR_NONE and re.search(r"#define PM_TKR_NONE 255u", plain)
