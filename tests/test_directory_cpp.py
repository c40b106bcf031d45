"""The node directory's plugin side without a GPU: GpuMatchPlugin's directory methods and their C face against a mock
(tests/cpp/directory_test.cpp + tests/cpp/mock_directory.cpp, a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer: the queries each method sends, the listing with its counts and group objects, the gauge, the two
status lists, paging, a row without an address, the texts and their sizing), and the new names agreeing across the header,
protocol_amd.engine.EXPORTS, the Rust twin's extern block, both libraries' dynamic symbol tables and the struct layouts."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = [os.path.join(ROOT, "include"), os.path.join(ROOT, "protocol_amd", "plugin"), os.path.join(ROOT, "protocol_amd", "csrc")]
PLUGIN = os.path.join(ROOT, "protocol_amd", "plugin")
SRC = [os.path.join(ROOT, "tests", "cpp", f) for f in ("directory_test.cpp", "mock_directory.cpp", "mock_engine.cpp")] + \
      [os.path.join(PLUGIN, f) for f in ("gpu_match_plugin.cpp", "gpu_match_directory.cpp", "pm_plugin_c.cpp", "pm_plugin_directory_c.cpp")] + \
      [os.path.join(ROOT, "protocol_amd", "csrc", "pm_host.cpp")]
PMX = ["pmx_list_nodes", "pmx_status_counts", "pmx_uninvited_nodes", "pmx_dead_nodes"]


def test_the_directory_twin_against_the_mock_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "directory_test")
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
    h = re.search(r"int32_t pm_directory\(([^;]*)\);", plain)
    r = re.search(r"fn pm_directory\(([^;]*)\) -> i32;", ext)
    assert h and r and _arity(h.group(1)) == _arity(r.group(1)) == 7
    assert "pm_directory" in E.EXPORTS and re.search(r"\bpm_directory\s*\(", body), "the Rust plugin body does not call pm_directory"
    assert re.search(r"\bT pm_directory\b", eng), "libpm_engine.so does not define pm_directory"
    assert re.search(r"\bU pm_directory\b", plug), "libpm_plugin.so does not import pm_directory"
    pmx = open(os.path.join(PLUGIN, "pm_plugin_c.h")).read()
    for name in PMX:
        assert re.search(r"int32_t " + name + r"\(", pmx) and re.search(r"\bT " + name + r"\b", plug), name
    for name in ("list_nodes", "status_counts", "uninvited_nodes", "dead_nodes"):
        assert re.search(r"pub fn " + name + r"\(", body), f"the Rust twin has no {name}"
    # gpu_match_plugin.cpp stays linkable against a mock without the new export
    main = open(os.path.join(PLUGIN, "gpu_match_plugin.cpp")).read() + open(os.path.join(PLUGIN, "pm_plugin_c.cpp")).read()
    assert "pm_directory" not in main
    assert {"gpu_match_directory.cpp", "pm_plugin_directory_c.cpp"} <= set(B.PLUGIN_SOURCES)
    assert {"pm_directory.inc", "pm_engine_directory.inc"} <= set(B.HEADERS)
    assert re.search(r"#define PM_ABI_VERSION 3\b", hdr)


def test_the_struct_layouts_agree_in_c_numpy_and_rust():
    from protocol_amd import engine as E
    hdr = open(os.path.join(ROOT, "include", "pm_engine.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    rs = open(os.path.join(ROOT, "rust", "gpu_match_plugin.rs")).read()
    c_size = {"uint8_t": 1, "uint16_t": 2, "uint32_t": 4, "uint64_t": 8}
    r_size = {"u8": 1, "u16": 2, "u32": 4, "u64": 8}
    for name, dt in (("pm_dir_query", E.dir_query_dt), ("pm_dir_row", E.dir_row_dt)):
        body = plain[plain.index("typedef struct %s {" % name):plain.index("} %s;" % name)]
        c_fields = []
        for t, decl in re.findall(r"(uint\d+_t) ([^;]+);", body):
            for f in decl.split(","):
                c_fields.append((f.strip(), c_size[t]))
        at = rs.index("pub struct %s {" % name)
        assert "#[repr(C)]" in rs[rs.rindex("\n\n", 0, at):at], name
        r_fields = [(f, r_size[t]) for f, t in re.findall(r"pub (\w+): (u\d+),", rs[at:rs.index("}", at)])]
        np_fields = [(n, dt.fields[n][0].itemsize) for n in dt.names]
        assert c_fields == np_fields == r_fields, (name, c_fields, np_fields, r_fields)
        # natural alignment without holes: every field sits at the sum of the sizes in front of it
        assert [dt.fields[n][1] for n in dt.names] == [sum(s for _, s in np_fields[:k]) for k in range(len(np_fields))]
    consts = dict(re.findall(r"pub const ((?:DIR|DC|NS)_\w+): (?:u32|usize) = (\d+);", rs))
    for k, name in enumerate(("ANY", "GROUPED", "UNGROUPED")):
        assert int(consts["DIR_" + name]) == k == getattr(E, "DIR_" + name) and re.search(r"PM_DIR_%s = %d\b" % (name, k), plain)
    for k, name in enumerate(("BY_ROW", "BY_ADDRESS")):
        assert int(consts["DIR_" + name]) == k == getattr(E, "DIR_" + name) and re.search(r"PM_DIR_%s = %d\b" % (name, k), plain)
    for k, name in enumerate(("HEALTHY", "DISCOVERED", "OTHER", "DEAD", "N")):
        assert int(consts["DC_" + name]) == k == getattr(E, "DC_" + name) and re.search(r"PM_DC_%s = %d\b" % (name, k), plain)
