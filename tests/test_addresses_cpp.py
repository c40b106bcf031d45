"""The address book's plugin side without a GPU: GpuMatchPlugin with the book on and its C face against a mock
(tests/cpp/addresses_test.cpp + tests/cpp/mock_addresses.cpp, a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer: the parser and its errors, what sync_nodes sends, the text cache, the invite digests, digit-only
addresses with the book on and off), and the new names agreeing across the header, protocol_amd.engine, the Rust twin's extern
block and both libraries' dynamic symbol tables."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = [os.path.join(ROOT, "include"), os.path.join(ROOT, "protocol_amd", "plugin"), os.path.join(ROOT, "protocol_amd", "csrc")]
PLUGIN = os.path.join(ROOT, "protocol_amd", "plugin")
SRC = [os.path.join(ROOT, "tests", "cpp", f) for f in ("addresses_test.cpp", "mock_addresses.cpp", "mock_directory.cpp", "mock_engine.cpp")] + \
      [os.path.join(PLUGIN, f) for f in ("gpu_match_plugin.cpp", "gpu_match_addresses.cpp", "gpu_match_directory.cpp", "pm_plugin_c.cpp",
                                         "pm_plugin_addresses_c.cpp")] + \
      [os.path.join(ROOT, "protocol_amd", "csrc", "pm_host.cpp")]
ENGINE = {"pm_addresses_enable": 2, "pm_addresses_set": 4, "pm_addresses_rank": 2, "pm_addresses_text": 4, "pm_keccak256_many": 5,
          "pm_invite_digests": 9}
PMX = ["pmx_enable_address_book", "pmx_invite_digests"]
METHODS = ("enable_address_book", "invite_digests")


def test_the_address_book_twin_against_the_mock_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "addresses_test")
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
    for name, arity in ENGINE.items():
        h = re.search(r"int32_t " + name + r"\(([^;]*)\);", plain)
        r = re.search(r"fn " + name + r"\(([^;]*)\) -> i32;", ext)
        assert h and r and _arity(h.group(1)) == _arity(r.group(1)) == arity, name
        assert name in E.EXPORTS + E.EXPORTS_NUMBERED
        assert re.search(r"\bT " + name + r"\b", eng), f"libpm_engine.so does not define {name}"
    for name in ("pm_addresses_enable", "pm_addresses_set", "pm_addresses_rank", "pm_addresses_text", "pm_invite_digests"):
        assert re.search(r"\b" + name + r"\s*\(", body), f"the Rust plugin body does not call {name}"
        assert re.search(r"\bU " + name + r"\b", plug), f"libpm_plugin.so does not import {name}"
    for name in ("pm_host_keccak256", "pm_host_eip55"):
        assert re.search(r"int32_t " + name + r"\(", plain) and re.search(r"\bT " + name + r"\b", eng) and name in E.EXPORTS_NUMBERED
    pmx = open(os.path.join(PLUGIN, "pm_plugin_c.h")).read()
    for name in PMX:
        assert re.search(r"int32_t " + name + r"\(", pmx) and re.search(r"\bT " + name + r"\b", plug), name
    hpp = open(os.path.join(PLUGIN, "gpu_match_plugin.hpp")).read()
    for name in METHODS:
        assert re.search(r"pub fn " + name + r"\(", body), f"the Rust twin has no {name}"
        assert re.search(r"\b" + name + r"\(", hpp), f"the C++ twin has no {name}"
    # gpu_match_plugin.cpp stays linkable against a mock without the new exports
    main = open(os.path.join(PLUGIN, "gpu_match_plugin.cpp")).read() + open(os.path.join(PLUGIN, "pm_plugin_c.cpp")).read()
    assert not re.search(r"\bpm_(addresses_\w+|invite_digests|keccak256_many)\s*\(", main)
    assert {"gpu_match_addresses.cpp", "pm_plugin_addresses_c.cpp"} <= set(B.PLUGIN_SOURCES)
    assert {"pm_keccak.inc", "pm_addresses.inc", "pm_engine_addresses.inc"} <= set(B.HEADERS)
    assert re.search(r"#define PM_ABI_VERSION 3\b", hdr)


def test_python_parser_is_the_plugins():
    """protocol_amd.addresses.parse_address and GpuMatchPlugin::parse_address_text are written twice: the same texts, the same answers
    (the C++ side's are checked in addresses_test.cpp's first test; the lists are kept alike by hand)"""
    from protocol_amd.addresses import parse_address
    good = "0xfB6916095ca1df60bB79Ce92cE3Ea74c37c5d359"
    for bad in ("", "0x", good[:41], good + "0", "0X" + good[2:], " " + good, good[:10] + "g" + good[11:], good[2:] + "\n", "0x0x" + good[6:]):
        with pytest.raises(ValueError):
            parse_address(bad)
    assert parse_address(good) == parse_address(good[2:].lower()) == parse_address("0x" + good[2:].upper())
