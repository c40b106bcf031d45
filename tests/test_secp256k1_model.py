"""The request gate's CPU side: tests/secp256k1_model.py held to known answers (tests/golden/secp256k1_kats.json), the named
cases of tests/gate_cases.py held to the properties they are named after, and pm_host_ecrecover — the engine library's plain
C++ recovery — against the model on every named case and a mixed batch."""
import json
import os

import pytest

from protocol_amd import engine as E
from protocol_amd import gate as G

import gate_cases as GC
import keccak_model as K
import secp256k1_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "secp256k1_kats.json")))


def test_curve_constants():
    assert (M.GY * M.GY - M.GX ** 3 - 7) % M.P == 0
    assert M.mul(M.N, M.G) is M.INF and M.mul(M.N - 1, M.G) == M.neg(M.G)
    two = M.add(M.G, M.G)
    assert "%064x" % two[0] == KATS["two_g"]["x"] and "%064x" % two[1] == KATS["two_g"]["y"]
    assert M.add(M.G, M.neg(M.G)) is M.INF and M.add(M.INF, M.G) == M.G == M.add(M.G, M.INF)


def test_key_one_address():
    assert M.address_of_key(1).hex() == KATS["key_one_address"]


def test_rfc6979_known_answer():
    k = KATS["rfc6979"]
    import hashlib
    z = hashlib.sha256(k["message"].encode()).digest()
    assert z.hex() == k["z"]
    r, s, parity = M.sign(k["key"], z)
    assert ("%064x" % r, "%064x" % s, parity) == (k["r"], k["s"], k["parity"])
    assert M.address_of(M.recover(z, r, s, parity)).hex() == KATS["key_one_address"]


def test_heartbeat_known_answer():
    k = KATS["heartbeat"]
    h = M.eip191(k["message"].encode())
    assert h.hex() == k["hash"]
    assert h == K.keccak256(b"\x19Ethereum Signed Message:\n%d" % len(k["message"]) + k["message"].encode())
    r, s, parity = M.sign(k["key"], h)
    assert ("%064x" % r, "%064x" % s, parity) == (k["r"], k["s"], k["parity"])
    assert k["r"].startswith("de8c0e6a") and k["r"].endswith("7bd28c83") and k["s"].startswith("34552d58") and k["s"].endswith("daefd0d0")
    ok, addr, _pub = M.ecrecover(h, M.sig65(r, s, parity))
    assert ok == 1 and addr.hex() == k["address"] == KATS["key_one_address"]
    assert E.host_ecrecover(h, M.sig65(r, s, parity)).hex() == k["address"]


def test_named_cases_have_their_properties():
    named = GC.named()
    mine = M.address_of_key(GC.KEY)
    for name in GC.OK_AS_KEY:
        ok, addr, _ = GC.expected(*named[name])
        assert ok == 1 and addr == mine, name
    for name in GC.NOT_OK:
        assert GC.expected(*named[name]) == (0, bytes(20), bytes(64)), name
    # v = the parity and 27 + the parity recover the key; the other two recover another key
    p = named["low_s"][1][64]
    for v in (0, 1, 27, 28):
        ok, addr, _ = GC.expected(*named[f"v_{v}"])
        assert ok == 1 and (addr == mine) == (M.parity_of_v(v) == p), v
    ok, addr, _ = GC.expected(*named["high_s_parity_kept"])
    assert ok == 1 and addr != mine
    s_low, s_high = (int.from_bytes(named[n][1][32:64], "big") for n in ("low_s", "high_s"))
    assert s_low <= M.N // 2 < s_high and s_low + s_high == M.N and named["low_s"][1][64] ^ named["high_s"][1][64] == 1
    # r + n is an x coordinate below p, r is none
    r = int.from_bytes(named["r_plus_n_is_x"][1][:32], "big")
    assert M.lift_x(r, 0) is None and M.lift_x(r + M.N, 0) is not None and r + M.N < M.P
    assert int.from_bytes(named["z_above_n"][0], "big") >= M.N and named["z_zero"][0] == bytes(32)
    for name, k in (("k_one", 1), ("k_n_minus_one", M.N - 1)):
        assert int.from_bytes(named[name][1][:32], "big") == M.GX and named[name][1][64] == (M.mul(k, M.G)[1] & 1)
    # the two products of the final addition are the same point / opposite points
    for name, same in (("final_add_equal", True), ("q_infinity", False)):
        z, sig = named[name]
        r, s = int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:64], "big")
        ri = pow(r, -1, M.N)
        a = M.mul(s * ri % M.N, M.lift_x(r, sig[64]))
        b = M.mul(-int.from_bytes(z, "big") * ri % M.N, M.G)
        assert (a == b) if same else (a == M.neg(b)), name
    for name in ("ladder_equal", "ladder_opposite", "ladder_equal_sum_entry", "ladder_top_bits", "sum_entry_infinity", "u1_zero"):
        assert GC.expected(*named[name])[0] == 1, name


@pytest.mark.parametrize("name", sorted(GC.named()))
def test_host_ecrecover_on_the_named_cases(name):
    z, sig = GC.named()[name]
    ok, addr, _ = GC.expected(z, sig)
    assert E.host_ecrecover(z, sig) == (addr if ok else None)


def test_host_ecrecover_on_a_mixed_batch():
    seen = 0
    for z, sig in GC.batch(65):
        ok, addr, _ = GC.expected(z, sig)
        assert E.host_ecrecover(z, sig) == (addr if ok else None)
        seen += ok
    assert 20 <= seen <= 60  # (both answers are well represented)
    assert E.lib().pm_host_ecrecover(None, None, None) == E.PM_EINVAL


def test_packing_helpers():
    good = "0x" + "ab" * 65
    assert G.parse_signature(good) == G.parse_signature(good[2:]) == b"\xab" * 65
    for bad in ("", "0x", good[:-1], good + "0", "0X" + good[2:], good[:9] + "g" + good[10:]):
        assert G.parse_signature(bad) is None
    buf, off, sigs, claimed, flags = G.pack_requests([(b"abc", good, "0x" + "11" * 20), (b"", b"\x01" * 65, b"\x22" * 20),
                                                      (b"defgh", "nonsense", "0x12")])
    assert buf.tobytes() == b"abcdefgh" and off.tolist() == [0, 3, 3, 8]
    assert sigs[0].tobytes() == b"\xab" * 65 and sigs[1].tobytes() == b"\x01" * 65 and sigs[2].tobytes() == b"\xff" * 65
    assert claimed[0].tobytes() == b"\x11" * 20 and claimed[1].tobytes() == b"\x22" * 20 and claimed[2].tobytes() == bytes(20)
    assert flags.tolist() == [0, 0, 1]
