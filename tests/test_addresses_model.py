"""The address book's CPU side: the Python sponge against hashlib (SHA3-256 shares everything with keccak-256 but the padding
byte), the EIP-55 known answers (the EIP's vectors, the reference's literals), the host helpers pm_host_keccak256 /
pm_host_eip55 against both, the address generator and parser, and the named cases' properties by the model."""
import hashlib
import json
import os

import numpy as np
import pytest

from protocol_amd import engine as E
from protocol_amd.addresses import VARIANTS, make_addresses, parse_address

import addresses_cases as AC
import addresses_model as M
import keccak_model as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "eip55_kats.json")))
LADDER = (0, 1, 135, 136, 137, 148, 271, 272, 273)


def _msg(n):
    return bytes((i * 7 + n) & 255 for i in range(n))


@pytest.mark.parametrize("n", LADDER)
def test_sponge_with_sha3_padding_is_hashlib(n):
    assert K.sha3_256(_msg(n)) == hashlib.sha3_256(_msg(n)).digest()


def test_keccak256_of_nothing():
    assert K.keccak256(b"").hex() == "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"
    assert K.keccak256(b"") != K.sha3_256(b"")


@pytest.mark.parametrize("n", LADDER)
def test_host_keccak_is_the_model(n):
    assert E.host_keccak256(_msg(n)) == K.keccak256(_msg(n))


def test_kat_file_is_data_only():
    assert set(KATS) == {"eip55", "reference_checksummed", "reference_not_a_checksum"}
    assert len(KATS["eip55"]) == 4 and len(KATS["reference_checksummed"]) == 26 and len(KATS["reference_not_a_checksum"]) == 5
    for t in sum(KATS.values(), []):
        assert isinstance(t, str) and len(t) == 42


@pytest.mark.parametrize("text", KATS["eip55"] + KATS["reference_checksummed"])
def test_eip55_known_answers(text):
    raw = bytes.fromhex(text[2:])
    assert M.eip55(raw) == text
    assert E.host_eip55(raw) == text
    assert parse_address(text) == raw and parse_address(text[2:].lower()) == raw


@pytest.mark.parametrize("text", KATS["reference_not_a_checksum"])
def test_hand_edited_literals_are_not_checksums(text):
    raw = bytes.fromhex(text[2:])
    assert not M.is_checksummed(text)
    assert E.host_eip55(raw) == M.eip55(raw) != text


def test_parser_refuses_what_is_no_address():
    good = "0x" + "aB" * 20
    assert parse_address(good) == bytes.fromhex("ab" * 20)
    for bad in ("", "0x", good[:-1], good + "0", "0X" + good[2:], good.replace("a", "g", 1), " " + good, good[2:] + "\n", "0x0x" + good[6:]):
        with pytest.raises(ValueError) as ei:
            parse_address(bad)
        assert repr(bad) in str(ei.value)


@pytest.mark.parametrize("variant", VARIANTS)
def test_generator_is_seeded_and_in_shape(variant):
    a = make_addresses(11, 200, variant)
    assert a.shape == (200, 20) and a.dtype == np.uint8
    assert np.array_equal(a, make_addresses(11, 200, variant))
    assert not np.array_equal(a, make_addresses(12, 200, variant))
    hexes = [r.tobytes().hex() for r in a]
    if variant == "letter_led":
        assert all(h[0] in "abcdef" and h[1] in "abcdef" for h in hexes)
    if variant.startswith("prefix"):
        k = int(variant[6:])
        assert len({h[:k] for h in hexes}) == 1 and len({h[:k + 1] for h in hexes}) > 1
    if variant == "duplicates":
        assert len(set(hexes)) < len(hexes)
    if variant == "uniform":
        assert len({h[:10] for h in hexes}) == len(hexes)
    assert make_addresses(1, 0, variant).shape == (0, 20)


def test_host_eip55_is_the_model_on_generated_addresses():
    for variant in VARIANTS:
        for r in make_addresses(21, 12, variant):
            assert E.host_eip55(r.tobytes()) == M.eip55(r.tobytes())


@pytest.mark.parametrize("name", sorted(AC.CASES))
def test_named_case_has_its_property(name):
    a = AC.CASES[name]()
    assert np.array_equal(a, AC.CASES[name]())
    texts = [M.eip55(r.tobytes()) for r in a]
    rank = M.ranks(a)
    assert sorted(rank) == list(range(len(a)))
    order = sorted(range(len(a)), key=lambda w: rank[w])
    for x, y in zip(order, order[1:]):  # ascending texts, equal ones by row
        assert (texts[x], x) < (texts[y], y)
    heads = [t[2:12] for t in texts]
    assert (len(set(heads)) < len(heads)) == (name in AC.DEEP)
    if name == "nine_B_a":
        for k in range(0, len(a), 3):
            assert [t[2] for t in texts[k:k + 3]] == ["a", "B", "9"]
            assert rank[k + 2] < rank[k + 1] < rank[k]
        low = M.ranks_lowercase(a)
        assert low != rank and all(low[k + 2] < low[k] < low[k + 1] for k in range(0, len(a), 3))
    if name == "last_nibble_pairs":
        assert all(texts[k][:41].lower() == texts[k + 1][:41].lower() and texts[k][41].lower() > texts[k + 1][41].lower() for k in range(0, len(a), 2))
    if name == "digits_only":
        assert rank == M.ranks_lowercase(a) and all(t[2:].isdigit() for t in texts)
    if name in ("duplicates", "all_equal"):
        seen = {}
        for w, t in enumerate(texts):
            if t in seen:
                assert rank[seen[t]] < rank[w]
            seen[t] = w
        assert len(seen) < len(texts)


def test_invite_digest_layout():
    """the 148 bytes and the EIP-191 prefix, spelled out once by hand"""
    addr, nonce = bytes(range(1, 21)), bytes(range(100, 132))
    msg = b"\0" * 31 + b"\x07" + b"\0" * 30 + b"\x01\x02" + addr + nonce + b"\0" * 24 + (1_700_000_000).to_bytes(8, "big")
    d = M.invite_digest(7, 0x0102, addr, nonce, 1_700_000_000)
    assert d == K.keccak256(msg) == E.host_keccak256(msg)
    assert M.signing_hash(d) == K.keccak256(b"\x19Ethereum Signed Message:\n32" + d)


def test_numbered_exports_are_in_the_library():
    """test_host_helpers' check of the header against EXPORTS takes names of letters and '_' only; this is the same check, both ways,
    for the declared names that carry a digit: the header's are exactly EXPORTS_NUMBERED, the library has each, none is in EXPORTS"""
    import re
    L = E.lib()
    hdr = open(os.path.join(ROOT, "include", "pm_engine.h")).read()
    every = set(re.findall(r"\b(pm_[a-z_0-9]+)\s*\(", hdr))
    plain = set(re.findall(r"\b(pm_[a-z_]+)\s*\(", hdr))
    assert {n for n in every - plain if re.search(r"\d", n)} == set(E.EXPORTS_NUMBERED) and len(set(E.EXPORTS_NUMBERED)) == 3
    assert not set(E.EXPORTS_NUMBERED) & set(E.EXPORTS)
    for name in E.EXPORTS_NUMBERED:
        assert hasattr(L, name), f"{name} declared in pm_engine.h but not exported"
