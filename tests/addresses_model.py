"""The address book's model: EIP-55 texts, their ranks, the invite digest and its signing hash, in plain Python over
tests/keccak_model.py."""
from keccak_model import keccak256


def eip55(addr20: bytes) -> str:
    """`Address: Display`: "0x" + the hex text, letter i upper-case where nibble i of keccak-256(lower-case text) >= 8"""
    low = bytes(addr20).hex()
    h = keccak256(low.encode("ascii")).hex()
    return "0x" + "".join(c.upper() if c in "abcdef" and int(h[i], 16) >= 8 else c for i, c in enumerate(low))


def is_checksummed(text: str) -> bool:
    return text.startswith("0x") and len(text) == 42 and eip55(bytes.fromhex(text[2:])) == text


def ranks_of_texts(texts) -> list:
    """a row's place in the texts sorted as byte strings, equal texts by ascending row: a permutation"""
    order = sorted(range(len(texts)), key=lambda w: (texts[w].encode("ascii"), w))
    rank = [0] * len(texts)
    for pos, w in enumerate(order):
        rank[w] = pos
    return rank


def ranks(addrs) -> list:
    return ranks_of_texts([eip55(bytes(a)) for a in addrs])


def ranks_lowercase(addrs) -> list:
    """what a host gets that sorts the lower-case texts (the order of the bytes)"""
    return ranks_of_texts(["0x" + bytes(a).hex() for a in addrs])


def invite_digest(domain_id: int, pool_id: int, addr20: bytes, nonce32: bytes, expiration_s: int) -> bytes:
    """NodeInviter::generate_invite's keccak: U256 big-endian domain and pool, the address, the nonce, U256 big-endian seconds"""
    assert len(addr20) == 20 and len(nonce32) == 32
    msg = domain_id.to_bytes(32, "big") + pool_id.to_bytes(32, "big") + bytes(addr20) + bytes(nonce32) + expiration_s.to_bytes(32, "big")
    assert len(msg) == 148
    return keccak256(msg)


def signing_hash(digest32: bytes) -> bytes:
    """what sign_message hashes (EIP-191)"""
    return keccak256(b"\x19Ethereum Signed Message:\n32" + bytes(digest32))
