"""A plain big-integer model of what the request gate computes (pm_ecrecover_many / pm_verify_requests of include/pm_engine.h):
secp256k1 in affine coordinates with Python integers, signing (RFC 6979, or an explicit k), recovery by the rules the header
states, the Ethereum address of a key, and the EIP-191 hash.  It shares nothing with the engine's limb arithmetic but the
curve's constants; the keccak is tests/keccak_model.py.  About 30-40 ms per sign + recover: make fixtures once per module."""
import hashlib
import hmac

import keccak_model as K

P = 2**256 - 2**32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
GX = 0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798
GY = 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8
G = (GX, GY)
INF = None  # the point at infinity


def add(a, b):
    """affine addition with every exceptional case"""
    if a is INF:
        return b
    if b is INF:
        return a
    if a[0] == b[0]:
        if (a[1] + b[1]) % P == 0:
            return INF
        lam = 3 * a[0] * a[0] * pow(2 * a[1], -1, P) % P
    else:
        lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, P) % P
    x = (lam * lam - a[0] - b[0]) % P
    return (x, (lam * (a[0] - x) - a[1]) % P)


def neg(a):
    return INF if a is INF else (a[0], (-a[1]) % P)


def mul(k, a):
    out = INF
    while k:
        if k & 1:
            out = add(out, a)
        a = add(a, a)
        k >>= 1
    return out


def lift_x(x, parity):
    """the point with this x and this parity of y, or None when x^3 + 7 is no square (or x is no field element)"""
    if x >= P:
        return None
    c = (x * x * x + 7) % P
    y = pow(c, (P + 1) // 4, P)
    if y * y % P != c:
        return None
    return (x, y if (y & 1) == parity else P - y)


def rfc6979_k(key: int, z32: bytes) -> int:
    x = key.to_bytes(32, "big")
    h1 = (int.from_bytes(z32, "big") % N).to_bytes(32, "big")
    v, k = b"\x01" * 32, b"\x00" * 32
    k = hmac.new(k, v + b"\x00" + x + h1, hashlib.sha256).digest()
    v = hmac.new(k, v, hashlib.sha256).digest()
    k = hmac.new(k, v + b"\x01" + x + h1, hashlib.sha256).digest()
    v = hmac.new(k, v, hashlib.sha256).digest()
    while True:
        v = hmac.new(k, v, hashlib.sha256).digest()
        cand = int.from_bytes(v, "big")
        if 1 <= cand < N:
            return cand
        k = hmac.new(k, v + b"\x00", hashlib.sha256).digest()
        v = hmac.new(k, v, hashlib.sha256).digest()


def sign(key: int, z32: bytes, k: int = None, low_s: bool = True):
    """(r, s, parity) of the 32-byte hash under `key`; k: the nonce (default RFC 6979); low_s: normalise s to the lower half,
    flipping the parity, as k256 does when it signs"""
    z = int.from_bytes(z32, "big") % N
    if k is None:
        k = rfc6979_k(key, z32)
    R = mul(k, G)
    r = R[0] % N
    s = pow(k, -1, N) * (z + r * key) % N
    parity = R[1] & 1
    assert r and s and R[0] < N, "a nonce the test cannot use"
    if low_s and s > N // 2:
        s, parity = N - s, parity ^ 1
    return r, s, parity


def recover(z32: bytes, r: int, s: int, parity: int):
    """the public key (x, y), or None: 1 <= r, s < n; R's x is r itself (never r + n) and its y has the given parity; any s of
    the range is taken (a high s recovers what (r, n - s, parity ^ 1) recovers); z is the hash mod n"""
    if not (1 <= r < N and 1 <= s < N):
        return None
    R = lift_x(r, parity)
    if R is None:
        return None
    z = int.from_bytes(z32, "big") % N
    ri = pow(r, -1, N)
    Q = add(mul(s * ri % N, R), mul((-z) * ri % N, G))
    return Q  # (None: the point at infinity is no key)


def address_of(Q) -> bytes:
    return K.keccak256(Q[0].to_bytes(32, "big") + Q[1].to_bytes(32, "big"))[12:]


def address_of_key(key: int) -> bytes:
    return address_of(mul(key, G))


def parity_of_v(v: int):
    """0 / 27 even, 1 / 28 odd, anything else None"""
    return {0: 0, 27: 0, 1: 1, 28: 1}.get(v)


def sig65(r: int, s: int, v: int) -> bytes:
    return r.to_bytes(32, "big") + s.to_bytes(32, "big") + bytes([v])


def ecrecover(z32: bytes, sig: bytes):
    """what pm_ecrecover_many answers for one entry: (ok, address20, pub64)"""
    parity = parity_of_v(sig[64])
    Q = None if parity is None else recover(z32, int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:64], "big"), parity)
    if Q is None:
        return 0, bytes(20), bytes(64)
    return 1, address_of(Q), Q[0].to_bytes(32, "big") + Q[1].to_bytes(32, "big")


def eip191(msg: bytes) -> bytes:
    return K.keccak256(b"\x19Ethereum Signed Message:\n" + str(len(msg)).encode() + msg)
