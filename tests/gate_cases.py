"""Named inputs of the request gate's recovery (pm_ecrecover_many, pm_host_ecrecover), each a (hash32, sig65) pair built the
same way every time, and what tests/secp256k1_model.py says of it.  What a case is for stands beside it;
test_secp256k1_model.py asserts by the model that it has the property it is named after.  Built once per process."""
import functools
import hashlib

import secp256k1_model as M

KEY = 0x1F2E3D4C5B6A79880796A5B4C3D2E1F00112233445566778899AABBCCDDEEFF1
N, G = M.N, M.G


def _z(tag: str) -> bytes:
    return hashlib.sha256(tag.encode()).digest()


def _crafted(k: int, u1: int, u2: int):
    """the entry whose recovery is u1 G + u2 R with R = k G: r = x(R), s = u2 r, z = -u1 r (mod n)"""
    R = M.mul(k, G)
    r = R[0] % N
    s, z = u2 * r % N, (-u1) * r % N
    assert r == R[0] and s
    return z.to_bytes(32, "big"), M.sig65(r, s, R[1] & 1)


def _not_an_x(start: int) -> int:
    r = start
    while M.lift_x(r, 0) is not None:
        r += 1
    return r


@functools.lru_cache(maxsize=None)
def named():
    """{name: (hash32, sig65)}"""
    out = {}
    z = _z("low and high s")
    r, s, p = M.sign(KEY, z)
    out["low_s"] = (z, M.sig65(r, s, p))
    out["high_s"] = (z, M.sig65(r, N - s, p ^ 1))            # the same key as low_s
    out["high_s_parity_kept"] = (z, M.sig65(r, N - s, p))    # a key, but another one
    for v in (0, 1, 27, 28):                                 # v = p and 27 + p recover KEY's address, the other two another key
        out[f"v_{v}"] = (z, M.sig65(r, s, v))
    for v in (2, 26, 29, 35):
        out[f"v_{v}"] = (z, M.sig65(r, s, v))                # not ok
    out["r_zero"] = (z, M.sig65(0, s, p))
    out["s_zero"] = (z, M.sig65(r, 0, p))
    out["r_is_n"] = (z, M.sig65(N, s, p))
    out["s_is_n"] = (z, M.sig65(r, N, p))
    out["r_no_x"] = (z, M.sig65(_not_an_x(r + 1), s, p))
    # an r for which r + n < p is an x coordinate but r is not: a recovery that tried r + n would find a key
    small = 1
    while not (M.lift_x(small, 0) is None and M.lift_x(small + N, 0) is not None):
        small += 1
    out["r_plus_n_is_x"] = (z, M.sig65(small, s, p))
    z0 = bytes(32)
    out["z_zero"] = (z0, M.sig65(*M.sign(KEY, z0)))
    zn = (N + 5).to_bytes(32, "big")
    out["z_above_n"] = (zn, M.sig65(*M.sign(KEY, zn)))
    zf = b"\xff" * 32
    out["z_all_ones"] = (zf, M.sig65(*M.sign(KEY, zf)))
    z1 = _z("k = 1")
    out["k_one"] = (z1, M.sig65(*M.sign(KEY, z1, k=1, low_s=False)))        # R = G: the table's third entry is 2 G
    out["k_n_minus_one"] = (z1, M.sig65(*M.sign(KEY, z1, k=N - 1, low_s=False)))  # R = -G: the third entry is infinity
    # s R and -z G are the same point: a recovery that adds two products adds equal points at the end
    k, s2 = 0x1234567, 0xABCDEF0123456789
    R = M.mul(k, G)
    out["final_add_equal"] = (((-s2 * k) % N).to_bytes(32, "big"), M.sig65(R[0], s2, R[1] & 1))
    out["q_infinity"] = ((s2 * k % N).to_bytes(32, "big"), M.sig65(R[0], s2, R[1] & 1))  # s R = z G: no key
    # the interleaved ladder's own exceptions: with R = 2 G, bits (1, 0) then (0, 1) add 2 G to 2 G; with R = -2 G they add
    # -2 G to 2 G and the ladder goes on from infinity; with R = G, bits (1, 0) then (1, 1) add the entry G + R to 2 G
    low1, low2 = 0x5A5A5A5A5A5A5A5A1234, 0x0F0F0F0F0F0F0F0F4321
    out["ladder_equal"] = _crafted(2, (1 << 200) | low1, (1 << 199) | low2)
    out["ladder_opposite"] = _crafted(N - 2, (1 << 200) | low1, (1 << 199) | low2)
    out["ladder_equal_sum_entry"] = _crafted(1, (3 << 199) | low1, (1 << 199) | low2)
    out["ladder_top_bits"] = _crafted(2, (1 << 255) | low1, (1 << 254) | low2)
    out["sum_entry_infinity"] = _crafted(N - 1, (7 << 100) | low1, (5 << 100) | low2)
    out["u1_zero"] = _crafted(0x77, 0, low2)                 # z = 0 by construction: Q = u2 R alone
    return out


OK_AS_KEY = ("low_s", "high_s", "z_zero", "z_above_n", "z_all_ones", "k_one", "k_n_minus_one")  # recover KEY's address
NOT_OK = ("v_2", "v_26", "v_29", "v_35", "r_zero", "s_zero", "r_is_n", "s_is_n", "r_no_x", "r_plus_n_is_x", "q_infinity")


@functools.lru_cache(maxsize=None)
def signed(count: int = 12):
    """`count` ordinary signatures by different keys: [(key, hash32, sig65)]"""
    out = []
    for i in range(count):
        key = int.from_bytes(hashlib.sha256(b"gate key %d" % i).digest(), "big") % (N - 1) + 1
        z = _z("gate message %d" % i)
        out.append((key, z, M.sig65(*M.sign(key, z))))
    return out


@functools.lru_cache(maxsize=None)
def expected(z: bytes, sig: bytes):
    """the model's (ok, address20, pub64), remembered per entry"""
    return M.ecrecover(z, sig)


def batch(n: int):
    """n entries: every named case first (as far as n goes), then the ordinary signatures in turn with every fifth one spoilt
    (a flipped bit in s: another key; in r: mostly no key)"""
    pool = list(named().values())
    ordinary = signed()
    out = []
    for i in range(n):
        if i < len(pool):
            out.append(pool[i])
            continue
        _key, z, sig = ordinary[i % len(ordinary)]
        if i % 5 == 3:
            b = bytearray(sig)
            b[(17 if i % 2 else 45)] ^= 1 << (i % 7)
            sig = bytes(b)
        out.append((z, sig))
    return out
