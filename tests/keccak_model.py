"""A plain Python Keccak sponge (rate 136, 32 bytes out) with the padding byte as a parameter: 0x06 is SHA3-256, which
hashlib has, and 0x01 is the keccak-256 Ethereum uses, which it has not.  test_addresses_model.py holds the first to hashlib —
that pins the permutation and the absorb loop — and everything else to the second."""

RATE = 136
MASK = (1 << 64) - 1
ROT = [[0, 36, 3, 41, 18], [1, 44, 10, 45, 2], [62, 6, 43, 15, 61], [28, 55, 25, 21, 56], [27, 20, 39, 8, 14]]  # [x][y]


def _round_constants():
    out, r = [], 1
    for _ in range(24):
        rc = 0
        for j in range(7):
            r = ((r << 1) ^ ((r >> 7) * 0x71)) & 0xFF
            if r & 2:
                rc ^= 1 << ((1 << j) - 1)
        out.append(rc)
    return out


RC = _round_constants()


def _rotl(v, n):
    return ((v << n) | (v >> (64 - n))) & MASK if n else v


def keccak_f1600(a):
    """a[x][y], in place"""
    for rc in RC:
        c = [a[x][0] ^ a[x][1] ^ a[x][2] ^ a[x][3] ^ a[x][4] for x in range(5)]
        d = [c[(x + 4) % 5] ^ _rotl(c[(x + 1) % 5], 1) for x in range(5)]
        for x in range(5):
            for y in range(5):
                a[x][y] ^= d[x]
        b = [[0] * 5 for _ in range(5)]
        for x in range(5):
            for y in range(5):
                b[y][(2 * x + 3 * y) % 5] = _rotl(a[x][y], ROT[x][y])
        for x in range(5):
            for y in range(5):
                a[x][y] = b[x][y] ^ (~b[(x + 1) % 5][y] & MASK & b[(x + 2) % 5][y])
        a[0][0] ^= rc


def sponge256(data: bytes, pad: int) -> bytes:
    data = bytes(data)
    tail = len(data) % RATE
    block = bytearray(RATE - tail)
    block[0] ^= pad
    block[-1] ^= 0x80
    padded = data + bytes(block)
    a = [[0] * 5 for _ in range(5)]
    for at in range(0, len(padded), RATE):
        for i in range(RATE // 8):
            a[i % 5][i // 5] ^= int.from_bytes(padded[at + 8 * i:at + 8 * i + 8], "little")
        keccak_f1600(a)
    return b"".join(a[i % 5][i // 5].to_bytes(8, "little") for i in range(4))


def keccak256(data: bytes) -> bytes:
    return sponge256(data, 0x01)


def sha3_256(data: bytes) -> bytes:
    return sponge256(data, 0x06)
