"""Node addresses for the address book (include/pm_engine.h "address book"): a seeded generator of 20-byte addresses in the
shapes that decide how the rank is computed, and the text-to-bytes parser.

make_swarm's digit-only addresses (swarm.py) stay what they are: every order agrees on them.  These are for the cases where
the EIP-55 text order, the byte order and the lower-case text order part ways."""
from __future__ import annotations

import numpy as np

VARIANTS = ("uniform", "letter_led", "prefix10", "prefix20", "prefix39", "duplicates")


def make_addresses(seed: int, n: int, variant: str = "uniform") -> np.ndarray:
    """n addresses as uint8 [n, 20], the same for the same (seed, n, variant).

    uniform      every byte uniform: the first ten characters tell any two apart (the rank's one-word sort)
    letter_led   both nibbles of the first byte from a-f: the text's first characters are letters, whose case the checksum
                 decides — where the EIP-55 order leaves the lower-case order most often
    prefix10 / prefix20 / prefix39
                 every address shares its first 10 / 20 / 39 nibbles with the others; the rest is uniform (prefix39: only the
                 last nibble differs, so there are at most 16 distinct addresses and many equal ones)
    duplicates   n // 2 + 1 uniform addresses, each row one of them: equal texts, which rank by ascending row"""
    if variant not in VARIANTS:
        raise ValueError(f"unknown variant {variant!r}")
    rng = np.random.default_rng([seed, VARIANTS.index(variant)])
    nib = rng.integers(0, 16, size=(n, 40), dtype=np.uint8)
    if variant == "letter_led":
        nib[:, :2] = rng.integers(10, 16, size=(n, 2), dtype=np.uint8)
    elif variant.startswith("prefix"):
        k = int(variant[6:])
        nib[:, :k] = rng.integers(0, 16, size=k, dtype=np.uint8)
    elif variant == "duplicates":
        nib = nib[rng.integers(0, n // 2 + 1, size=n)]
    return (nib[:, 0::2] << 4 | nib[:, 1::2]).astype(np.uint8)


def parse_address(text: str) -> bytes:
    """An address text — an optional "0x", then exactly 40 hex digits of either case — as its 20 bytes.  Anything else raises
    ValueError naming the text.  (The case is not checked against the checksum: `Address::from_str` accepts any.)"""
    body = text[2:] if text[:2] == "0x" else text
    if len(body) != 40 or any(c not in "0123456789abcdefABCDEF" for c in body):
        raise ValueError(f"not an address: {text!r}")
    return bytes.fromhex(body)
