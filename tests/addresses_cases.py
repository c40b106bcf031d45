"""Named address lists for the address book's tests (CPU model, GPU): each is uint8 [n, 20], built the same way every time.
What a case is for stands beside it; test_addresses_model.py asserts by the model that it has the property it is named after."""
import numpy as np

from protocol_amd.addresses import make_addresses

import addresses_model as M


def _find(rng, want):
    """the first drawn address whose EIP-55 text satisfies `want`"""
    while True:
        a = rng.integers(0, 256, size=20, dtype=np.uint8)
        if want(a, M.eip55(a.tobytes())):
            return a


def nine_B_a(seed: int = 5, triples: int = 4) -> np.ndarray:
    """rows (3 k, 3 k + 1, 3 k + 2): texts that begin 'a' (a letter the checksum leaves lower), 'B' (one it raises), '9' — as
    bytes and as lower-case text they order 9 < a < b, as EIP-55 text '9' < 'B' < 'a'"""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(triples):
        rows.append(_find(rng, lambda a, t: t[2] == "a"))
        rows.append(_find(rng, lambda a, t: t[2] == "B"))
        rows.append(_find(rng, lambda a, t: t[2] == "9"))
    return np.stack(rows)


def last_nibble_pairs(seed: int = 6, pairs: int = 8) -> np.ndarray:
    """rows (2 k, 2 k + 1) differ in the last nibble alone, the higher one first: only the key's last word tells them apart"""
    a = make_addresses(seed, pairs, "uniform")
    out = np.repeat(a, 2, axis=0)
    out[0::2, 19] |= 0x01
    out[1::2, 19] &= 0xFE
    return out


def digits_only(seed: int = 7, n: int = 40) -> np.ndarray:
    """hex texts without a letter, as make_swarm's addresses are: bytes, lower-case text and EIP-55 text order alike"""
    rng = np.random.default_rng(seed)
    nib = rng.integers(0, 10, size=(n, 40), dtype=np.uint8)
    return (nib[:, 0::2] << 4 | nib[:, 1::2]).astype(np.uint8)


CASES = {
    "single": lambda: make_addresses(1, 1, "uniform"),
    "two": lambda: make_addresses(2, 2, "uniform"),
    "nine_B_a": nine_B_a,
    "last_nibble_pairs": last_nibble_pairs,
    "digits_only": digits_only,
    "letter_led": lambda: make_addresses(3, 48, "letter_led"),
    "prefix10": lambda: make_addresses(4, 48, "prefix10"),
    "prefix20": lambda: make_addresses(4, 48, "prefix20"),
    "prefix39": lambda: make_addresses(4, 48, "prefix39"),
    "duplicates": lambda: make_addresses(8, 48, "duplicates"),
    "all_equal": lambda: np.repeat(make_addresses(9, 1, "uniform"), 5, axis=0),
}
# cases in which two rows share their first ten characters: the rank must take its all-words sort
DEEP = {"last_nibble_pairs", "prefix10", "prefix20", "prefix39", "duplicates", "all_equal"}
