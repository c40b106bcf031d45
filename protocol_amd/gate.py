"""Packing for the request gate (include/pm_engine.h "request gate"): what the middleware sees of a request — the text it
hashes, the signature header, the x-address header — as the flat arrays pm_verify_requests takes.

Serialising the JSON stays with the caller: `message` is path + payload string exactly as the middleware formats it."""
from __future__ import annotations

import numpy as np

from .addresses import parse_address


def parse_signature(text: str):
    """A signature header — an optional "0x", then exactly 130 hex digits — as its 65 bytes (r | s | v), or None: the
    middleware's INVALID_SIGNATURE_FORMAT, which the device never sees as such (pack_requests sends v = 0xFF)."""
    body = text[2:] if text[:2] == "0x" else text
    if len(body) != 130 or any(c not in "0123456789abcdefABCDEF" for c in body):
        return None
    return bytes.fromhex(body)


def pack_requests(requests):
    """requests: (message bytes, signature, x-address) triples; the signature is 65 bytes or a header text, the address 20 bytes
    or a header text -> (bytes, offsets, sig65 [n, 65], claimed [n, 20], flags [n]).  A signature text that does not parse goes
    as 65 bytes of 0xFF (v = 0xFF is no recovery id: PM_RQ_BAD_SIGNATURE); an address text that does not parse sets
    PM_RQ_FLAG_BAD_ADDRESS and goes as zeros."""
    n = len(requests)
    msgs = [bytes(m) for m, _s, _a in requests]
    off = np.zeros(n + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
    buf = np.frombuffer(b"".join(msgs), dtype=np.uint8)
    sigs = np.zeros((max(n, 1), 65), dtype=np.uint8)
    claimed = np.zeros((max(n, 1), 20), dtype=np.uint8)
    flags = np.zeros(max(n, 1), dtype=np.uint8)
    for i, (_m, sig, addr) in enumerate(requests):
        if isinstance(sig, str):
            sig = parse_signature(sig)
        sigs[i] = np.frombuffer(sig, dtype=np.uint8) if sig is not None else 0xFF
        if isinstance(addr, str):
            try:
                addr = parse_address(addr)
            except ValueError:
                addr, flags[i] = bytes(20), 1
        claimed[i] = np.frombuffer(bytes(addr), dtype=np.uint8)
    return buf, off, sigs[:n], claimed[:n], flags[:n]
