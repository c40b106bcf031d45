"""Packing for the request gate's admission (include/pm_engine.h "request gate: admission"): what the middleware sees of a request
behind its signature — the request's timestamp and nonce, and whether the route is /heartbeat — beside what
protocol_amd.gate.pack_requests packs, as the flat arrays pm_admit_requests takes."""
from __future__ import annotations

import numpy as np

from .gate import pack_requests

FLAG_NO_TIMESTAMP, FLAG_NO_NONCE, FLAG_BEAT = 2, 4, 8


def pack_admissions(requests):
    """requests: (message bytes, signature, x-address, timestamp in seconds | None, nonce bytes or text | None, is_beat) ->
    (bytes, offsets, sig65 [n, 65], claimed [n, 20], flags [n], timestamp_s uint64 [n], nonce bytes, nonce offsets [n + 1]).
    A missing timestamp or nonce sets its flag and goes as 0 / as no bytes; the timestamp is taken modulo 2^64, as a u64 is."""
    n = len(requests)
    buf, off, sigs, claimed, flags = pack_requests([(m, s, a) for m, s, a, _t, _n, _b in requests])
    flags = flags.copy()
    ts = np.zeros(max(n, 1), dtype=np.uint64)
    nonces = []
    for i, (_m, _s, _a, t, nonce, beat) in enumerate(requests):
        if t is None:
            flags[i] |= FLAG_NO_TIMESTAMP
        else:
            ts[i] = int(t) & 0xFFFFFFFFFFFFFFFF
        if nonce is None:
            flags[i] |= FLAG_NO_NONCE
            nonce = b""
        nonces.append(nonce.encode("utf-8") if isinstance(nonce, str) else bytes(nonce))
        if beat:
            flags[i] |= FLAG_BEAT
    noff = np.zeros(n + 1, dtype=np.uint32)
    noff[1:] = np.cumsum([len(x) for x in nonces], dtype=np.uint64)
    nbuf = np.frombuffer(b"".join(nonces), dtype=np.uint8)
    return buf, off, sigs, claimed, flags, ts[:n], nbuf, noff
