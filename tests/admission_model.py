"""The middleware behind its signature check, one request at a time (auth_signature_middleware.rs:424-483 and the heartbeat
handler's stamp): what pm_admit_requests must equal.  Plain Python, dictionaries for the three stores; written from the
middleware, not from the kernels: nothing here sorts, ranks or merges.

A request is what the gate already decided about it — (gate_code, row) — with its flags, timestamp and nonce; the gate's own
rules are the gate's tests' business (tests/test_gpu_gate.py)."""

# pm_engine.h's codes and flags
BAD_SIGNATURE, NO_KEY, BAD_ADDRESS, MISMATCH, UNKNOWN, EJECTED, BANNED, OK = range(8)
RATE_LIMITED, EXPIRED, BAD_NONCE, REPLAY, NO_NONCE, N_CODES = range(8, 14)
FLAG_BAD_ADDRESS, FLAG_NO_TIMESTAMP, FLAG_NO_NONCE, FLAG_BEAT = 1, 2, 4, 8
WINDOW_MS, MAX_REQUESTS, MAX_AGE_S, NONCE_TTL_MS = 60000, 100, 300, 60000
U64 = (1 << 64) - 1
NONCE_CHARS = frozenset(b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz-")


def nonce_ok(nonce: bytes) -> bool:
    """:135-140: 16 to 64 bytes, ASCII alphanumeric or '-'"""
    return 16 <= len(nonce) <= 64 and all(c in NONCE_CHARS for c in nonce)


def nonce_live(now_ms: int, stored_ms: int) -> bool:
    """EX 60 by the liveness ledger's convention: the edge millisecond is still there"""
    return now_ms < stored_ms or now_ms - stored_ms <= NONCE_TTL_MS


class Model:
    def __init__(self):
        self.rate = {}    # row -> (window_start_ms, count); absent = (0, 0)
        self.nonces = {}  # nonce bytes -> stored_ms
        self.beats = {}   # row -> last_beat_ms; absent = 0

    def drop_rows(self):
        """pm_upload_workers(keep_groups = 0): the row identities are gone; the nonce set is tied to none"""
        self.rate.clear()
        self.beats.clear()

    def set_rate(self, row, window_start_ms, count):
        if window_start_ms == 0 and count == 0:
            self.rate.pop(row, None)
        else:
            self.rate[row] = (window_start_ms, count)

    def rate_of(self, row):
        return self.rate.get(row, (0, 0))

    def beat_of(self, row):
        return self.beats.get(row, 0)

    def counters(self, now_ms):
        """(entries live at now_ms, entries held)"""
        return sum(1 for t in self.nonces.values() if nonce_live(now_ms, t)), len(self.nonces)

    def admit_one(self, now_ms, gate_code, row, flags, timestamp_s, nonce) -> int:
        if gate_code not in (BANNED, OK):
            return gate_code
        # check_rate_limit (:142-157)
        w, c = self.rate_of(row)
        if (w == 0 and c == 0) or max(now_ms - w, 0) >= WINDOW_MS:
            self.rate[row] = (now_ms, 1)
        elif c >= MAX_REQUESTS:
            return RATE_LIMITED
        else:
            self.rate[row] = (w, c + 1)
        # the age (:433-447), wrapping as a release build's u64 does
        if not flags & FLAG_NO_TIMESTAMP and ((now_ms // 1000 - timestamp_s) & U64) > MAX_AGE_S:
            return EXPIRED
        # the nonce (:135-140, :159-183, :449-483)
        if flags & FLAG_NO_NONCE:
            return NO_NONCE
        if not nonce_ok(nonce):
            return BAD_NONCE
        stored = self.nonces.get(nonce)
        if stored is not None and nonce_live(now_ms, stored):
            return REPLAY  # (NX: the entry keeps its time)
        self.nonces[nonce] = now_ms
        if gate_code == BANNED:
            return BANNED
        if flags & FLAG_BEAT:
            self.beats[row] = max(self.beat_of(row), now_ms)
        return OK

    def admit(self, now_ms, requests):
        """requests: (gate_code, row, flags, timestamp_s, nonce bytes) in batch order -> the codes; entries that are no longer
        live leave the set during the call"""
        codes = [self.admit_one(now_ms, *r) for r in requests]
        self.nonces = {k: t for k, t in self.nonces.items() if nonce_live(now_ms, t)}
        return codes
