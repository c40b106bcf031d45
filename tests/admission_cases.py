"""Named cases of the request gate's admission (include/pm_engine.h "request gate: admission"), with the answers written by
hand from the middleware's rules.  tests/test_admission_model.py holds the sequential model to them; tests/test_gpu_admission.py
holds pm_admit_requests to them and to the model.

The cast is fixed: signers 0, 1, 2 are healthy nodes, signer 3 is Banned, signer 4 is Ejected, signer 5 is in no row.  A
request is (who, gate, age, nonce, beat): `gate` is the code the request gate gives it (the GPU test builds a request that
gets it), `age` the seconds its timestamp lies before now_ms // 1000 (negative: in the future; None: no x-timestamp), `nonce`
its bytes (None: no x-nonce).  A case: rate = the windows set before the first call {who: (window_start_ms, count)}; calls =
[(now_ms, [requests])]; want = the codes of each call; and what the ledgers hold in the end where the case is about that:
end_rate {who: (window_start_ms, count)}, end_beats {who: ms}, end_held = entries in the nonce set."""
import admission_model as A

T0 = 1_700_000_000_000
BANNED_SIGNER, EJECTED_SIGNER, STRANGER = 3, 4, 5


def nonce(k: int) -> bytes:
    return b"nonce-%06d-AbCdEf" % k  # 19 bytes


def ok(who, k, beat=False, age=0):
    return (who, A.BANNED if who == BANNED_SIGNER else A.OK, age, nonce(k), beat)


CASES = {}


def case(name, calls, want, rate=None, **end):
    assert name not in CASES and len(calls) == len(want) and all(len(c[1]) == len(w) for c, w in zip(calls, want)), name
    CASES[name] = dict(rate=rate or {}, calls=calls, want=want, **end)


# ---- precedence: every code once, and the earlier rule of each adjacent pair wins
case("gate_codes_touch_nothing",
     [(T0, [(0, A.BAD_SIGNATURE, 0, nonce(1), True), (0, A.NO_KEY, 0, nonce(1), True), (0, A.BAD_ADDRESS, 0, nonce(1), True),
            (0, A.MISMATCH, 0, nonce(1), True), (STRANGER, A.UNKNOWN, 0, nonce(1), True), (EJECTED_SIGNER, A.EJECTED, 0, nonce(1), True),
            ok(0, 1)])],
     [[A.BAD_SIGNATURE, A.NO_KEY, A.BAD_ADDRESS, A.MISMATCH, A.UNKNOWN, A.EJECTED, A.OK]],
     end_rate={0: (T0, 1), EJECTED_SIGNER: (0, 0)}, end_beats={0: 0, EJECTED_SIGNER: 0}, end_held=1)
case("the_new_codes",
     [(T0, [ok(0, 1), ok(0, 2), (1, A.OK, 301, nonce(3), False), (1, A.OK, 0, b"short", False), (1, A.OK, 0, nonce(1), False),
            (1, A.OK, 0, None, False), ok(BANNED_SIGNER, 4)])],
     [[A.OK, A.RATE_LIMITED, A.EXPIRED, A.BAD_NONCE, A.REPLAY, A.NO_NONCE, A.BANNED]],
     rate={0: (T0 - 1, 99)})
case("ejected_before_rate_limit", [(T0, [(EJECTED_SIGNER, A.EJECTED, 0, nonce(1), False)])], [[A.EJECTED]],
     rate={EJECTED_SIGNER: (T0 - 1, 100)}, end_rate={EJECTED_SIGNER: (T0 - 1, 100)})
case("rate_limit_before_age", [(T0, [(0, A.OK, 301, nonce(1), False)])], [[A.RATE_LIMITED]], rate={0: (T0 - 1, 100)})
case("age_before_no_nonce", [(T0, [(0, A.OK, 301, None, False)])], [[A.EXPIRED]])
case("no_nonce_before_format", [(T0, [(0, A.OK, 0, None, False)])], [[A.NO_NONCE]])
case("format_before_replay",  # (a refused nonce is never stored: its second copy is refused for its format again)
     [(T0, [(0, A.OK, 0, b"bad_nonce_with_underscore", False), (1, A.OK, 0, b"bad_nonce_with_underscore", False)])],
     [[A.BAD_NONCE, A.BAD_NONCE]], end_held=0)
case("replay_before_banned",
     [(T0, [ok(0, 1), (BANNED_SIGNER, A.BANNED, 0, nonce(1), False), ok(BANNED_SIGNER, 2), ok(1, 2)])],
     [[A.OK, A.REPLAY, A.BANNED, A.REPLAY]], end_held=2)

# ---- rate limit
case("count_98_interleaved",
     [(T0, [ok(0, 1), ok(1, 2), ok(0, 3), ok(2, 4), ok(0, 5), ok(1, 6), ok(0, 7)])],
     [[A.OK, A.OK, A.OK, A.OK, A.RATE_LIMITED, A.OK, A.RATE_LIMITED]],
     rate={0: (T0 - 1000, 98)}, end_rate={0: (T0 - 1000, 100), 1: (T0, 2), 2: (T0, 1)}, end_held=5)
case("count_99", [(T0, [ok(0, 1), ok(0, 2)])], [[A.OK, A.RATE_LIMITED]], rate={0: (T0 - 1, 99)}, end_rate={0: (T0 - 1, 100)})
case("count_100", [(T0, [ok(0, 1)])], [[A.RATE_LIMITED]], rate={0: (T0 - 1, 100)}, end_rate={0: (T0 - 1, 100)}, end_held=0)
case("window_59999_ms", [(T0, [ok(0, 1)])], [[A.RATE_LIMITED]], rate={0: (T0 - 59999, 100)}, end_rate={0: (T0 - 59999, 100)})
case("window_60000_ms", [(T0, [ok(0, 1), ok(0, 2)])], [[A.OK, A.OK]], rate={0: (T0 - 60000, 100)}, end_rate={0: (T0, 2)})
case("now_below_the_window_start",  # (duration_since saturates: elapsed 0)
     [(T0, [ok(0, 1), ok(1, 2)])], [[A.RATE_LIMITED, A.OK]],
     rate={0: (T0 + 5000, 100), 1: (T0 + 5000, 3)}, end_rate={0: (T0 + 5000, 100), 1: (T0 + 5000, 4)})
case("fresh_row", [(T0, [ok(2, 1)])], [[A.OK]], end_rate={2: (T0, 1)})
case("mismatch_and_unknown_do_not_count",
     [(T0, [(0, A.MISMATCH, 0, nonce(1), False), (STRANGER, A.UNKNOWN, 0, nonce(2), False)])], [[A.MISMATCH, A.UNKNOWN]],
     end_rate={0: (0, 0)}, end_held=0)
case("banned_and_expired_count",
     [(T0, [ok(BANNED_SIGNER, 1), (0, A.OK, 301, nonce(2), False), (0, A.OK, 0, None, False), (0, A.OK, 0, b"x", False)])],
     [[A.BANNED, A.EXPIRED, A.NO_NONCE, A.BAD_NONCE]], end_rate={BANNED_SIGNER: (T0, 1), 0: (T0, 3)}, end_held=1)
case("a_hundred_and_one_from_nothing", [(T0, [ok(0, k) for k in range(101)])], [[A.OK] * 100 + [A.RATE_LIMITED]],
     end_rate={0: (T0, 100)}, end_held=100)

# ---- age
case("age_300_s", [(T0, [ok(0, 1, age=300)])], [[A.OK]])
case("age_301_s", [(T0, [ok(0, 1, age=301)])], [[A.EXPIRED]], end_held=0)
case("a_future_timestamp_expires", [(T0, [ok(0, 1, age=-1)])], [[A.EXPIRED]], end_rate={0: (T0, 1)})
case("no_timestamp_skips_the_age", [(T0, [ok(0, 1, age=None)])], [[A.OK]])

# ---- the nonce's format
case("nonce_lengths", [(T0, [(0, A.OK, 0, b"a" * 15, False), (0, A.OK, 0, b"b" * 16, False), (0, A.OK, 0, b"c" * 64, False),
                             (0, A.OK, 0, b"d" * 65, False)])],
     [[A.BAD_NONCE, A.OK, A.OK, A.BAD_NONCE]], end_held=2)
case("nonce_characters",
     [(T0, [(0, A.OK, 0, b"0123-abcd-WXYZ-789", False), (0, A.OK, 0, b"0123_abcd_WXYZ_789", False),
            (0, A.OK, 0, b"0123 abcd WXYZ 789", False), (0, A.OK, 0, b"0123abcdWXYZ789\x80zz", False),
            (0, A.OK, 0, b"azAZ09-/zzzzzzzzzzzz", False), (0, A.OK, 0, b"azAZ09-:zzzzzzzzzzzz", False),
            (0, A.OK, 0, b"azAZ09-@zzzzzzzzzzzz", False), (0, A.OK, 0, b"azAZ09-[zzzzzzzzzzzz", False),
            (0, A.OK, 0, b"azAZ09-`zzzzzzzzzzzz", False), (0, A.OK, 0, b"azAZ09-{zzzzzzzzzzzz", False)])],
     [[A.OK] + [A.BAD_NONCE] * 9], end_held=1)

# ---- the nonce set, inside one batch
case("duplicate_in_one_batch", [(T0, [ok(0, 1), ok(1, 2), ok(2, 1), ok(1, 1)])], [[A.OK, A.OK, A.REPLAY, A.REPLAY]], end_held=2)
case("first_copy_rate_limited", [(T0, [ok(0, 1), ok(1, 1)])], [[A.RATE_LIMITED, A.OK]], rate={0: (T0 - 1, 100)}, end_held=1)
case("first_copy_expired", [(T0, [ok(0, 1, age=301), ok(1, 1), ok(2, 1)])], [[A.EXPIRED, A.OK, A.REPLAY]], end_held=1)

# ---- the nonce set, across calls
case("replay_across_calls", [(T0, [ok(0, 1), ok(0, 2)]), (T0 + 1000, [ok(1, 2), ok(1, 3)])], [[A.OK, A.OK], [A.REPLAY, A.OK]],
     end_held=3)
case("ttl_edges_and_no_refresh",  # (a refresh at + 40 s would still refuse at + 60,001 ms)
     [(T0, [ok(0, 1)]), (T0 + 40000, [ok(1, 1)]), (T0 + 60000, [ok(2, 1)]), (T0 + 60001, [ok(1, 1)]), (T0 + 60002, [ok(2, 1)])],
     [[A.OK], [A.REPLAY], [A.REPLAY], [A.OK], [A.REPLAY]], end_held=1)
case("purge", [(T0, [ok(0, 1), ok(0, 2), ok(0, 3)]), (T0 + 30000, [ok(1, 4)]), (T0 + 70000, [ok(1, 5)])],
     [[A.OK] * 3, [A.OK], [A.OK]], end_held=2)

# ---- beats
case("ok_beat_stamps", [(T0, [ok(0, 1, beat=True)])], [[A.OK]], end_beats={0: T0})
case("what_does_not_stamp",
     [(T0, [ok(BANNED_SIGNER, 1, beat=True), ok(0, 2), ok(1, 2, beat=True), ok(2, 3, beat=True, age=301),
            (EJECTED_SIGNER, A.EJECTED, 0, nonce(4), True)])],
     [[A.BANNED, A.OK, A.REPLAY, A.EXPIRED, A.EJECTED]], end_beats={0: 0, 1: 0, 2: 0, BANNED_SIGNER: 0, EJECTED_SIGNER: 0})
case("two_beats_of_one_row", [(T0, [ok(0, 1, beat=True), ok(1, 2), ok(0, 3, beat=True)]), (T0 + 500, [ok(1, 4, beat=True)])],
     [[A.OK, A.OK, A.OK], [A.OK]], end_beats={0: T0, 1: T0 + 500})
