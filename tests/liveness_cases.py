"""Named cases of one liveness sweep: every arm of tests/liveness_model.py and both sides of every edge.  A case is a row's
state before the sweep and what the header's table (include/pm_engine.h "liveness") says comes out of it, written down by
hand: `m` is the missing_heartbeat_threshold the case is named for, `beat` the beat's age in ms (None = never beaten, a
negative age = a beat in the future).  tests/test_liveness_model.py holds the model to the `want`s; tests/test_gpu_liveness.py
runs all of them through the engine under every threshold that occurs here, judged by the model."""
from liveness_model import (BANNED, DEAD, DISCOVERED, EJECTED, HEALTHY, LOWBALANCE, U32_MAX, UNHEALTHY, WAITING)

NOW_MS = 1_760_000_000_000
FRESH, STALE = 1000, 100_000   # well inside / well outside the 90 s


def case(name, status, counter, beat, in_pool, m, want_status, want_counter, listed):
    return dict(name=name, status=status, counter=counter, beat=beat, in_pool=in_pool, m=m,
                want=(want_status, want_counter, listed))


CASES = [
    # ---- absent, Unhealthy: Dead iff c' >= m (c' = m - 1, m, m + 1)
    case("unhealthy c'=m-1 stays", UNHEALTHY, 1, STALE, True, 3, UNHEALTHY, 2, False),
    case("unhealthy c'=m dies", UNHEALTHY, 2, STALE, True, 3, DEAD, 3, True),
    case("unhealthy c'=m+1 dies", UNHEALTHY, 3, STALE, True, 3, DEAD, 4, True),
    case("unhealthy out of pool c'=m dies", UNHEALTHY, 2, STALE, False, 3, DEAD, 3, True),
    # ---- absent, WaitingForHeartbeat: Unhealthy iff c' >= m
    case("waiting c'=m-1 stays", WAITING, 1, STALE, True, 3, WAITING, 2, False),
    case("waiting c'=m turns unhealthy", WAITING, 2, STALE, True, 3, UNHEALTHY, 3, True),
    case("waiting c'=m+1 turns unhealthy", WAITING, 3, STALE, True, 3, UNHEALTHY, 4, True),
    # ---- absent, Discovered
    case("discovered in pool turns unhealthy", DISCOVERED, 0, STALE, True, 3, UNHEALTHY, 1, True),
    case("discovered out of pool c'=360 stays", DISCOVERED, 359, STALE, False, 3, DISCOVERED, 360, False),
    case("discovered out of pool c'=361 dies", DISCOVERED, 360, STALE, False, 3, DEAD, 361, True),
    # ---- m = 0 and m = 1
    case("m=0: unhealthy dies at once", UNHEALTHY, 0, STALE, True, 0, DEAD, 1, True),
    case("m=0: waiting turns unhealthy at once", WAITING, 0, STALE, True, 0, UNHEALTHY, 1, True),
    case("m=1: unhealthy c'=1 dies", UNHEALTHY, 0, STALE, True, 1, DEAD, 1, True),
    case("m=1: waiting c'=1 turns unhealthy", WAITING, 0, STALE, True, 1, UNHEALTHY, 1, True),
    # ---- absent, Healthy
    case("healthy misses a beat", HEALTHY, 0, STALE, True, 3, UNHEALTHY, 1, True),
    case("healthy out of pool misses a beat", HEALTHY, 7, STALE, False, 3, UNHEALTHY, 8, True),
    # ---- present: the four that move
    case("unhealthy beats in pool", UNHEALTHY, 2, FRESH, True, 3, HEALTHY, 0, True),
    case("unhealthy beats out of pool", UNHEALTHY, 2, FRESH, False, 3, DISCOVERED, 0, True),
    case("waiting beats in pool", WAITING, 0, FRESH, True, 3, HEALTHY, 0, True),
    case("waiting beats out of pool", WAITING, 1, FRESH, False, 3, DISCOVERED, 0, True),
    case("discovered beats in pool", DISCOVERED, 5, FRESH, True, 3, HEALTHY, 0, True),
    case("discovered -> discovered is listed", DISCOVERED, 5, FRESH, False, 3, DISCOVERED, 0, True),
    case("dead revives in pool", DEAD, 9, FRESH, True, 3, HEALTHY, 0, True),
    case("dead beats out of pool", DEAD, 9, FRESH, False, 3, DISCOVERED, 0, True),
    # ---- the four sticky statuses, with and without a beat
    case("healthy beats", HEALTHY, 4, FRESH, True, 3, HEALTHY, 0, False),
    case("ejected beats", EJECTED, 4, FRESH, True, 3, EJECTED, 0, False),
    case("banned beats", BANNED, 4, FRESH, False, 3, BANNED, 0, False),
    case("lowbalance beats", LOWBALANCE, 4, FRESH, True, 3, LOWBALANCE, 0, False),
    case("dead stays dead, counting", DEAD, 4, STALE, True, 3, DEAD, 5, False),
    case("ejected silent, counting", EJECTED, 4, STALE, True, 3, EJECTED, 5, False),
    case("banned silent, counting", BANNED, 4, STALE, False, 3, BANNED, 5, False),
    case("lowbalance silent, counting", LOWBALANCE, 4, STALE, True, 3, LOWBALANCE, 5, False),
    # ---- the counter at u32 max (DEVIATION: saturates)
    case("counter at u32 max, unhealthy", UNHEALTHY, U32_MAX, STALE, True, 3, DEAD, U32_MAX, True),
    case("counter at u32 max - 1, banned", BANNED, U32_MAX - 1, STALE, True, 3, BANNED, U32_MAX, False),
    case("counter at u32 max, dead", DEAD, U32_MAX, STALE, True, 3, DEAD, U32_MAX, False),
    case("counter at u32 max cleared by a beat", WAITING, U32_MAX, FRESH, True, 3, HEALTHY, 0, True),
    # ---- the beat's age: 89,999 / 90,000 present, 90,001 absent; the future; never
    case("beat 89,999 ms old", UNHEALTHY, 1, 89_999, True, 3, HEALTHY, 0, True),
    case("beat 90,000 ms old", UNHEALTHY, 1, 90_000, True, 3, HEALTHY, 0, True),
    case("beat 90,001 ms old", HEALTHY, 0, 90_001, True, 3, UNHEALTHY, 1, True),
    case("beat in the future", WAITING, 2, -5000, True, 3, HEALTHY, 0, True),
    case("beat now", DEAD, 0, 0, True, 3, HEALTHY, 0, True),
    case("never beaten", HEALTHY, 0, None, True, 3, UNHEALTHY, 1, True),
    case("never beaten, waiting", WAITING, 0, None, True, 3, WAITING, 1, False),
]
THRESHOLDS = sorted({c["m"] for c in CASES})


def beat_ms(c, now_ms=NOW_MS) -> int:
    return 0 if c["beat"] is None else now_ms - c["beat"]
