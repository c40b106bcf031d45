"""A plain model of one liveness sweep (pm_liveness_sweep of include/pm_engine.h), written from the reference:
NodeStatusUpdater's process_node, orchestrator/src/status_update/mod.rs:191-372.  Every arm carries a label that names its
lines; tests/test_liveness_model.py holds the model to the reference's own tests (tests/golden/status_update_kats.json) and to
the named cases of tests/liveness_cases.py, and checks that every label is reached.  The GPU tests judge the engine by it."""
import numpy as np

# NodeStatus, models/node.rs:75-85, in its order
DISCOVERED, WAITING, HEALTHY, UNHEALTHY, DEAD, EJECTED, BANNED, LOWBALANCE, N_STATUS = range(9)
NAMES = ["Discovered", "WaitingForHeartbeat", "Healthy", "Unhealthy", "Dead", "Ejected", "Banned", "LowBalance"]
TTL_MS = 90000        # heartbeat_store.rs:32 (EX 90)
GIVE_UP = 360         # status_update/mod.rs:295
U32_MAX = 0xFFFFFFFF
W_HEALTHY = 1 << 9    # PM_W_HEALTHY

LABELS = {
    "beat:233-243:in_pool": "present, Unhealthy / Waiting, in pool -> Healthy, listed",
    "beat:233-243:out": "present, Unhealthy / Waiting, not in pool -> Discovered, listed",
    "beat:245-252:in_pool": "present, Discovered / Dead, in pool -> Healthy, listed",
    "beat:245-252:out": "present, Discovered / Dead, not in pool -> Discovered, listed (also Discovered -> Discovered)",
    "beat:sticky": "present, Healthy / Ejected / Banned / LowBalance -> unchanged, not listed",
    "none:274-277": "absent, Healthy -> Unhealthy, listed",
    "none:278-283:dead": "absent, Unhealthy, c' >= m -> Dead, listed",
    "none:278-283:stay": "absent, Unhealthy, c' < m -> unchanged",
    "none:285-291": "absent, Discovered, in pool -> Unhealthy, listed",
    "none:295-298:dead": "absent, Discovered, not in pool, c' > 360 -> Dead, listed",
    "none:295-298:stay": "absent, Discovered, not in pool, c' <= 360 -> unchanged",
    "none:301-308:unhealthy": "absent, Waiting, c' >= m -> Unhealthy, listed",
    "none:301-308:stay": "absent, Waiting, c' < m -> unchanged",
    "none:309": "absent, Dead / Ejected / Banned / LowBalance -> unchanged, not listed (the counter still counts)",
}
# on top of the arms: what happens to the counter
COUNTER_LABELS = {
    "counter:255-261": "present -> 0",
    "counter:265-271": "absent -> c + 1",
    "counter:saturated": "absent at u32 max -> stays (DEVIATION: the reference's parse::<u32> fails there)",
}


def beat_present(now_ms: int, beat_ms: int) -> bool:
    """get_heartbeat is Some: the key was set (beat != 0) and its 90 s have not run out; the edge millisecond is ours"""
    return beat_ms != 0 and (beat_ms > now_ms or now_ms - beat_ms <= TTL_MS)


def step(status: int, counter: int, present: bool, in_pool: bool, m: int):
    """one process_node -> (new status, new counter, listed, arm label, counter label)"""
    if present:
        clabel, c = "counter:255-261", 0
        if status in (UNHEALTHY, WAITING):                                   # :233-243
            return (HEALTHY if in_pool else DISCOVERED), c, True, "beat:233-243:" + ("in_pool" if in_pool else "out"), clabel
        if status in (DISCOVERED, DEAD):                                     # :245-252
            return (HEALTHY if in_pool else DISCOVERED), c, True, "beat:245-252:" + ("in_pool" if in_pool else "out"), clabel
        return status, c, False, "beat:sticky", clabel
    if counter >= U32_MAX:
        clabel, c = "counter:saturated", U32_MAX
    else:
        clabel, c = "counter:265-271", counter + 1
    if status == HEALTHY:                                                    # :274-277
        return UNHEALTHY, c, True, "none:274-277", clabel
    if status == UNHEALTHY:                                                  # :278-283
        if c >= m:
            return DEAD, c, True, "none:278-283:dead", clabel
        return status, c, False, "none:278-283:stay", clabel
    if status == DISCOVERED:                                                 # :284-300
        if in_pool:
            return UNHEALTHY, c, True, "none:285-291", clabel
        if c > GIVE_UP:
            return DEAD, c, True, "none:295-298:dead", clabel
        return status, c, False, "none:295-298:stay", clabel
    if status == WAITING:                                                    # :301-308
        if c >= m:
            return UNHEALTHY, c, True, "none:301-308:unhealthy", clabel
        return status, c, False, "none:301-308:stay", clabel
    return status, c, False, "none:309", clabel                              # :309


def pool_bit(bits, w: int) -> bool:
    return True if bits is None else bool((int(bits[w >> 6]) >> (w & 63)) & 1)


def pack_bits(flags) -> np.ndarray:
    """bool [W] -> uint64 [(W + 63) // 64], bit w & 63 of word w // 64"""
    flags = np.asarray(flags, dtype=bool)
    out = np.zeros((len(flags) + 63) // 64, dtype=np.uint64)
    for w in np.nonzero(flags)[0]:
        out[w >> 6] |= np.uint64(1) << np.uint64(w & 63)
    return out


class Ledger:
    """the engine's ledger and its last list, as the header specifies them"""

    def __init__(self, flags, m: int):
        self.m = int(m)
        self.status = [HEALTHY if int(f) & W_HEALTHY else DISCOVERED for f in flags]
        self.counter = [0] * len(self.status)
        self.rows = []

    def append(self, flags):
        self.status += [HEALTHY if int(f) & W_HEALTHY else DISCOVERED for f in flags]
        self.counter += [0] * len(flags)

    def set(self, idx, status, counter=None):
        for k, w in enumerate(idx):
            self.status[int(w)] = int(status[k])
            self.counter[int(w)] = 0 if counter is None else int(counter[k])

    def sweep(self, now_ms: int, beats, pool_bits=None):
        """-> (rows [(worker, old, new, counter)] ascending, census [N_STATUS])"""
        rows = []
        for w in range(len(self.status)):
            old = self.status[w]
            new, c, listed, _, _ = step(old, self.counter[w], beat_present(int(now_ms), int(beats[w])), pool_bit(pool_bits, w), self.m)
            self.status[w], self.counter[w] = new, c
            if listed:
                rows.append((w, old, new, c))
        self.rows = rows
        census = [0] * N_STATUS
        for s in self.status:
            census[s] += 1
        return rows, census
