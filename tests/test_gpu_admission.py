"""The request gate's admission on the GPU (pm_admit_requests and its ledgers, include/pm_engine.h "request gate: admission";
kernels in pm_admission.inc) against the sequential model (tests/admission_model.py) and the answers written by hand
(tests/admission_cases.py).  Integers only: every comparison is equality.

Requests are signed with the big-integer model as tests/test_gpu_gate.py does; the nonce and the timestamp travel beside the
signed bytes, so six signatures serve every test, and pm_admission_rate_set reaches the count edges."""
import numpy as np
import pytest

from protocol_amd import admission as AD
from protocol_amd import engine as E
from protocol_amd import host
from protocol_amd.addresses import make_addresses
from protocol_amd.swarm import make_swarm

import admission_cases as AC
import admission_model as A
from test_gpu_addresses import TWO_CHUNKS
from test_gpu_gate import ADDR, _code, _cols, _published, _req

pytestmark = pytest.mark.gpu

EINVAL, ERANGE, ESTATE = -1, -5, -4
NONE = 0xFFFFFFFF
T0 = AC.T0
MSG = [b"/heartbeat{\"signer\":%d}" % k for k in range(6)]
BAD_V = bytes(64) + b"\x1d"                    # v = 29: no recovery id
NO_KEY = bytes(32) + (1).to_bytes(32, "big") + b"\x1b"  # r = 0: nothing is recovered


def _request(who, gate, rows):
    """(message, signature, x-address, BAD_ADDRESS flag) of a request the gate gives `gate`"""
    msg, sig, addr = _req(who, MSG[who])
    if gate == A.BAD_SIGNATURE:
        sig = BAD_V
    elif gate == A.NO_KEY:
        sig = NO_KEY
    elif gate == A.MISMATCH:
        addr = ADDR[(who + 1) % 3]
    return msg, sig, addr, 1 if gate == A.BAD_ADDRESS else 0


def _pack(reqs, now_ms, rows):
    """abstract requests (tests/admission_cases.py) -> pack_admissions' arrays, and the model's batch"""
    full, bad, batch = [], [], []
    for who, gate, age, nonce, beat in reqs:
        msg, sig, addr, flag = _request(who, gate, rows)
        ts = None if age is None else (now_ms // 1000 - age) & A.U64
        full.append((msg, sig, addr, ts, nonce, beat))
        bad.append(flag)
        flags = (A.FLAG_NO_TIMESTAMP if age is None else 0) | (A.FLAG_NO_NONCE if nonce is None else 0) | (A.FLAG_BEAT if beat else 0)
        batch.append((gate, rows.get(who, NONE), flags, ts or 0, nonce or b""))
    packed = list(AD.pack_admissions(full))
    packed[4] = packed[4] | np.asarray(bad, dtype=np.uint8)
    return tuple(packed), batch


class Pair:
    """an engine and the model side by side: rows = {signer: row}"""

    def __init__(self, W, rows, on=True, liveness=True, seed=3):
        self.eng = E.Engine(device=0)
        self.rows = dict(rows)
        self.eng.upload_workers(_cols(W))
        self.eng.enable_addresses(True)
        self.place(seed)
        if liveness:
            self.eng.liveness_enable(True)
            self.eng.liveness_set([self.rows[AC.BANNED_SIGNER], self.rows[AC.EJECTED_SIGNER]], [E.NS_BANNED, E.NS_EJECTED])
        self.reset(on)

    def place(self, seed=3):
        addrs = make_addresses(seed, self.eng.W, "uniform")
        for who, row in self.rows.items():
            addrs[row] = np.frombuffer(ADDR[who], dtype=np.uint8)
        self.eng.set_addresses(0, addrs)

    def reset(self, on=True):
        self.eng.enable_admission(on)
        self.model = A.Model()

    def set_rate(self, who, window_start_ms, count):
        self.eng.admission_rate_set([self.rows[who]], [window_start_ms], [count])
        self.model.set_rate(self.rows[who], window_start_ms, count)

    def admit(self, now_ms, reqs):
        packed, batch = _pack(reqs, now_ms, self.rows)
        v, counts = self.eng.admit_requests(packed, now_ms)
        got = [int(c) for c in v["code"]]
        assert counts.tolist() == np.bincount(got, minlength=E.AD_N_CODES).tolist()  # the device's census
        want = self.model.admit(now_ms, batch)
        assert got == want, [(k, g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w][:8]
        for k, (gate, row, *_rest) in enumerate(batch):  # the row as pm_verify_requests fills it: from MISMATCH on
            assert int(v["row"][k]) == (row if gate >= A.MISMATCH else NONE), k
        self.last = v
        return got

    def readout(self, now_ms):
        idx = np.arange(self.eng.W, dtype=np.uint32)
        win, cnt = self.eng.admission_rate_get(idx)
        return win.tolist(), cnt.tolist(), self.eng.admission_nonces(now_ms), self.eng.beats_get(idx).tolist()

    def check_state(self, now_ms):
        win, cnt, counters, beats = self.readout(now_ms)
        for w in range(self.eng.W):
            assert (win[w], cnt[w]) == self.model.rate_of(w), w
            assert beats[w] == self.model.beat_of(w), w
        assert counters == self.model.counters(now_ms)
        return win, cnt, counters, beats

    def close(self):
        self.eng.close()


ROWS = {0: 7, 1: 299, 2: 64, 3: 150, 4: 0}  # (signer 5 is in no row)


@pytest.fixture(scope="module")
def cast():
    p = Pair(300, ROWS)
    yield p
    p.close()


# ---- every named case: the codes written by hand, the model, and what the ledgers hold

@pytest.mark.parametrize("name", list(AC.CASES))
def test_every_named_case(cast, name):
    c = AC.CASES[name]
    cast.reset()
    for who, (w, n) in c["rate"].items():
        cast.set_rate(who, w, n)
    now_ms = T0
    for (now_ms, reqs), want in zip(c["calls"], c["want"]):
        assert cast.admit(now_ms, reqs) == want
        cast.check_state(now_ms)
    win, cnt, counters, beats = cast.readout(now_ms)
    for who, want in c.get("end_rate", {}).items():
        assert (win[ROWS[who]], cnt[ROWS[who]]) == want, who
    for who, want in c.get("end_beats", {}).items():
        assert beats[ROWS[who]] == want, who
    if "end_held" in c:
        assert counters[1] == c["end_held"]


def test_the_verdict_carries_the_gates_row_status_and_address(cast):
    cast.reset()
    cast.admit(T0, [AC.ok(0, 1), AC.ok(AC.BANNED_SIGNER, 2), (AC.EJECTED_SIGNER, A.EJECTED, 0, AC.nonce(3), False),
                    (AC.STRANGER, A.UNKNOWN, 0, AC.nonce(4), False), (0, A.BAD_SIGNATURE, 0, AC.nonce(5), False)])
    v = cast.last
    assert [int(x) for x in v["status"]] == [E.NS_HEALTHY, E.NS_BANNED, E.NS_EJECTED, 0xFF, 0xFF]
    assert [v["address"][k].tobytes() for k in range(5)] == [ADDR[0], ADDR[3], ADDR[4], ADDR[5], bytes(20)]


# ---- the rate ledger's keys

@pytest.mark.parametrize("W, row", [(200, 199), (70000, 69999)])
def test_row_key_widths(W, row):
    """the sort by row takes as many byte passes as W needs: one, (W = 300: two, every named case,) three — a row >= 65,536"""
    rows = dict(ROWS)
    rows[0] = row
    rows[1], rows[3] = 100, 101
    p = Pair(W, rows)
    c = AC.CASES["count_98_interleaved"]
    p.set_rate(0, *c["rate"][0])
    assert p.admit(T0, c["calls"][0][1]) == c["want"][0]
    p.check_state(T0)
    assert _rate(p.eng, [row]) == ([T0 - 1000], [100])
    p.close()


def test_two_rows_with_one_address_count_on_the_lowest():
    p = Pair(65, {0: 40, 1: 5, 2: 6, 3: 8, 4: 9})
    p.eng.set_addresses(12, [ADDR[0]])
    p.eng.set_addresses(63, [ADDR[0]])
    p.rows[0] = 12
    p.admit(T0, [AC.ok(0, 1, beat=True), AC.ok(0, 2)])
    p.check_state(T0)
    assert _rate(p.eng, [12, 40, 63]) == ([T0, 0, 0], [2, 0, 0])
    assert p.eng.beats_get([12, 40, 63]).tolist() == [T0, 0, 0]
    p.close()


def test_a_batch_one_past_a_sort_chunk(cast):
    """TWO_CHUNKS requests: both sorts run over two chunks; rows at 90, 0 and 100 of a hundred, nonces that repeat"""
    cast.reset()
    cast.set_rate(0, T0 - 5, 90)
    cast.set_rate(2, T0 - 5, 100)
    rng = np.random.default_rng(5)
    reqs = []
    for k in range(TWO_CHUNKS):
        who = int(rng.integers(0, 6))
        gate = {3: A.BANNED, 4: A.EJECTED, 5: A.UNKNOWN}.get(who, A.OK)
        reqs.append((who, gate, int(rng.choice([0, 0, 0, 301])), AC.nonce(int(rng.integers(0, 150))), bool(rng.integers(0, 2))))
    got = cast.admit(T0, reqs)
    assert {A.OK, A.BANNED, A.EJECTED, A.UNKNOWN, A.RATE_LIMITED, A.EXPIRED, A.REPLAY} <= set(got)
    cast.check_state(T0)


# ---- the nonce set

def test_prefix_narrowed_to_four_bits(cast):
    """64 distinct nonces under a 4-bit key: runs of equal keys on both sides; no false replay, every true one found"""
    cast.eng.enable_admission(E.ad_debug_prefix_bits(4))
    cast.model = A.Model()
    first = [AC.ok(k % 3, k) for k in range(32)]
    second = [AC.ok(k % 3, k) for k in range(32, 64)]
    assert cast.admit(T0, first) == [A.OK] * 32
    assert cast.admit(T0 + 1, second) == [A.OK] * 32
    assert cast.eng.admission_nonces(T0 + 1) == (64, 64)
    both = [AC.ok(k % 3, k) for k in range(63, -1, -1)] + [AC.ok(k % 3, k) for k in range(64, 70)] + [AC.ok(0, 64)]
    assert cast.admit(T0 + 2, both) == [A.REPLAY] * 64 + [A.OK] * 6 + [A.REPLAY]
    cast.check_state(T0 + 2)
    assert _code(lambda: cast.eng.enable_admission(E.ad_debug_prefix_bits(65))) == EINVAL
    cast.reset()


def _rate(eng, idx):
    win, cnt = eng.admission_rate_get(idx)
    return win.tolist(), cnt.tolist()


def _key(nonce: bytes) -> int:
    return int.from_bytes(E.host_keccak256(nonce)[:8], "big")


def test_a_standing_set_one_past_a_sort_chunk(cast):
    """TWO_CHUNKS standing nonces, then a batch whose keys fall before the first, between, and behind the last of them"""
    cast.reset()
    pool = sorted((AC.nonce(k) for k in range(TWO_CHUNKS + 7)), key=_key)
    late = [pool[0], pool[1], pool[400], pool[401], pool[777], pool[-2], pool[-1]]
    standing = [x for x in pool if x not in late]
    assert len(standing) == TWO_CHUNKS
    rng = np.random.default_rng(9)
    order = [standing[i] for i in rng.permutation(len(standing))]
    for lo in range(0, len(order), 300):  # a hundred a row and window: the windows are put back between the calls
        chunk = order[lo:lo + 300]
        for who in range(3):
            cast.set_rate(who, 0, 0)
        assert cast.admit(T0, [(k % 3, A.OK, 0, x, False) for k, x in enumerate(chunk)]) == [A.OK] * len(chunk)
    assert cast.eng.admission_nonces(T0) == (TWO_CHUNKS, TWO_CHUNKS)
    for who in range(3):
        cast.set_rate(who, 0, 0)
    srt = sorted(standing, key=_key)
    batch = late + [srt[0], srt[-1], srt[500]]
    assert max(_key(late[0]), _key(late[1])) < _key(srt[0]) and min(_key(late[-1]), _key(late[-2])) > _key(srt[-1])
    assert cast.admit(T0 + 1, [(k % 3, A.OK, 0, x, False) for k, x in enumerate(batch)]) == [A.OK] * 7 + [A.REPLAY] * 3
    assert cast.eng.admission_nonces(T0 + 1) == (TWO_CHUNKS + 7, TWO_CHUNKS + 7)
    again = late + [srt[1], srt[-2], AC.nonce(999999)]
    assert cast.admit(T0 + 2, [(k % 3, A.OK, 0, x, False) for k, x in enumerate(again)]) == [A.REPLAY] * 9 + [A.OK]
    cast.check_state(T0 + 2)
    # and all of it leaves together
    assert cast.admit(T0 + 2 + 60001, [AC.ok(0, 5)]) == [A.OK]
    assert cast.eng.admission_nonces(T0 + 2 + 60001) == (1, 1)


def test_n_held_falls_after_the_purge(cast):
    cast.reset()
    cast.admit(T0, [AC.ok(0, k) for k in range(20)])
    assert cast.eng.admission_nonces(T0 + 60000) == (20, 20)
    assert cast.eng.admission_nonces(T0 + 60001) == (0, 20)  # (a read: nothing leaves)
    cast.admit(T0 + 59000, [AC.ok(1, 100)])
    assert cast.eng.admission_nonces(T0 + 60001) == (1, 21)
    cast.admit(T0 + 60001, [AC.ok(1, 100)])                  # a replay: nothing stored, the twenty leave
    assert cast.eng.admission_nonces(T0 + 60001) == (1, 1)
    cast.check_state(T0 + 60001)


def test_the_set_survives_an_upload_the_row_ledgers_do_not():
    W = 40
    p = Pair(W, {0: 3, 1: 4, 2: 5, 3: 6, 4: 7}, liveness=False)
    assert p.admit(T0, [AC.ok(0, 1, beat=True), AC.ok(1, 2, beat=True), (3, A.OK, 0, AC.nonce(3), True)]) == [A.OK] * 3  # liveness off: no BANNED
    p.check_state(T0)
    first = p.eng.append_workers(_cols(5))                   # appended rows start empty, the others keep theirs
    assert first == W
    p.check_state(T0)
    assert _rate(p.eng, [3, W, W + 4]) == ([T0, 0, 0], [1, 0, 0])
    p.eng.upload_workers(_cols(W + 5), keep_groups=True)     # keep_groups = 1: kept
    p.check_state(T0)
    p.eng.upload_workers(_cols(W + 5))                       # keep_groups = 0: the rows are new rows, the nonces are not
    p.place()
    p.model.drop_rows()
    p.check_state(T0)
    assert p.eng.admission_nonces(T0) == (3, 3)
    assert p.eng.beats_get([3, 4]).tolist() == [0, 0] and _rate(p.eng, [3, 4]) == ([0, 0], [0, 0])
    assert p.admit(T0 + 5, [AC.ok(0, 1), AC.ok(0, 4)]) == [A.REPLAY, A.OK]
    p.check_state(T0 + 5)
    p.close()


# ---- beats and the sweep

def _sweep_leg(use_device_column, host_col):
    """a table of 300, beats stamped by admission and by pm_beats_set, then one sweep — from the device's column (and host_col
    beside it), or pm_liveness_sweep fed what pm_beats_get reads (the later of it and host_col)"""
    W = 300
    p = Pair(W, ROWS)
    now = T0 + 400_000
    rng = np.random.default_rng(21)
    idx = rng.permutation(W)[:200].astype(np.uint32)
    p.eng.beats_set(idx, (now - rng.integers(0, 400_000, 200)).astype(np.uint64))
    for w, ms in zip(idx.tolist(), p.eng.beats_get(idx).tolist()):
        p.model.beats[w] = ms
    p.admit(now - 10, [AC.ok(0, 1, beat=True), AC.ok(1, 2, beat=True), AC.ok(2, 3)])
    p.check_state(now)
    col = p.eng.beats_get(np.arange(W, dtype=np.uint32))
    pool = rng.integers(0, 2**63, (W + 63) // 64, dtype=np.uint64)
    if use_device_column:
        n, census = p.eng.liveness_sweep_beats(now, host_col, pool)
    else:
        n, census = p.eng.liveness_sweep(now, col if host_col is None else np.maximum(col, host_col), pool)
    rows = p.eng.liveness_transitions().tolist()
    status, counter = p.eng.liveness_get()
    assert p.eng.beats_get(np.arange(W, dtype=np.uint32)).tolist() == col.tolist()  # the sweep reads the column
    p.close()
    return n, census.tolist(), rows, status.tolist(), counter.tolist()


def test_sweep_from_the_device_column_equals_the_sweep_fed_with_it():
    a, b = _sweep_leg(True, None), _sweep_leg(False, None)
    assert a == b and a[0] > 0


def test_sweep_takes_the_later_of_the_device_and_the_host_column():
    rng = np.random.default_rng(22)
    host_col = (T0 + rng.integers(0, 400_000, 300)).astype(np.uint64)  # later than the device's for some rows, earlier for others
    host_col[::7] = 0
    a, b = _sweep_leg(True, host_col), _sweep_leg(False, host_col)
    assert a == b and a[0] > 0 and a != _sweep_leg(True, None)


# ---- soak

SOAK_ROWS = {0: 7, 1: 29, 2: 64, 3: 15, 4: 0}


def soak_script():
    """40 batches of up to 64 requests over the six signers, signer 0 the busiest, the clock advancing by nothing, a millisecond,
    seconds or more than a window; after some of them rows are appended or a signer's status changes -> [(now_ms, requests,
    rows to append, (signer, status) or None)]"""
    rng = np.random.default_rng(33)
    status = {0: E.NS_HEALTHY, 1: E.NS_HEALTHY, 2: E.NS_HEALTHY, 3: E.NS_BANNED, 4: E.NS_EJECTED}
    now, script = T0, []
    for step in range(40):
        now += int(rng.choice([0, 1, 700, 4000, 15000, 61000], p=[.15, .15, .35, .25, .07, .03]))
        reqs = []
        for _ in range(int(rng.integers(1, 65))):
            who = int(rng.choice(6, p=[.4, .15, .15, .1, .1, .1]))
            gate = A.UNKNOWN if who == 5 else {E.NS_BANNED: A.BANNED, E.NS_EJECTED: A.EJECTED}.get(status[who], A.OK)
            roll = int(rng.integers(0, 20))
            if roll == 0:
                gate = int(rng.choice([A.BAD_SIGNATURE, A.NO_KEY, A.BAD_ADDRESS, A.MISMATCH]))
            age = None if roll == 1 else int(rng.choice([0, 10, 300, 301, -1], p=[.5, .3, .1, .05, .05]))
            nonce = None if roll == 2 else b"short" if roll == 3 else AC.nonce(int(rng.integers(0, 400)))
            reqs.append((who, gate, age, nonce, bool(rng.integers(0, 2))))
        append = int(rng.integers(1, 9)) if step % 7 == 3 else 0
        change = None
        if step % 5 == 2:
            who = int(rng.integers(0, 5))
            status[who] = int(rng.choice([E.NS_HEALTHY, E.NS_BANNED, E.NS_EJECTED]))
            change = (who, status[who])
        script.append((now, reqs, append, change))
    return script


def _soak():
    p = Pair(70, SOAK_ROWS)
    log = []
    for now, reqs, append, change in soak_script():
        got = p.admit(now, reqs)
        log.append((got, p.last.tobytes(), p.check_state(now)))
        if append:
            p.eng.append_workers(_cols(append))
        if change:
            p.eng.liveness_set([SOAK_ROWS[change[0]]], [change[1]])
    seen = {c for got, _v, _s in log for c in got}
    p.close()
    return log, seen


def test_soak_against_the_model_twice():
    first, seen = _soak()
    assert seen == set(range(A.N_CODES))
    second, _ = _soak()
    assert first == second  # the verdicts' bytes and every read-out, run to run


# ---- errors and state

def test_state_and_argument_errors():
    L = E.lib()
    p = Pair(30, {0: 3, 1: 4, 2: 5, 3: 6, 4: 7}, on=False)
    eng = p.eng
    packed, _ = _pack([AC.ok(0, 1, beat=True), AC.ok(1, 2)], T0, p.rows)
    buf, off, sigs, claimed, flags, ts, nbuf, noff = packed
    out, counts = np.zeros(2, dtype=E.RQ_VERDICT), np.zeros(E.AD_N_CODES, dtype=np.uint32)

    def call(f=flags, t=ts, nb=nbuf, no=noff, o=off):
        return L.pm_admit_requests(eng._h, T0, buf.ctypes.data, o.ctypes.data, sigs.ctypes.data, claimed.ctypes.data,
                                   None if f is None else f.ctypes.data, None if t is None else t.ctypes.data,
                                   None if nb is None else nb.ctypes.data, None if no is None else no.ctypes.data, 2,
                                   out.ctypes.data, counts.ctypes.data)

    # admission is off: every call says so
    assert call() == ESTATE
    for f in (lambda: eng.admission_rate_get([0]), lambda: eng.admission_rate_set([0], [1], [1]), lambda: eng.admission_nonces(T0),
              lambda: eng.beats_get([0]), lambda: eng.beats_set([0], [1]), lambda: eng.liveness_sweep_beats(T0)):
        assert _code(f) == ESTATE
    # it needs the book
    eng.enable_addresses(False)
    assert _code(lambda: eng.enable_admission(True)) == ESTATE
    eng.enable_addresses(True)
    p.place()
    eng.enable_admission(True)
    assert call() == 0 and out["code"].tolist() == [E.RQ_OK, E.RQ_OK]
    before = p.readout(T0)
    assert before[2] == (2, 2) and before[3][3] == T0
    # what a call refuses, and that a refused call leaves the three ledgers as they were
    down = np.array([0, 20, 19], dtype=np.uint32)
    assert call(no=down) == EINVAL and call(o=down) == EINVAL
    assert call(t=None) == EINVAL and call(no=None) == EINVAL and call(nb=None) == EINVAL and call(f=None, t=None) == EINVAL
    assert _code(lambda: eng.admission_rate_get([30])) == ERANGE and _code(lambda: eng.admission_rate_set([0, 30], [1, 1], [1, 1])) == ERANGE
    assert _code(lambda: eng.beats_get([30])) == ERANGE and _code(lambda: eng.beats_set([30], [5])) == ERANGE
    assert p.readout(T0) == before
    # NULL columns go with their flags on every request
    all_flags = flags | np.uint8(E.RQ_FLAG_NO_TIMESTAMP | E.RQ_FLAG_NO_NONCE)
    assert call(f=all_flags, t=None, nb=None, no=None) == 0 and out["code"].tolist() == [E.RQ_NO_NONCE] * 2
    # an index given twice takes its last entry
    eng.admission_rate_set([4, 5, 4], [10, 20, 30], [1, 2, 3])
    assert _rate(eng, [4, 5]) == ([30, 20], [3, 2])
    eng.beats_set([9, 9], [5, 4])
    assert eng.beats_get([9]).tolist() == [4]
    # n == 0 is a no-op; the sweep keeps its own refusal
    v, c = eng.admit_requests(AD.pack_admissions([]), T0)
    assert len(v) == 0 and c.tolist() == [0] * E.AD_N_CODES
    assert _code(lambda: eng.liveness_sweep(T0, None)) == EINVAL
    eng.liveness_sweep_beats(T0)
    # off releases everything; on again starts empty
    eng.enable_admission(False)
    assert call() == ESTATE
    eng.enable_admission(True)
    assert eng.admission_nonces(T0) == (0, 0) and eng.beats_get([3]).tolist() == [0]
    # liveness off: BANNED and EJECTED are never given
    eng.liveness_enable(False)
    p.model = A.Model()
    assert _code(lambda: eng.liveness_sweep_beats(T0)) == ESTATE
    v, _c = eng.admit_requests(_pack([(3, A.OK, 0, AC.nonce(7), True), (4, A.OK, 0, AC.nonce(8), True)], T0, p.rows)[0], T0)
    assert v["code"].tolist() == [E.RQ_OK] * 2 and v["status"].tolist() == [0xFF] * 2 and eng.beats_get([6, 7]).tolist() == [T0, T0]
    p.close()


def test_refused_inside_a_stepwise_tick():
    sw = make_swarm(11, 60, 200)
    p = Pair(8, {0: 3, 1: 4, 2: 5, 3: 6, 4: 7}, liveness=False)
    eng = p.eng
    host.load_swarm(eng, sw)
    p.place()
    assert p.admit(T0, [AC.ok(0, 1, beat=True)]) == [A.OK]
    eng.dist_configure(0, 1)
    eng.dist_tick_begin()
    packed, _ = _pack([AC.ok(0, 2)], T0, p.rows)
    for f in (lambda: eng.admit_requests(packed, T0), lambda: eng.admission_rate_get([0]), lambda: eng.admission_nonces(T0),
              lambda: eng.beats_get([0]), lambda: eng.enable_admission(True)):
        assert _code(f) == ESTATE
    eng.dist_carve_wait()
    eng.dist_match_begin()
    eng.dist_tick_end()
    assert p.admit(T0, [AC.ok(0, 1), AC.ok(0, 2)]) == [A.REPLAY, A.OK]
    p.close()


def test_admission_changes_nothing_a_tick_publishes():
    W = 600
    sw = make_swarm(13, 120, W)

    def leg(with_admission):
        eng = E.Engine(device=0, group_id_seed=7)
        host.load_swarm(eng, sw)
        eng.liveness_enable(True)
        eng.enable_addresses(True)
        eng.set_addresses(0, make_addresses(5, W, "uniform"))
        eng.set_addresses(3, [ADDR[0]])
        eng.tick()
        first = _published(eng, W)
        if with_admission:
            eng.enable_admission(True)
            packed, _ = _pack([AC.ok(0, 1, beat=True), AC.ok(0, 1), (5, A.UNKNOWN, 0, AC.nonce(2), False)], T0, {0: 3})
            v, _c = eng.admit_requests(packed, T0)
            assert v["code"].tolist() == [E.RQ_OK, E.RQ_REPLAY, E.RQ_UNKNOWN]
            eng.admission_rate_set([5], [T0], [9])
            eng.beats_set([6], [T0])
        eng.tick()
        second = _published(eng, W)
        status = eng.liveness_get()
        eng.close()
        return first, second, status[0].tolist(), status[1].tolist()

    assert leg(True) == leg(False)
