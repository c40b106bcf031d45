"""The request gate on the GPU (pm_ecrecover_many, pm_verify_requests of include/pm_engine.h; kernels in pm_secp256k1.inc)
against the big-integer model (tests/secp256k1_model.py).  Integers only: every comparison is equality.

The EIP-191 hash has no call of its own: a request is signed over the MODEL's hash, so the address the gate recovers is the
signer's exactly when the device hashed the same bytes — a decimal length of the wrong width, or a block edge missed, recovers
some other key's address."""
import functools
import hashlib

import numpy as np
import pytest

from protocol_amd import engine as E
from protocol_amd import gate as G
from protocol_amd import host
from protocol_amd.addresses import make_addresses
from protocol_amd.swarm import make_swarm

import gate_cases as GC
import secp256k1_model as M
from test_gpu_addresses import TWO_CHUNKS

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -4
ON = E.W_HEALTHY | E.W_HAS_P2P
NONE = 0xFFFFFFFF
KEYS = [int.from_bytes(hashlib.sha256(b"gate signer %d" % i).digest(), "big") % (M.N - 1) + 1 for i in range(6)]
ADDR = [M.address_of_key(k) for k in KEYS]
# message lengths: where the decimal length gains a digit, and where the prefixed message (26 bytes + the digits + the message)
# ends one short of, on, and one past a keccak block edge (135, 136, 137 and 271, 272, 273 bytes)
LADDER = (0, 9, 10, 99, 100, 999, 1000, 106, 107, 108, 242, 243, 244)


def _cols(n, flags=ON):
    z = np.zeros(n, dtype=np.uint32)
    return dict(flags=np.full(n, flags, dtype=np.uint32), gpu_count=z, gpu_mem_mb=z, gpu_model_class=z, cpu_cores=z, ram_mb=z,
                storage_gb=z, price=z, lat=np.zeros(n), lon=np.zeros(n))


def _code(call):
    with pytest.raises(E.EngineError) as ei:
        call()
    return ei.value.code


def _msg(n, salt=0):
    return bytes((i * 11 + n + salt * 29) & 255 for i in range(n))


@functools.lru_cache(maxsize=None)
def _signed(key_i: int, msg: bytes) -> bytes:
    return M.sig65(*M.sign(KEYS[key_i], M.eip191(msg)))


def _req(key_i, msg, claimed=None):
    return (msg, _signed(key_i, msg), ADDR[key_i] if claimed is None else claimed)


def _want(reqs, flags, book, status):
    """the model's verdicts: book = the rows' addresses (None: the row holds none), status = the ledger's bytes or None"""
    out = []
    for k, (msg, sig, claimed) in enumerate(reqs):
        if M.parity_of_v(sig[64]) is None:
            out.append((E.RQ_BAD_SIGNATURE, NONE, 0xFF, bytes(20)))
            continue
        ok, addr, _ = GC.expected(M.eip191(msg), sig)
        if not ok:
            out.append((E.RQ_NO_KEY, NONE, 0xFF, bytes(20)))
            continue
        if flags is not None and flags[k] & 1:
            out.append((E.RQ_BAD_ADDRESS, NONE, 0xFF, addr))
            continue
        row = next((w for w, a in enumerate(book) if a == addr), NONE)
        st = int(status[row]) if row != NONE and status is not None else 0xFF
        if addr != claimed:
            code = E.RQ_MISMATCH
        elif row == NONE:
            code = E.RQ_UNKNOWN
        elif st == E.NS_EJECTED:
            code = E.RQ_EJECTED
        elif st == E.NS_BANNED:
            code = E.RQ_BANNED
        else:
            code = E.RQ_OK
        out.append((code, row, st, addr))
    return out


def _verify(eng, reqs, flags=None):
    packed = list(G.pack_requests(reqs))
    packed[4] = None if flags is None else np.asarray(flags, dtype=np.uint8)
    v, counts = eng.verify_requests(tuple(packed))
    got = [(int(r["code"]), int(r["row"]), int(r["status"]), r["address"].tobytes()) for r in v]
    assert counts.tolist() == np.bincount([g[0] for g in got], minlength=E.RQ_N_CODES).tolist()  # the device's census
    return got


def _book(W, placed, seed=1):
    """an engine whose book holds make_addresses(seed, W) with `placed` {row: address} on top -> (engine, the rows' addresses)"""
    eng = E.Engine(device=0)
    eng.upload_workers(_cols(W))
    eng.enable_addresses(True)
    addrs = make_addresses(seed, W, "uniform")
    for row, a in placed.items():
        addrs[row] = np.frombuffer(a, dtype=np.uint8)
    eng.set_addresses(0, addrs)
    return eng, [r.tobytes() for r in addrs]


@pytest.fixture(scope="module")
def bare():
    eng = E.Engine(device=0)
    yield eng
    eng.close()


# ---- recovery

def _recover(eng, entries, want_pub=True):
    h = np.frombuffer(b"".join(z for z, _ in entries), dtype=np.uint8).reshape(-1, 32)
    s = np.frombuffer(b"".join(g for _, g in entries), dtype=np.uint8).reshape(-1, 65)
    return eng.ecrecover_many(h, s, want_pub=want_pub)


def test_every_named_case_against_the_model(bare):
    named = GC.named()
    ok, addr, pub = _recover(bare, list(named.values()))
    for k, name in enumerate(named):
        want = GC.expected(*named[name])
        assert (int(ok[k]), addr[k].tobytes(), pub[k].tobytes()) == want, name
    assert sum(int(x) for x in ok) == len(named) - len(GC.NOT_OK)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_recovery_batches_against_the_model(bare, n):
    entries = GC.batch(n)
    ok, addr, pub = _recover(bare, entries)
    assert len(ok) == n
    for k, (z, sig) in enumerate(entries):
        assert (int(ok[k]), addr[k].tobytes(), pub[k].tobytes()) == GC.expected(z, sig), k
    ok2, addr2 = _recover(bare, entries, want_pub=False)   # pub64_out = NULL
    assert np.array_equal(ok, ok2) and np.array_equal(addr, addr2)
    if n >= 63:
        assert 0 < int(ok.sum()) < n


def test_recovery_needs_no_book_and_its_errors(bare):
    L = E.lib()
    z, sig = GC.named()["low_s"]
    h, s = np.frombuffer(z, dtype=np.uint8), np.frombuffer(sig, dtype=np.uint8)
    a, ok = np.zeros(20, dtype=np.uint8), np.zeros(1, dtype=np.uint8)
    assert L.pm_ecrecover_many(bare._h, None, None, 0, None, None, None) == 0                      # n == 0: a no-op
    for args in ((None, s.ctypes.data, 1, a.ctypes.data, None, ok.ctypes.data), (h.ctypes.data, None, 1, a.ctypes.data, None, ok.ctypes.data),
                 (h.ctypes.data, s.ctypes.data, 1, None, None, ok.ctypes.data), (h.ctypes.data, s.ctypes.data, 1, a.ctypes.data, None, None)):
        assert L.pm_ecrecover_many(bare._h, *args) == EINVAL
    assert L.pm_ecrecover_many(None, h.ctypes.data, s.ctypes.data, 1, a.ctypes.data, None, ok.ctypes.data) == EINVAL
    assert L.pm_ecrecover_many(bare._h, h.ctypes.data, s.ctypes.data, 1, a.ctypes.data, None, ok.ctypes.data) == 0
    assert ok[0] == 1 and a.tobytes() == M.address_of_key(GC.KEY)


# ---- the EIP-191 hash, through the signer's address

def test_eip191_length_ladder():
    eng, book = _book(3, {1: ADDR[0]})
    reqs = [_req(0, _msg(n)) for n in LADDER]
    got = _verify(eng, reqs)
    for n, g in zip(LADDER, got):
        assert g == (E.RQ_OK, 1, 0xFF, ADDR[0]), n
    # one request a call too: offset 0, and the last word of the buffer
    for n in (0, 9, 107, 243):
        assert _verify(eng, [_req(0, _msg(n))]) == [(E.RQ_OK, 1, 0xFF, ADDR[0])], n
    eng.close()


def test_eip191_mixed_lengths_at_unaligned_offsets():
    eng, book = _book(3, {2: ADDR[1]})
    lens = [5, 0, 1, 7, 8, 9, 135, 3, 136, 137, 0, 110, 109, 1000, 2, 243, 63, 64, 65, 10, 99, 100, 31, 999, 4]
    reqs = [_req(1, _msg(n, salt=k)) for k, n in enumerate(lens)]
    offs = np.cumsum([0] + lens)
    assert len({int(o) % 8 for o in offs}) == 8  # every alignment of a message's first byte
    assert _verify(eng, reqs) == [(E.RQ_OK, 2, 0xFF, ADDR[1])] * len(lens)
    eng.close()


# ---- verdicts

def _eight_codes():
    z, bad_r = GC.named()["r_no_x"]
    m = [b"/heartbeat{\"n\":%d}" % k for k in range(12)]
    v29 = bytearray(_signed(0, m[0]))
    v29[64] = 29
    reqs = [(m[0], bytes(v29), ADDR[0]),              # 0 BAD_SIGNATURE
            (m[1], bad_r, ADDR[0]),                   # 1 NO_KEY
            _req(0, m[2]),                            # 2 BAD_ADDRESS (flag)
            _req(0, m[3], claimed=ADDR[1]),           # 3 MISMATCH
            _req(5, m[4]),                            # 4 UNKNOWN
            _req(1, m[5]),                            # 5 EJECTED
            _req(2, m[6]),                            # 6 BANNED
            _req(0, m[7]),                            # 7 OK
            (m[8], bad_r, ADDR[0]),                   # 8 flag + no key: NO_KEY
            (m[9], bytes(v29), ADDR[0]),              # 9 flag + bad v: BAD_SIGNATURE
            _req(1, m[10], claimed=ADDR[0]),          # 10 an ejected node's signature under another address: MISMATCH
            _req(5, m[11])]                           # 11 flag + unknown signer: BAD_ADDRESS
    flags = [0, 0, 1, 0, 0, 0, 0, 0, 1, 1, 0, 1]
    return reqs, flags


def test_all_eight_codes_and_their_precedence():
    eng, book = _book(65, {3: ADDR[0], 10: ADDR[1], 20: ADDR[2]})
    eng.liveness_enable(True)
    eng.liveness_set([10, 20], [E.NS_EJECTED, E.NS_BANNED])
    status, _ = eng.liveness_get()
    reqs, flags = _eight_codes()
    got = _verify(eng, reqs, flags)
    assert got == _want(reqs, flags, book, status)
    assert [g[0] for g in got] == [E.RQ_BAD_SIGNATURE, E.RQ_NO_KEY, E.RQ_BAD_ADDRESS, E.RQ_MISMATCH, E.RQ_UNKNOWN, E.RQ_EJECTED, E.RQ_BANNED,
                                   E.RQ_OK, E.RQ_NO_KEY, E.RQ_BAD_SIGNATURE, E.RQ_MISMATCH, E.RQ_BAD_ADDRESS]
    assert got[7][1:3] == (3, E.NS_HEALTHY) and got[5][1:3] == (10, E.NS_EJECTED) and got[10][1] == 10
    assert _verify(eng, reqs, flags) == got                 # the same from call to call
    assert _verify(eng, reqs) == _want(reqs, None, book, status)  # flags = NULL: no flag
    # liveness off: no EJECTED, no BANNED, no status
    eng.liveness_enable(False)
    off = _verify(eng, reqs, flags)
    assert off == _want(reqs, flags, book, None)
    assert [g[0] for g in off][5:8] == [E.RQ_OK] * 3 and all(g[2] == 0xFF for g in off)
    eng.close()


@pytest.mark.parametrize("W", [1, 65, TWO_CHUNKS])
def test_the_join_finds_the_row(W):
    rows = sorted({0, W // 2, W - 1})
    placed = {row: ADDR[k] for k, row in enumerate(rows)}
    eng, book = _book(W, placed, seed=W)
    reqs = [_req(k, b"/storage%d" % k) for k in range(4)]
    got = _verify(eng, reqs)
    assert got == _want(reqs, None, book, None)
    assert [g[1] for g in got] == rows + [NONE] * (4 - len(rows))
    assert [g[0] for g in got] == [E.RQ_OK] * len(rows) + [E.RQ_UNKNOWN] * (4 - len(rows))
    eng.close()


def test_two_rows_with_one_address_and_rows_without():
    W = 65
    eng = E.Engine(device=0)
    eng.upload_workers(_cols(W))
    eng.enable_addresses(True)
    reqs = [_req(k, b"/heartbeat") for k in range(3)]
    assert [g[:2] for g in _verify(eng, reqs)] == [(E.RQ_UNKNOWN, NONE)] * 3   # an empty book
    book = [None] * W
    for row, k in ((40, 0), (7, 0), (64, 1), (41, 0)):                         # the higher rows first
        eng.set_addresses(row, [ADDR[k]])
        book[row] = ADDR[k]
    got = _verify(eng, reqs)
    assert got == _want(reqs, None, book, None)
    assert [g[:2] for g in got] == [(E.RQ_OK, 7), (E.RQ_OK, 64), (E.RQ_UNKNOWN, NONE)]
    eng.close()


def test_the_index_follows_the_book():
    W = 30
    eng, book = _book(W, {3: ADDR[0]})
    req = [_req(0, b"/heartbeat{}")]
    other = make_addresses(99, 4, "uniform")
    assert _verify(eng, req)[0][:2] == (E.RQ_OK, 3)
    eng.set_addresses(3, other[:1])                       # the row is rewritten: the signer is nobody
    assert _verify(eng, req)[0][:2] == (E.RQ_UNKNOWN, NONE)
    eng.set_addresses(5, [ADDR[0]])
    assert _verify(eng, req)[0][:2] == (E.RQ_OK, 5)
    eng.set_addresses(5, other[1:2])
    first = eng.append_workers(_cols(4))                  # appended rows hold no address yet
    assert first == W and _verify(eng, req)[0][:2] == (E.RQ_UNKNOWN, NONE)
    eng.set_addresses(W + 2, [ADDR[0]])
    assert _verify(eng, req)[0][:2] == (E.RQ_OK, W + 2)
    eng.upload_workers(_cols(W + 4), keep_groups=True)    # keep_groups = 1: the addresses stay
    assert _verify(eng, req)[0][:2] == (E.RQ_OK, W + 2)
    eng.upload_workers(_cols(W + 4))                      # keep_groups = 0: every address is forgotten
    assert _verify(eng, req)[0][:2] == (E.RQ_UNKNOWN, NONE)
    eng.set_addresses(1, [ADDR[0]])
    assert _verify(eng, req)[0][:2] == (E.RQ_OK, 1)
    eng.enable_addresses(True)                            # on while on: emptied
    assert _verify(eng, req)[0][:2] == (E.RQ_UNKNOWN, NONE)
    eng.close()


def test_state_and_argument_errors():
    L = E.lib()
    req = [_req(0, b"abc")]
    buf, off, sigs, claimed, flags = G.pack_requests(req)
    out, counts = np.zeros(2, dtype=E.RQ_VERDICT), np.zeros(E.RQ_N_CODES, dtype=np.uint32)
    call = lambda eng, b=buf.ctypes.data, o=off.ctypes.data, s=sigs.ctypes.data, c=claimed.ctypes.data, n=1, v=out.ctypes.data, \
        k=counts.ctypes.data: L.pm_verify_requests(eng._h, b, o, s, c, None, n, v, k)
    eng = E.Engine(device=0)
    eng.enable_addresses(True)
    assert call(eng) == ESTATE                            # no worker table yet
    eng.enable_addresses(False)
    eng.upload_workers(_cols(4))
    assert call(eng) == ESTATE                            # the book is off
    eng.enable_addresses(True)
    assert call(eng) == 0 and out[0]["code"] == E.RQ_UNKNOWN
    for kw in (dict(o=None), dict(s=None), dict(c=None), dict(v=None), dict(k=None), dict(b=None)):
        assert call(eng, **kw) == EINVAL, kw
    assert L.pm_verify_requests(None, buf.ctypes.data, off.ctypes.data, sigs.ctypes.data, claimed.ctypes.data, None, 1, out.ctypes.data,
                                counts.ctypes.data) == EINVAL
    two = np.array([5, 3, 3], dtype=np.uint32)            # offsets that descend
    sig2, cl2 = np.repeat(sigs, 2, axis=0), np.repeat(claimed, 2, axis=0)
    assert call(eng, o=two.ctypes.data, s=sig2.ctypes.data, c=cl2.ctypes.data, n=2) == EINVAL
    assert L.pm_verify_requests(eng._h, None, None, None, None, None, 0, None, None) == 0   # n == 0: a no-op
    v, c = eng.verify_requests(G.pack_requests([]))
    assert len(v) == 0 and c.tolist() == [0] * E.RQ_N_CODES
    eng.close()


def test_both_calls_are_refused_inside_a_stepwise_tick():
    sw = make_swarm(11, 60, 200)
    eng = E.Engine(device=0)
    host.load_swarm(eng, sw)
    eng.enable_addresses(True)
    eng.set_addresses(0, make_addresses(78, sw.W, "uniform"))
    eng.set_addresses(9, [ADDR[0]])
    req = [_req(0, b"/heartbeat{}")]
    entries = [GC.named()["low_s"]]
    assert _verify(eng, req)[0][:2] == (E.RQ_OK, 9)
    eng.dist_configure(0, 1)
    eng.dist_tick_begin()
    assert _code(lambda: _verify(eng, req)) == ESTATE
    assert _code(lambda: _recover(eng, entries)) == ESTATE
    eng.dist_carve_wait()
    eng.dist_match_begin()
    eng.dist_tick_end()
    assert _verify(eng, req)[0][:2] == (E.RQ_OK, 9)
    assert int(_recover(eng, entries)[0][0]) == 1
    eng.close()


def _published(eng, W):
    rows = []
    for w in range(W):
        a = eng.lookup(w)
        rows.append((a.task, a.group_slot, a.group_index, a.group_size, a.next_worker, a.group_id))
    return rows


def test_the_gate_changes_nothing_a_tick_publishes():
    W = 600
    sw = make_swarm(13, 120, W)
    reqs, flags = _eight_codes()

    def leg(with_gate):
        eng = E.Engine(device=0, group_id_seed=7)
        host.load_swarm(eng, sw)
        eng.liveness_enable(True)
        eng.enable_addresses(True)
        eng.set_addresses(0, make_addresses(5, W, "uniform"))
        eng.set_addresses(3, [ADDR[0]])
        eng.tick()
        first = _published(eng, W)
        if with_gate:
            assert _verify(eng, reqs, flags)[7][:2] == (E.RQ_OK, 3)
            _recover(eng, GC.batch(5))
        eng.tick()
        second = _published(eng, W)
        status = eng.liveness_get()
        eng.close()
        return first, second, status[0].tolist(), status[1].tolist()

    assert leg(True) == leg(False)
