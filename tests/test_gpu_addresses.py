"""The address book on the GPU (pm_addresses_*, pm_keccak256_many, pm_invite_digests of include/pm_engine.h; kernels in
pm_keccak.inc and pm_addresses.inc) against tests/keccak_model.py and tests/addresses_model.py, which test_addresses_model.py
holds to hashlib and to the EIP-55 known answers.

Where thousands of texts are needed they come from pm_host_eip55 (a loop-and-array implementation written apart from the device's
unrolled one, held to the model on the CPU), and the model takes a sample: the Python sponge is a millisecond a call.  The ranks
are always the model's sort of texts with its row tie-break."""
import json
import os
import re

import numpy as np
import pytest

from protocol_amd import build as B
from protocol_amd import engine as E
from protocol_amd import host
from protocol_amd.addresses import make_addresses
from protocol_amd.swarm import make_swarm

import addresses_cases as AC
import addresses_model as M
import keccak_model as K

pytestmark = pytest.mark.gpu
EINVAL, ESTATE, ERANGE = -1, -4, -5
ON = E.W_HEALTHY | E.W_HAS_P2P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "eip55_kats.json")))
LADDER = (0, 1, 135, 136, 137, 148, 271, 272, 273)


def _sort_sizes():
    """what launch_ro_radix_pass works in, read from the device source: the keys of a chunk, and the entries of a tile of the
    scan that runs over its 256 x chunks histogram -> the smallest W with two chunks, and the smallest whose histogram has two tiles"""
    dev = open(os.path.join(B.CSRC, "pm_device.h")).read()
    chunk = int(re.search(r"\bPM_RO_CHUNK\s*=\s*(\d+)", dev).group(1))
    ro = open(os.path.join(B.CSRC, "pm_rollout.inc")).read()
    body = ro[ro.index("void launch_ro_radix_pass("):]
    body = body[:body.index("\n}\n")]
    assert "(N + PM_RO_CHUNK - 1u) / PM_RO_CHUNK" in body and "launch_mx_scan(hist, 256u * chunks" in body
    mx = open(os.path.join(B.CSRC, "pm_metrics.inc")).read()
    scan = mx[mx.index("void mx_scan_kernel("):mx.index("void mx_copy_kernel(")]
    tile = int(re.search(r"base \+= (\d+)u", scan).group(1))
    assert tile % 256 == 0
    return chunk + 1, (tile // 256) * chunk + 1


TWO_CHUNKS, TWO_TILES = _sort_sizes()
RANK_W = [1, 2, 63, 64, 65, TWO_CHUNKS, TWO_TILES, 5003]


def _cols(n, flags=ON):
    z = np.zeros(n, dtype=np.uint32)
    return dict(flags=np.full(n, flags, dtype=np.uint32), gpu_count=z, gpu_mem_mb=z, gpu_model_class=z, cpu_cores=z, ram_mb=z,
                storage_gb=z, price=z, lat=np.zeros(n), lon=np.zeros(n))


def _code(call):
    with pytest.raises(E.EngineError) as ei:
        call()
    return ei.value.code


def _book(n):
    eng = E.Engine(device=0)
    eng.upload_workers(_cols(n))
    eng.enable_addresses(True)
    return eng


def _texts(addrs):
    return [E.host_eip55(r.tobytes()) for r in addrs]


def _want_ranks(addrs):
    return M.ranks_of_texts(_texts(addrs))


@pytest.fixture(scope="module")
def eng1():
    eng = _book(1)
    yield eng
    eng.close()


# ---- keccak-256

def _msg(n, salt=0):
    return bytes((i * 7 + n + salt * 13) & 255 for i in range(n))


def test_keccak_length_ladder_against_the_model(eng1):
    msgs = [_msg(n) for n in LADDER]
    got = eng1.keccak256_many(msgs)
    for m, d in zip(msgs, got):
        assert d.tobytes() == K.keccak256(m), len(m)
    assert got[0].tobytes().hex() == "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"
    assert got[0].tobytes() != K.sha3_256(b"")  # (what a SHA-3-padded sponge would give)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_keccak_batches_of_mixed_lengths(eng1, n):
    rng = np.random.default_rng(n)
    lens = rng.choice(np.array(LADDER + (7, 40, 60, 408, 409, 700)), size=n)
    msgs = [rng.integers(0, 256, size=int(k), dtype=np.uint8).tobytes() for k in lens]
    got = eng1.keccak256_many(msgs)
    assert got.shape == (n, 32)
    for m, d in zip(msgs, got):
        assert d.tobytes() == E.host_keccak256(m), len(m)
    for k in rng.choice(n, size=min(n, 8), replace=False):
        assert got[k].tobytes() == K.keccak256(msgs[k])
    assert np.array_equal(got, eng1.keccak256_many(msgs))


def test_keccak_empty_batch_and_bad_offsets(eng1):
    assert eng1.keccak256_many([]).shape == (0, 32)
    off = np.array([0, 4, 2], dtype=np.uint32)
    buf, out = np.zeros(8, dtype=np.uint8), np.zeros(64, dtype=np.uint8)
    assert E.lib().pm_keccak256_many(eng1._h, buf.ctypes.data, off.ctypes.data, 2, out.ctypes.data) == EINVAL
    eng = E.Engine(device=0)  # no workers, no book
    assert eng.keccak256_many([b"abc"])[0].tobytes() == K.keccak256(b"abc")
    eng.close()


# ---- texts

def test_texts_of_the_known_answers():
    texts = KATS["eip55"] + KATS["reference_checksummed"]
    eng = _book(len(texts))
    eng.set_addresses(0, [bytes.fromhex(t[2:]) for t in texts])
    assert eng.address_texts() == texts
    rows = [len(texts) - 1, 0, 3, 3]
    assert eng.address_texts(rows) == [texts[r] for r in rows]
    assert eng.address_texts(n=2) == texts[:2] and eng.address_texts([]) == []
    eng.close()


def test_texts_of_generated_addresses():
    addrs = np.concatenate([make_addresses(31, 700, "uniform"), make_addresses(31, 300, "letter_led")])
    eng = _book(len(addrs))
    eng.set_addresses(0, addrs)
    got = eng.address_texts()
    assert got == _texts(addrs)
    for k in np.random.default_rng(1).choice(len(addrs), size=50, replace=False):
        assert got[k] == M.eip55(addrs[k].tobytes())
    eng.close()


# ---- ranks

def _rank_check(eng, addrs, deep, tag=""):
    before = eng.debug_address_sorts()
    got = eng.rank_addresses()
    after = eng.debug_address_sorts()
    assert got.tolist() == _want_ranks(addrs), tag
    assert (after["deep"] - before["deep"], after["shallow"] - before["shallow"]) == ((1, 0) if deep else (0, 1)), tag
    return got


@pytest.mark.parametrize("W", RANK_W)
def test_ranks_of_uniform_addresses_take_the_one_word_sort(W):
    addrs = make_addresses(40 + W, W, "uniform")
    assert len({t[2:12] for t in _texts(addrs)}) == W
    eng = _book(W)
    eng.set_addresses(0, addrs)
    first = _rank_check(eng, addrs, deep=False)
    assert np.array_equal(first, eng.rank_addresses())  # (two calls: the same bits)
    eng.close()


@pytest.mark.parametrize("W", [65, TWO_CHUNKS, 5003])
def test_ranks_of_letter_led_addresses(W):
    addrs = make_addresses(50 + W, W, "letter_led")
    heads = [t[2:12] for t in _texts(addrs)]
    eng = _book(W)
    eng.set_addresses(0, addrs)
    got = _rank_check(eng, addrs, deep=len(set(heads)) < W)
    assert got.tolist() != M.ranks_of_texts([t.lower() for t in _texts(addrs)])  # (the lower-case order is another one)
    eng.close()


@pytest.mark.parametrize("variant", ["prefix10", "prefix20", "prefix39", "duplicates"])
@pytest.mark.parametrize("W", [65, TWO_CHUNKS, TWO_TILES])
def test_ranks_of_shared_prefixes_take_the_all_words_sort(W, variant):
    addrs = make_addresses(60 + W, W, variant)
    eng = _book(W)
    eng.set_addresses(0, addrs)
    first = _rank_check(eng, addrs, deep=True)
    assert sorted(first.tolist()) == list(range(W))
    assert np.array_equal(first, eng.rank_addresses())
    eng.close()


@pytest.mark.parametrize("name", sorted(AC.CASES))
def test_ranks_of_the_named_cases(name):
    addrs = AC.CASES[name]()
    eng = _book(len(addrs))
    eng.set_addresses(0, addrs)
    got = _rank_check(eng, addrs, deep=name in AC.DEEP, tag=name)
    assert got.tolist() == M.ranks(addrs)  # (small enough for the model's own texts)
    eng.close()


def test_rewrite_a_row_and_append_rows():
    W = 200
    addrs = make_addresses(70, W + 60, "letter_led")
    eng = _book(W)
    eng.set_addresses(0, addrs[:W])
    _rank_check(eng, addrs[:W], deep=False)
    cur = addrs[:W].copy()
    cur[17] = addrs[W + 59]          # a row takes another address
    cur[18] = cur[3]                 # ... and one a duplicate of an earlier row's: the all-words sort
    eng.set_addresses(17, cur[17:19])
    _rank_check(eng, cur, deep=True)
    eng.append_workers(_cols(50))
    assert _code(eng.rank_addresses) == ESTATE  # the new rows hold no address yet
    assert eng.address_texts(n=W) == _texts(cur)
    eng.set_addresses(W, addrs[W:W + 50])
    _rank_check(eng, np.concatenate([cur, addrs[W:W + 50]]), deep=True)
    eng.set_addresses(18, addrs[18:19])  # the duplicate goes
    _rank_check(eng, np.concatenate([cur[:18], addrs[18:19], cur[19:], addrs[W:W + 50]]), deep=False)
    eng.close()


def test_rank_out_is_the_engines_column():
    """the node directory's BY_ADDRESS order reads the column the tick reads; pm_set_addr_ranks afterwards wins"""
    W = 300
    addrs = make_addresses(71, W, "letter_led")
    eng = E.Engine(device=0, group_id_seed=3)
    cfg_rows, alt_rows, _ = host.pack_configs([("any", 1, 8, None)])
    eng.set_configs(cfg_rows, alt_rows)
    eng.upload_workers(_cols(W))
    eng.upload_tasks(np.full(3, 1, dtype=np.uint64), np.array([3, 2, 1], dtype=np.int64), np.array([11, 12, 13], dtype=np.uint64))
    eng.liveness_enable(True)
    eng.enable_addresses(True)
    eng.set_addresses(0, addrs)
    got = eng.rank_addresses()
    assert eng.rank_addresses(want=False) is None
    _, _, rows = eng.directory(order=E.DIR_BY_ADDRESS)
    assert rows["worker"].tolist() == np.argsort(got, kind="stable").tolist()
    eng.set_addr_ranks(np.arange(W, dtype=np.uint32)[::-1].copy())
    _, _, rows = eng.directory(order=E.DIR_BY_ADDRESS)
    assert rows["worker"].tolist() == list(range(W))[::-1]
    eng.rank_addresses()
    _, _, rows = eng.directory(order=E.DIR_BY_ADDRESS)
    assert rows["worker"].tolist() == np.argsort(got, kind="stable").tolist()
    eng.close()


# ---- state and errors

def test_book_off_and_unset_rows_and_ranges():
    W = 10
    addrs = make_addresses(72, W, "uniform")
    eng = E.Engine(device=0)
    eng.upload_workers(_cols(W))
    nonce, exp = np.zeros((1, 32), dtype=np.uint8), [1]
    for call in (lambda: eng.set_addresses(0, addrs), eng.rank_addresses, lambda: eng.address_texts([0]),
                 lambda: eng.address_texts([]), lambda: eng.invite_digests(1, 1, [0], nonce, exp)):
        assert _code(call) == ESTATE  # the book is off
    eng.enable_addresses(True)
    assert _code(eng.rank_addresses) == ESTATE          # no row holds an address
    assert _code(lambda: eng.address_texts([0])) == ESTATE
    eng.set_addresses(0, addrs[:0])                     # n == 0: a no-op
    eng.set_addresses(1, addrs[1:])
    assert _code(eng.rank_addresses) == ESTATE          # row 0 still holds none
    assert _code(lambda: eng.address_texts()) == ESTATE
    assert _code(lambda: eng.invite_digests(1, 1, [0], nonce, exp)) == ESTATE
    assert eng.address_texts([1, 9]) == _texts(addrs[[1, 9]])
    assert _code(lambda: eng.set_addresses(W, addrs[:1])) == ERANGE
    assert _code(lambda: eng.set_addresses(W - 1, addrs[:2])) == ERANGE
    assert _code(lambda: eng.set_addresses(0xFFFFFFFF, addrs[:2])) == ERANGE
    assert _code(lambda: eng.address_texts([W])) == ERANGE
    assert _code(lambda: eng.address_texts(n=W + 1)) == ERANGE
    assert _code(lambda: eng.invite_digests(1, 1, [W], nonce, exp)) == ERANGE
    assert E.lib().pm_addresses_set(eng._h, 0, None, 1) == EINVAL
    eng.set_addresses(0, addrs[:1])
    assert eng.rank_addresses().tolist() == _want_ranks(addrs)
    d, s = eng.invite_digests(1, 1, [], np.zeros((0, 32), dtype=np.uint8), [])
    assert d.shape == s.shape == (0, 32)
    eng.close()


def test_upload_rules_and_enable_again():
    W = 40
    addrs = make_addresses(73, W + 8, "uniform")
    eng = _book(W)
    eng.set_addresses(0, addrs[:W])
    want = _want_ranks(addrs[:W])
    assert eng.rank_addresses().tolist() == want
    eng.upload_workers(_cols(W + 8), keep_groups=True)   # keep_groups = 1: the addresses stay, the new rows hold none
    assert _code(eng.rank_addresses) == ESTATE
    assert eng.address_texts(n=W) == _texts(addrs[:W])
    assert _code(lambda: eng.address_texts([W])) == ESTATE
    eng.set_addresses(W, addrs[W:])
    assert eng.rank_addresses().tolist() == _want_ranks(addrs)
    eng.upload_workers(_cols(W))                         # keep_groups = 0: every address is forgotten
    assert _code(eng.rank_addresses) == ESTATE
    assert _code(lambda: eng.address_texts([0])) == ESTATE
    eng.set_addresses(0, addrs[:W])
    assert eng.rank_addresses().tolist() == want
    eng.enable_addresses(False)                          # off frees the book
    assert _code(eng.rank_addresses) == ESTATE
    eng.enable_addresses(True)                           # on again: empty
    assert _code(eng.rank_addresses) == ESTATE
    eng.set_addresses(0, addrs[:W])
    assert eng.rank_addresses().tolist() == want
    eng.enable_addresses(True)                           # on while on: emptied
    assert _code(lambda: eng.address_texts([0])) == ESTATE
    eng.close()


def test_enable_before_the_workers():
    eng = E.Engine(device=0)
    eng.enable_addresses(True)
    assert _code(eng.rank_addresses) == ESTATE           # no worker table yet
    eng.upload_workers(_cols(3))
    addrs = make_addresses(74, 3, "uniform")
    eng.set_addresses(0, addrs)
    assert eng.rank_addresses().tolist() == M.ranks(addrs)
    eng.close()


def test_every_call_is_refused_inside_a_stepwise_tick():
    sw = make_swarm(11, 60, 200)
    addrs = make_addresses(78, sw.W, "uniform")
    eng = E.Engine(device=0)
    host.load_swarm(eng, sw)
    eng.enable_addresses(True)
    eng.set_addresses(0, addrs)
    want = eng.rank_addresses()
    nonce = np.zeros((1, 32), dtype=np.uint8)
    eng.dist_configure(0, 1)
    eng.dist_tick_begin()
    for call in (lambda: eng.enable_addresses(True), lambda: eng.enable_addresses(False), lambda: eng.set_addresses(0, addrs[:1]),
                 eng.rank_addresses, lambda: eng.address_texts([0]), lambda: eng.keccak256_many([b"abc"]),
                 lambda: eng.invite_digests(1, 1, [0], nonce, [1])):
        assert _code(call) == ESTATE
    eng.dist_carve_wait()
    eng.dist_match_begin()
    eng.dist_tick_end()
    assert np.array_equal(eng.rank_addresses(), want) and eng.address_texts([3]) == _texts(addrs[3:4])  # the book is as it was
    assert eng.keccak256_many([b"abc"])[0].tobytes() == K.keccak256(b"abc")
    eng.close()


# ---- end to end: the tick's published rows under the book's ranks, under the model's, and under the lower-case order

def _published(eng, W):
    rows = []
    for w in range(W):
        a = eng.lookup(w)
        rows.append((a.task, a.group_index, a.group_size, a.next_worker, a.group_id))
    return rows


def _groups(eng):
    _, groups, members = eng.get_groups()
    return [(int(g["id"]), int(g["config"]), members[int(g["member_begin"]):int(g["member_begin"]) + int(g["n_members"])].tolist())
            for g in groups]


def test_tick_under_book_ranks_is_tick_under_model_ranks():
    W = 1500
    sw = make_swarm(9, 400, W, configs="uniform")
    big = sum(1 << i for i, c in enumerate(sw.configs) if c[1] >= 4)
    assert big
    addrs = make_addresses(75, W, "letter_led")
    texts = _texts(addrs)
    for k in np.random.default_rng(2).choice(W, size=20, replace=False):
        assert texts[k] == M.eip55(addrs[k].tobytes())
    by_text, by_lower = M.ranks_of_texts(texts), M.ranks_of_texts([t.lower() for t in texts])

    def leg(rank_it):
        eng = E.Engine(device=0, group_id_seed=5)
        host.load_swarm(eng, sw, enabled=sw.enabled_mask() & big)
        rank_it(eng)
        eng.tick()
        _, _, rows, members = eng.group_directory()
        listed = [members[int(r["member_begin"]):int(r["member_begin"]) + int(r["size"])].tolist() for r in rows]
        out = (_groups(eng), _published(eng, W), listed)
        eng.close()
        return out

    def through_the_book(eng):
        eng.enable_addresses(True)
        eng.set_addresses(0, addrs)
        assert eng.rank_addresses().tolist() == by_text

    book = leg(through_the_book)
    model = leg(lambda eng: eng.set_addr_ranks(np.array(by_text, dtype=np.uint32)))
    lower = leg(lambda eng: eng.set_addr_ranks(np.array(by_lower, dtype=np.uint32)))
    groups = book[0]
    assert len(groups) >= 20 and all(len(m) >= 4 for _, _, m in groups)
    # the inputs can tell the orders apart: by the model, at least 30 % of the groups list their members differently
    differ = sum(sorted(m, key=lambda w: by_text[w]) != sorted(m, key=lambda w: by_lower[w]) for _, _, m in groups)
    assert differ >= 0.3 * len(groups), (differ, len(groups))
    for gid, _, m in groups:
        assert m == sorted(m, key=lambda w: by_text[w])  # (members come in BTreeSet order)
    assert book[0] == model[0] and book[1] == model[1] and book[2] == model[2]
    assert any(r[1] != 0 for r in book[1])
    assert sorted(map(sorted, (m for _, _, m in lower[0]))) == sorted(map(sorted, (m for _, _, m in groups)))
    assert lower[1] != book[1]  # ... and a host that ranks lower-case text publishes other rows


# ---- invite digests

@pytest.mark.parametrize("n", [1, 64, 65])
def test_invite_digests_against_the_model(n):
    W = 80
    addrs = make_addresses(76, W, "uniform")
    eng = _book(W)
    eng.set_addresses(0, addrs)
    rng = np.random.default_rng(n)
    rows = rng.integers(0, W, size=n)
    rows[-1] = rows[0]  # a row asked twice
    nonces = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    exp = rng.integers(0, 1 << 63, size=n, dtype=np.uint64)
    d, s = eng.invite_digests(0xC0FFEE, 42, rows, nonces, exp)
    for k in range(n):
        want = M.invite_digest(0xC0FFEE, 42, addrs[rows[k]].tobytes(), nonces[k].tobytes(), int(exp[k]))
        assert d[k].tobytes() == want and s[k].tobytes() == M.signing_hash(want), k
    d2, s2 = eng.invite_digests(0xC0FFEE, 42, rows, nonces, exp)
    assert np.array_equal(d, d2) and np.array_equal(s, s2)
    eng.close()


def test_invite_digests_at_the_ends_of_every_field():
    addrs = make_addresses(77, 4, "uniform")
    eng = _book(4)
    eng.set_addresses(0, addrs)
    ends32, ends64 = (0, 1, 0xFFFFFFFF), (0, 1, 0xFFFFFFFFFFFFFFFF)
    nonce = np.arange(32, dtype=np.uint8)
    for dom in ends32:
        for pool in ends32:
            exp = np.array(ends64, dtype=np.uint64)
            d, s = eng.invite_digests(dom, pool, [2, 2, 1], np.stack([nonce, nonce, nonce]), exp)
            for k, row in enumerate((2, 2, 1)):
                want = M.invite_digest(dom, pool, addrs[row].tobytes(), nonce.tobytes(), ends64[k])
                assert d[k].tobytes() == want and s[k].tobytes() == M.signing_hash(want), (dom, pool, k)
    eng.close()
