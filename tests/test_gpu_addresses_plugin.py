"""The C++ plugin over the real engine with the address book on (pmx_enable_address_book of pm_plugin_c.h): on make_swarm's
digit-only addresses it reads exactly as with the book off; on lower-case spellings of letter-led addresses every rendered
address is the EIP-55 text and every rendered GROUP_INDEX the model's (tests/addresses_model.py), which a plugin that ranked
the texts it was given would not produce."""
import ctypes as C

import numpy as np
import pytest

from protocol_amd.addresses import make_addresses
from protocol_amd.swarm import make_swarm

from plugin_cxx import PluginCxx, _check, _text, plugin_lib

import addresses_model as M

pytestmark = pytest.mark.gpu
ENV = {"IDX": "${GROUP_INDEX}/${GROUP_SIZE}", "NEXT": "${NEXT_P2P_ADDRESS}"}


def bind(L):
    vp, sz, s, u32, u64 = C.c_void_p, C.c_size_t, C.c_char_p, C.c_uint32, C.c_uint64
    L.pmx_enable_address_book.argtypes = [vp]
    L.pmx_enable_liveness.argtypes = [vp, u32]
    L.pmx_uninvited_nodes.argtypes = [vp, s, sz, C.POINTER(sz)]
    L.pmx_invite_digests.argtypes = [vp, u32, u32, u64, u64, s, sz, C.POINTER(sz)]
    return L


def _plugin(sw, book, addr=None):
    p = PluginCxx(sw)
    if addr is not None:
        p.addr = [a.encode() for a in addr]
        p.node_of_addr = {a: i for i, a in enumerate(addr)}
    if book:
        _check(p.L.pmx_enable_address_book(p._p))
    p.set_clock(1_760_000_000_000)
    p.sync_nodes(range(sw.W), set(range(sw.W)))
    p.sync_tasks(sw.task_masks(), sw.created_at, sw.task_uid, env=ENV)
    p.eng.W = sw.W
    p.tick()
    return p


def _shown(p):
    """what a caller sees: the groups with their nodes, and every node's rendered task"""
    groups = sorted((g["id"], g["config"], tuple(g["nodes"])) for g in p.get_all_groups())
    tasks = []
    for node in range(p.sw.W):
        t = p.task_for_node(node)
        tasks.append(None if t is None else (t["uid"], t["env"]["IDX"], t["env"]["NEXT"]))
    return groups, tasks


def test_book_on_reads_as_book_off_on_digit_only_addresses():
    sw = make_swarm(51, 60, 300, configs="uniform")
    bind(plugin_lib())
    off, on = _plugin(sw, False), _plugin(sw, True)
    a, b = _shown(off), _shown(on)
    assert len(a[0]) >= 10 and any(t is not None for t in a[1])
    assert a == b
    for p in (off, on):
        p.close()


def test_mixed_case_inputs_render_the_models_group_index():
    sw = make_swarm(52, 60, 300, configs="uniform")
    bind(plugin_lib())
    raw = make_addresses(52, sw.W, "letter_led")
    texts = [M.eip55(r.tobytes()) for r in raw]
    given = ["0x" + r.tobytes().hex() if k % 3 else r.tobytes().hex() for k, r in enumerate(raw)]  # lower case, a third without "0x"
    p = _plugin(sw, True, given)
    _, groups, members = p.eng.get_groups()
    want_idx, want_groups, reordered = {}, [], 0
    for g in groups:
        mem = members[int(g["member_begin"]):int(g["member_begin"]) + int(g["n_members"])].tolist()
        by_text = sorted(mem, key=lambda w: texts[w])
        assert mem == by_text                                  # the engine lists them in EIP-55 text order
        reordered += by_text != sorted(mem, key=lambda w: given[w].removeprefix("0x"))
        for k, w in enumerate(by_text):
            want_idx[w] = (k, len(mem), by_text[(k + 1) % len(mem)])
        want_groups.append(tuple(texts[w] for w in by_text))
    assert len(want_groups) >= 10 and reordered >= 3, (reordered, len(want_groups))  # groups the lower-case order lists otherwise
    shown, tasks = _shown(p)
    assert sorted(g[2] for g in shown) == sorted(want_groups)
    served = 0
    for node, t in enumerate(tasks):
        if t is None:
            continue
        k, n, nxt = want_idx[node]
        assert (t[1], t[2]) == ("%d/%d" % (k, n), "p2p-%d" % nxt), node
        served += 1
    assert served >= 20
    # a node is found under any spelling, and shown under the one the device computed
    some = next(iter(want_idx))
    for spelling in (texts[some], texts[some].lower(), texts[some][2:].upper()):
        got = p.get_node_group(spelling)
        assert got is not None and got[0] == want_idx[some][0] and texts[some] in got[1]["nodes"]
    p.close()


def test_invite_digests_of_the_uninvited_nodes():
    sw = make_swarm(53, 10, 40, configs="uniform")
    L = bind(plugin_lib())
    raw = make_addresses(53, sw.W, "uniform")
    p = PluginCxx(sw)
    p.addr = [("0x" + r.tobytes().hex()).encode() for r in raw]
    _check(L.pmx_enable_address_book(p._p))
    _check(L.pmx_enable_liveness(p._p, 3))
    p.sync_nodes(range(sw.W), set(range(0, sw.W, 2)))  # (a row that comes in not Healthy starts in the ledger as Discovered)
    listed = _text(lambda o, c, n: L.pmx_uninvited_nodes(p._p, o, c, n)).split()
    assert listed == [M.eip55(raw[node].tobytes()) for node in range(1, sw.W, 2)]
    text = _text(lambda o, c, n: L.pmx_invite_digests(p._p, 9, 4, 1234, 1_760_000_000, o, c, n))
    lines = [ln.split("\t") for ln in text.splitlines()]
    assert [ln[0] for ln in lines] == listed
    texts = {M.eip55(r.tobytes()): r.tobytes() for r in raw}
    for address, nonce, digest, signing in lines:
        want = M.invite_digest(9, 4, texts[address], bytes.fromhex(nonce), 1_760_000_000)
        assert digest == want.hex() and signing == M.signing_hash(want).hex()
    p.close()
