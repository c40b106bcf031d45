"""tests/discovery_model.py held to the reference: its three tests (discovery/monitor.rs:450-794, as data in
golden/discovery_sync_kats.json), the named cases of tests/discovery_cases.py with their hand-written outcomes, every arm
reached, and the parallel formulation pm_discovery_sync computes equal to the literal sequential pass — on the named cases and
on 400 seeded ones, of which enough must be order-dependent to test the join at all."""
import json
import os

import pytest

import discovery_cases as DC
import discovery_model as M

HERE = os.path.dirname(os.path.abspath(__file__))


def _kats():
    with open(os.path.join(HERE, "golden", "discovery_sync_kats.json")) as f:
        return json.load(f)["kats"]


@pytest.mark.parametrize("kat", _kats(), ids=lambda k: k["name"])
def test_reference_tests(kat):
    status = {n: k for k, n in enumerate(M.STATUS_NAMES)}
    store = M.make_store([M.node(n["address"], status[n["status"]], n["ip_address"], n["port"]) for n in kat["store"]])
    for step in kat["steps"]:
        d = step["discovery"]
        M.sync_single_node(store, M.sighting(d["id"], d["ip_address"], d["port"], d["is_validated"], d["is_provider_whitelisted"],
                                             d["is_active"]), DC.NOW_MS, kat["max_healthy_nodes_with_same_endpoint"])
        for address, want in step["after"].items():
            if want is None:
                assert address not in store
                continue
            assert M.STATUS_NAMES[store[address]["status"]] == want["status"]
            if "ip_address" in want:
                assert store[address]["ip_address"] == want["ip_address"]


def _check_equal(store, discovery, now, max_same, tag):
    seq, seq_status, seq_ep, after, abi, outs = M.run_sequential(store, discovery, now, max_same)
    par, par_status, par_ep, _ = M.parallel_pass(abi["status"], abi["row_endpoint"], abi["rows"], now, max_same)
    assert par == seq, tag
    assert par_status == seq_status and par_ep == seq_ep, tag
    stamp_now = {abi["addresses"][r[0]]: bool(res["ops"] & M.DO_STAMP_NOW) for r, res in zip(abi["rows"], par) if r[0] != M.DISC_NEW}
    for address, flag in stamp_now.items():                              # the stamp: now, or the snapshot's
        assert after[address]["last_status_change"] == (now if flag else store[address]["last_status_change"]), tag
    return seq, abi, outs


@pytest.mark.parametrize("case", DC.CASES, ids=lambda c: c["name"])
def test_named_case(case):
    store = M.make_store(case["store"])
    seq, abi, outs = _check_equal(store, case["discovery"], case["now"], case["max"], case["name"])
    after = {a: dict(n) for a, n in store.items()}
    M.sequential_pass(after, case["discovery"], case["now"], case["max"])
    for d, res, (final, updates, ip) in zip(case["discovery"], seq, case["want"]):
        if final == "skip":
            assert res["ops"] == M.DO_SKIP and d["id"] not in after
        elif final == "admit":
            assert res["ops"] == M.DO_ADMIT and after[d["id"]]["status"] == M.DISCOVERED and after[d["id"]]["ip_address"] == ip
        else:
            assert (res["final_status"], res["updates"]) == (final, updates)
            assert after[d["id"]]["ip_address"] == ip and after[d["id"]]["port"] == store[d["id"]]["port"]
        assert len(res["updates"]) <= 3


def test_every_arm_is_reached_by_a_named_case():
    seen = set()
    for case in DC.CASES:
        for o in M.sequential_pass(M.make_store(case["store"]), case["discovery"], case["now"], case["max"]):
            assert set(o["arms"]) <= set(M.ARMS)
            seen |= set(o["arms"])
    assert seen == set(M.ARMS)


def test_seeded_cases_and_their_order_dependence():
    rows = order_dependent = 0
    for seed in range(M.N_SEEDED):
        store, discovery, now, max_same = M.seeded_case(seed)
        seq, abi, _ = _check_equal(store, discovery, now, max_same, "seed %d" % seed)
        rows += len(seq)
        order_dependent += M.count_once_differs(abi["status"], abi["row_endpoint"], abi["rows"], seq, max_same)
    print("rows", rows, "order-dependent", order_dependent)
    assert order_dependent >= 100, "the generator does not reach the join: %d of %d rows" % (order_dependent, rows)
