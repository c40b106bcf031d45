"""tests/metrics_model.py against the reference's own tests (tests/golden/metrics_store_kats.json, transcribed from
store/domains/metrics_store.rs:251-446 and api/routes/heartbeat.rs:195-377) and against the hand-written outcomes of
tests/metrics_cases.py — the literal store (strings, one dict per address) and the ledger model (series numbers, beats) both;
the two are held to each other on seeded call sequences.  No GPU."""
import json
import math
import os
import random

import pytest

import metrics_cases as MC
import metrics_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "metrics_store_kats.json")))["kats"]


def _metrics(step):
    return [(m["task_id"], m["label"], m["value"]) for m in step["metrics"]]


@pytest.mark.parametrize("kat", KATS, ids=[k["test"] for k in KATS])
def test_model_gives_what_the_references_tests_assert(kat):
    st = M.Store()
    asserted = 0
    for s in kat["steps"]:
        if s.get("op") == "store":
            st.store_metrics(_metrics(s), s["address"])
        elif s.get("op") == "heartbeat":
            st.heartbeat(s["address"], _metrics(s))
        elif s["expect"] == "node":
            assert st.get_metrics_for_node(s["address"]).get(s["task_id"], {}).get(s["label"]) == s["want"]
        elif s["expect"] == "node_task":
            assert (s["task_id"] in st.get_metrics_for_node(s["address"])) == s["present"]
        elif s["expect"] == "node_empty":
            assert st.get_metrics_for_node(s["address"]) == {}
        elif s["expect"] == "aggregate_for_task":
            assert st.get_aggregate_metrics_for_task(s["task_id"]).get(s["label"]) == s["want"]
        elif s["expect"] == "aggregate_for_all_tasks":
            assert st.get_aggregate_metrics_for_all_tasks().get(s["label"]) == s["want"]
        elif s["expect"] == "aggregate_for_all_tasks_len":
            assert len(st.get_aggregate_metrics_for_all_tasks()) == s["want"]
        else:
            raise AssertionError(s)
        asserted += "expect" in s
    assert asserted >= 2


def test_the_kats_name_the_references_tests():
    assert [k["test"] for k in KATS] == ["test_store_metrics", "test_get_metrics_for_node", "test_store_metrics_value_overwrite",
                                         "test_heartbeat"]


def run_store(ops):
    st = M.Store()
    for op in ops:
        if op[0] == "beat":
            st.heartbeat(op[1], op[2])
        elif op[0] == "store":
            st.store_metrics(op[2], op[1])
        elif op[0] == "manual":
            st.store_manual_metrics(op[1], op[2])
        elif op[0] == "delete":
            st.delete_metric(op[1], op[2], op[3])
        elif op[0] == "clear":
            st.clear_node(op[1])
        else:
            assert op[0] == "flush"
    return st


def run_ledger(ops, addresses, one_beat_a_batch=False):
    """the same calls through Host (interner, queue) into a Ledger; a batch per ("flush",) and one at the end"""
    host, led = M.Host(addresses), M.Ledger()
    for op in ops:
        if op[0] == "beat":
            host.heartbeat(op[1], op[2])
        elif op[0] == "store":
            host.store_metrics(op[2], op[1])
        elif op[0] == "manual":
            host.store_manual_metrics(op[1], op[2])
        elif op[0] == "delete":
            host.delete_metric(op[1], op[2], op[3])
        elif op[0] == "clear":
            host.clear_node(op[1])
        if op[0] == "flush" or one_beat_a_batch:
            led.ingest(*host.take())
    led.ingest(*host.take())
    return host, led


@pytest.mark.parametrize("c", MC.CASES, ids=[c["name"] for c in MC.CASES])
def test_named_case(c):
    assert M.same_fields(run_store(c["ops"]).fields(), c["want"])
    for split in (False, True):
        host, led = run_ledger(c["ops"], MC.ADDRESSES, one_beat_a_batch=split)
        assert M.same_fields(host.fields(led.listing()), c["want"]), split


def test_case_names_are_distinct_and_cover_the_issues_list():
    names = [c["name"] for c in MC.CASES]
    assert len(set(names)) == len(names)
    for word in ("max lower", "max equal", "max higher", "stored NaN", "with a NaN", "-0.0", "max set max", "re-added lower",
                 "middle one lacks", "merge onto a replace", "delete of an absent", "empty replace", "manual entries",
                 "dashboard:-progress"):
        assert any(word in n for n in names), word


def _random_ops(rng, addresses, n_ops):
    tasks, labels = ["", "t1", "t2"], ["loss", "lr", "dashboard-progress", "dashboard:-progress", "a:b", "ab", "x/y"]
    values = [0.0, -0.0, 1.0, -1.0, 2.5, 1e300, -1e300, float("inf"), float("nan"), 3.0]
    ops = []
    for _ in range(n_ops):
        k = rng.random()
        mets = [(rng.choice(tasks), rng.choice(labels), rng.choice(values)) for _ in range(rng.randrange(0, 5))]
        a = rng.choice(addresses + [M.ZERO])
        if k < 0.45:
            ops.append(("beat", a, mets if rng.random() < 0.9 else None))
        elif k < 0.65:
            ops.append(("store", a, mets))
        elif k < 0.75:
            ops.append(("manual", rng.choice(labels), rng.choice(values)))
        elif k < 0.9:
            ops.append(("delete", rng.choice(["manual", "t1", "t2"]), rng.choice(labels), a))
        elif k < 0.95:
            ops.append(("clear", a))
        else:
            ops.append(("flush",))
    return ops


@pytest.mark.parametrize("seed", range(40))
def test_ledger_model_is_the_store_on_seeded_sequences(seed):
    rng = random.Random(seed)
    addresses = [f"0x{w:040x}" for w in range(1, 6)]
    ops = _random_ops(rng, addresses, 60)
    st = run_store(ops)
    host, led = run_ledger(ops, addresses)
    assert M.same_fields(host.fields(led.listing()), st.fields())
    # the totals are the store's hashes added up field by field in the ledger's order, bit for bit
    order = [M.ZERO] + addresses
    sums, counts = led.totals()
    for s in range(led.n_series):
        held = [st.nodes[a][host.intern.field(s)] for a in order if host.intern.field(s) in st.nodes.get(a, {})]
        ref = 0.0
        for v in held:
            ref += v
        assert (M.bits(sums[s]), counts[s]) == (M.bits(ref), len(held)) or (math.isnan(ref) and math.isnan(sums[s]))
    # ... and the label names that have a total are the reference's aggregate's keys
    assert {host.intern.keys[s][1] for s in range(led.n_series) if counts[s]} == set(st.get_aggregate_metrics_for_all_tasks())


def test_row_bound_refuses_the_whole_batch():
    led = M.Ledger()
    full = [(s, 0, float(s)) for s in range(M.ROW_MAX)]
    led.ingest([(3, M.MERGE, 0, len(full))], full, M.ROW_MAX + 1)
    before = led.listing()
    with pytest.raises(M.Refused):
        led.ingest([(4, M.MERGE, 0, 1), (3, M.MERGE, 1, 1)], [(0, 0, 1.0), (M.ROW_MAX, 0, 2.0)], M.ROW_MAX + 1)
    assert led.listing() == before
    # a REPLACE that drops first has room
    led.ingest([(3, M.REPLACE, 0, 1)], [(M.ROW_MAX, 0, 2.0)], M.ROW_MAX + 1)
    assert led.listing() == [(3, M.ROW_MAX, 2.0)]


def test_totals_add_in_ascending_row_order_the_manual_row_first():
    led = M.Ledger()
    led.ingest([(7, M.MERGE, 0, 1), (M.MANUAL, M.MERGE, 1, 1), (2, M.MERGE, 2, 1)], [(0, 0, 1.0), (0, 0, 1e100), (0, 0, -1e100)], 1)
    assert led.order() == [M.MANUAL, 2, 7]
    assert led.totals() == ([((0.0 + 1e100) + -1e100) + 1.0], [3])
