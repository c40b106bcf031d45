"""The rollout ledger's model (tests/rollout_model.py) on the named cases (tests/rollout_cases.py) and against the reference: the
expectations of heartbeat.rs' own tests about the stored task fields (tests/golden/heartbeat_with_task.json), update_node_task's
match, TaskState::from — in the model and in pm_host_task_state — and nodes_per_task as the sync service counts it."""
import json
import os

import pytest

import rollout_cases as RC
import rollout_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "heartbeat_with_task.json")
NEAR_MISSES = ["", "running", "Running", "RUNNING ", " RUNNING", "RUNNING\n", "RUNNIN", "RUNNINGG", "PENDING,", "unknown", "NONE",
               "2", "\"RUNNING\"", "RÜNNING", "COMPLETE", "FAIL", "PAUSE", "RESTART", "PULL"]


def run_case(case):
    run = RC.Run(case)
    for step in case["steps"]:
        run.apply(step)
    return run


@pytest.mark.parametrize("case", RC.CASES, ids=[c["name"] for c in RC.CASES])
def test_the_model_on_the_named_cases(case):
    run = run_case(case)
    got = run.read()
    assert [w[3] for w in got["workers"]] == case["classes"]
    assert {row[0]: sum(row[6]) for row in got["tasks"] if sum(row[6])} == case["per_task"]
    by_class, by_state, with_task, converged, distinct = got["summary"]
    assert converged == case["converged"] == sum(r[5][M.RUNNING] == r[4] for r in got["groups"])
    assert by_class == tuple(case["classes"].count(c) for c in range(M.RO_N)) and sum(by_state) == case["W"]
    assert with_task == len(got["groups"]) and distinct == len(got["tasks"])
    assert [r[0] for r in got["tasks"]] == sorted({r[0] for r in got["tasks"]})          # ascending, every id once
    for gid, slot, cfg, task, size, same, other, silent in got["groups"]:
        assert sum(same) + other + silent == size
    for uid, task, groups, groups_conv, assigned, conv, reporters in got["tasks"]:
        held = [r for r in got["groups"] if run.task_uids()[r[3]] == uid]
        assert groups == len(held) and assigned == sum(r[4] for r in held) and conv == sum(r[5][M.RUNNING] for r in held)
        assert groups_conv == sum(r[5][M.RUNNING] == r[4] for r in held)
        if uid == M.ALL_ONES or uid not in run.task_uids():
            assert task == M.NONE
        else:
            assert task == run.task_uids().index(uid)


def test_every_class_occurs_in_the_cases():
    seen = set()
    for case in RC.CASES:
        seen |= set(case["classes"])
    assert seen == set(range(M.RO_N))


def test_the_store_against_the_reference_tests():
    """what heartbeat.rs' tests assert about the stored record: a heartbeat without task fields leaves none"""
    for g in json.load(open(GOLDEN))["cases"]:
        store = M.Store()
        addr = g["request"]["address"]
        store.add_node(addr)
        store.update_node_task(addr, "stale-task", "RUNNING", {"old": 1})      # whatever stood there before
        store.update_node_task(addr, g["request"].get("task_id"), g["request"].get("task_state"), g["request"].get("task_details"))
        want = g["stored"]
        assert store.record(addr) == (want["task_id"], want["task_state"], want["task_details"]), g["name"]
        assert M.nodes_per_task(store, [("t", t["name"]) for t in g["tasks"]]) == []


def test_update_node_task_is_a_match_on_both_options():
    s = M.Store()
    s.update_node_task("a", "t1", "RUNNING", {"d": 1})
    assert s.record("a") == ("t1", "RUNNING", {"d": 1})
    s.update_node_task("a", "t1", "bogus")                                   # (Some, Some, None): details go, the state is UNKNOWN
    assert s.record("a") == ("t1", "UNKNOWN", None)
    for task, state in ((None, "RUNNING"), ("t1", None), (None, None)):
        s.update_node_task("a", "t1", "RUNNING")
        s.update_node_task("a", task, state, {"d": 2})
        assert s.record("a") == (None, None, None)


def test_nodes_per_task_counts_the_reported_id():
    s = M.Store()
    for a, t, st in (("a", "t1", "RUNNING"), ("b", "t1", "FAILED"), ("c", "gone", "RUNNING"), ("d", None, None)):
        s.add_node(a)
        s.update_node_task(a, t, st)
    assert M.nodes_per_task(s, [("t1", "first"), ("t2", "second")]) == [("gone", "unknown", 1), ("t1", "first", 2)]


def test_task_state_from_in_the_model():
    for k, name in enumerate(M.TS_NAMES):
        assert M.task_state_from(name) == k
    for s in NEAR_MISSES:
        assert M.task_state_from(s) == M.UNKNOWN


def test_pm_host_task_state_on_all_names_and_near_misses():
    from protocol_amd import engine as E
    from protocol_amd import host
    assert E.TS_NAMES == M.TS_NAMES and (E.TS_N, E.TS_NONE, E.TS_RUNNING, E.TS_UNKNOWN) == (M.TS_N, M.TS_NONE, M.RUNNING, M.UNKNOWN)
    assert (E.RO_IDLE, E.RO_STRAY, E.RO_SILENT, E.RO_OTHER, E.RO_BEHIND, E.RO_CONVERGED, E.RO_N) == \
           (M.IDLE, M.STRAY, M.SILENT, M.OTHER, M.BEHIND, M.CONVERGED, M.RO_N)
    for k, name in enumerate(M.TS_NAMES):
        assert host.task_state(name) == k
    for s in NEAR_MISSES:
        assert host.task_state(s) == M.UNKNOWN == M.task_state_from(s), repr(s)
    assert host.task_state(None) == M.UNKNOWN


def test_the_structs_agree_between_the_header_and_numpy():
    import re
    from protocol_amd import engine as E
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    plain = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "pm_engine.h")).read(), flags=re.S)
    size = {"uint8_t": 1, "uint16_t": 2, "uint32_t": 4, "uint64_t": 8}
    dim = {"PM_RO_N": 6, "PM_TS_N": 8, "PM_TS_N + 1": 9}
    for name, dt in (("pm_ro_report", E.ro_report_dt), ("pm_ro_summary", E.ro_summary_dt), ("pm_ro_task_row", E.ro_task_row_dt),
                     ("pm_ro_group_row", E.ro_group_row_dt), ("pm_ro_worker_row", E.ro_worker_row_dt)):
        body = plain[plain.index("typedef struct %s {" % name):plain.index("} %s;" % name)]
        fields, off = [], 0
        for t, decl in re.findall(r"(uint\d+_t) ([^;]+);", body):
            for f in decl.split(","):
                m = re.match(r"\s*(\w+)(?:\[([^\]]+)\])?\s*$", f)
                n = dim[m.group(2)] if m.group(2) else 1
                off = (off + size[t] - 1) // size[t] * size[t]
                fields.append((m.group(1), off, size[t] * n))
                off += size[t] * n
        assert [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names] == fields, name
        assert dt.itemsize == (off + 7) // 8 * 8, name
