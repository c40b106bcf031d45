"""Group formation: a plain model written from the reference's Rust (tests/form_model.py) against the CPU oracle on every
case of tests/form_cases.py — a second, independent reading of mod.rs:478-628 beside oracle/pm_oracle.c — and the
conditions that keep tests/test_gpu_form_rules.py honest: conditions on the INPUTS and on the model's records that say
which rule every group of a case comes from and which hand-over point of the streaming carve the case sits on.  No GPU."""
import numpy as np
import pytest

from helpers import oracle_groups
import form_cases as FC
import form_model

TH = FC.THRESHOLDS
_results = {}


def _run(name):
    """(swarm, model result, the oracle's count, the oracle's groups as (configuration, members), expectations)"""
    if name not in _results:
        sw, enabled, policy, x, model = FC.modelled(name)
        st = FC.oracle_state(sw, enabled, policy, x)
        standing = len(oracle_groups(st))
        n = st.try_form_new_groups()
        groups = [(cfg, mem) for _gid, cfg, mem, _task in oracle_groups(st)[standing:]]
        _results[name] = (sw, model, n, groups, x, standing)
    return _results[name]


@pytest.mark.parametrize("name", list(FC.CASES))
def test_model_equals_oracle(name):
    """the groups — configuration by configuration, member by member, in creation order — and the number returned"""
    _sw, model, n, groups, _x, _standing = _run(name)
    assert n == len(model.groups)
    assert groups == model.groups


def _tail_len(model, cfg=0):
    """compatible candidates left at the configuration's first iteration without a located one"""
    return next(s.n_compatible for s in model.steps if s.cfg == cfg and s.n_located == 0)


def _group_steps(model, cfg=None):
    return [s for s in model.steps if s.group is not None and (cfg is None or s.cfg == cfg)]


@pytest.mark.parametrize("name", list(FC.CASES))
def test_case_reaches_what_it_is_named_for(name):
    sw, model, _n, _groups, x, standing = _run(name)
    e = x["expect"]
    assert e, "a case says what it is named for"
    steps = _group_steps(model)
    for cfg, k in e.get("entry", {}).items():
        assert model.entry(cfg)[3] == k
    for cfg, k in e.get("entry_compatible", {}).items():
        assert model.entry(cfg)[2] == k
    for cfg, k in e.get("entry_total", {}).items():
        assert model.entry(cfg)[1] == k
    if "eligible" in e:
        assert model.entries[0][1] == e["eligible"]
    if e.get("tail"):      # a located phase, then a first-come tail; where the last located group is filled, from in front too
        located = [s for s in steps if s.cfg == 0 and s.label.startswith("prox_")]
        assert model.entry(0)[3] == 0 or located
        assert model.entry(0)[2] > model.entry(0)[3]
        if model.entry(0)[3] >= 64:
            assert _tail_len(model) >= 1
            assert model.count("seed_unlocated") >= 1
    if "tail_len" in e:
        assert _tail_len(model) == e["tail_len"]
        mn, mx = sw.configs[0][1:3]
        r = e["tail_len"]
        assert model.count("seed_unlocated") == (0 if r < mn else r // mx + (r % mx >= mn))
    if "last_located" in e:
        assert [s for s in steps if s.label.startswith("prox_")][-1].label == e["last_located"]
    if e.get("phases"):     # the chain's share, 65..STREAM_SMALL in registers, a wave's worth on rows, the last STREAM_SMALL_AT
        seen = [s.n_located for s in steps if s.cfg == 0]
        assert seen[0] > TH["STREAM_SPARSE_MAX"] > TH["STREAM_LA_ALL"]
        assert any(TH["STREAM_LA_ALL"] >= k > TH["STREAM_SMALL_START"] for k in seen)
        assert any(TH["STREAM_SMALL_START"] >= k > 64 for k in seen) and any(64 >= k > TH["STREAM_SMALL_AT"] for k in seen)
        assert any(TH["STREAM_SMALL_AT"] >= k > 0 for k in seen)
    if "group_max" in e:
        assert max(len(s.group) for s in steps) == e["group_max"]
    if "crosses" in e:      # the second step's candidates sit d off the threshold: steps on either side of it
        thr, d = e["crosses"]
        assert steps[0].n_compatible > TH[thr] and steps[1].n_compatible == TH[thr] + d
        assert all(s.label in ("prox_full", "prox_short") for s in steps)
    if "first_label" in e:
        assert model.steps[0].label == e["first_label"]
        assert model.steps[0].n_total >= 100 * max(model.steps[0].n_compatible, 1) or e.get("big_stops")
    if "order" in e:
        assert [en[0] for en in model.entries] == e["order"]
        assert all(any(s.cfg == c for s in steps) or e.get("first_label") for c in e["order"])
    if e.get("wave_each"):
        assert all(TH["STREAM_SMALL_AT"] < en[3] <= 64 and en[2] <= 64 for en in model.entries)
    if e.get("big_stops"):  # both stops with more than STREAM_SMALL_START located candidates in hand
        stops = [s for s in model.steps if s.group is None]
        assert [s.label for s in stops] == ["stop_compatible", "stop_total"]
        assert all(s.n_located > TH["STREAM_SMALL_START"] for s in stops)
    if e.get("positions_differ"):
        elig = [w for w in range(sw.W) if sw.status[w] == 2 and sw.has_p2p[w]]
        assert sum(p != w for p, w in enumerate(elig)) > len(elig) // 2
    if e.get("standing"):   # standing groups, and new groups whose members lie between members of standing ones
        assert standing >= 20
        st = FC.oracle_state(*FC.make_case(name))
        held = np.nonzero(st.node_to_group >= 0)[0]
        assert sum(np.searchsorted(held, max(g.group)) > np.searchsorted(held, min(g.group)) for g in steps) > len(steps) // 2
    if "tie" in e:
        assert any(s.tie == e["tie"] for s in steps)
    if "first_tie" in e:
        assert steps[0].tie == e["first_tie"] and steps[0].seed == 0
    if "only" in e:
        assert {s.label for s in steps} == {e["only"]}


def _reached_sizes(model):
    """label -> the located counts it was reached at"""
    out = {}
    for s in model.steps:
        out.setdefault(s.label, []).append(s.n_located)
    return out


def test_coverage_conditions():
    """What the GPU suite's cases reach, from the model alone: every label in three cases or more; every label with a
    wave's worth of located candidates or fewer and with more than STREAM_SMALL_START of them (seed_unlocated has none by
    definition); every hand-over point with a case on it, one below it and one above it."""
    reached = {label: set() for label in form_model.LABELS}
    small = {label: set() for label in form_model.LABELS}
    large = {label: set() for label in form_model.LABELS}
    entry_located, entry_eligible, group_sizes, maxes, tails, ones, sparse_second = set(), set(), set(), set(), set(), set(), set()
    fill_in_front, ties = [], {"site": [], "cross": []}
    for name in FC.CASES:
        sw, model, _n, _groups, x, _standing = _run(name)
        for label, ks in _reached_sizes(model).items():
            reached[label].add(name)
            if min(ks) <= 64:
                small[label].add(name)
            if max(ks) > TH["STREAM_SMALL_START"]:
                large[label].add(name)
        entry_located.update(en[3] for en in model.entries)
        entry_eligible.add(model.entries[0][1])
        steps = _group_steps(model)
        group_sizes.update(len(s.group) for s in steps)
        maxes.update(sw.configs[en[0]][2] for en in model.entries if any(s.cfg == en[0] for s in steps))
        tails.update(s.n_compatible for s in steps if s.label == "seed_unlocated")
        if "tail_len" in x["expect"]:
            tails.add(_tail_len(model))
        ones.update(en[2] for en in model.entries if sw.configs[en[0]][2] == 1)
        if "crosses" in x["expect"]:
            sparse_second.add(steps[1].n_compatible)
        if any(s.fill_in_front for s in model.steps):
            fill_in_front.append(name)
        for kind in ties:
            if any(s.tie == kind for s in model.steps):
                ties[kind].append(name)
    print({k: len(v) for k, v in reached.items()}, "fill in front:", len(fill_in_front), "ties:", {k: len(v) for k, v in ties.items()})
    for label in form_model.LABELS:
        assert len(reached[label]) >= 3, (label, reached[label])
        assert small[label], label
        if label != "seed_unlocated":
            assert large[label], label

    def around(values, thr, what):
        assert {thr - 1, thr, thr + 1} <= values, (what, thr, sorted(v for v in values if abs(v - thr) < 70))

    around(entry_located, TH["STREAM_SMALL_AT"], "located at entry")
    around(entry_located, TH["ROWS"], "located at entry")
    around(entry_located, TH["STREAM_SMALL"], "located at entry")
    around(entry_located, TH["STREAM_SMALL_START"], "located at entry")
    around(entry_located, TH["STREAM_LA_ALL"], "located at entry")
    around(sparse_second, TH["STREAM_SPARSE_MAX"], "candidates of an exact step")
    around(tails, TH["STREAM_TAIL_MAX"], "first-come tail")
    around(ones, TH["STREAM_TAIL_MAX"], "candidates of a (1, 1) configuration")
    around(entry_eligible, TH["PM_CARVE_SLOTS"], "eligible positions")
    around({m - 1 for m in maxes}, TH["PM_PROP_KMAX"], "neighbours a group takes")
    around(group_sizes, TH["PM_CARVE_SEL_CAP"], "members staged")
    assert {0, 1, 2, 7, 8, 9} <= entry_located           # min - 1 .. max + 1 of (2, 8)
    assert {0, 1, 2, 8, 9} <= tails                       # 0, 1 = min - 1, min, max, max + 1
    assert len(fill_in_front) >= 5, fill_in_front
    assert len(ties["site"]) >= 2 and len(ties["cross"]) >= 1, ties


def test_stream_abort_list_is_long_enough():
    """the cases tests/test_gpu_form_rules.py sends down an aborted streaming launch: at least ten, from the model"""
    import test_gpu_form_rules as G
    assert len(G.ABORT_AT_1) >= 10 and len(G.ABORT_AT_THIRD) >= 10, (G.ABORT_AT_1, G.ABORT_AT_THIRD)


def test_oracle_in_reference_shape_agrees():
    """orc.State(reference_shaped=True) — the oracle restating the reference's loops as they are — on the cases of up to 700
    workers"""
    n_cases = 0
    for name in FC.CASES:
        if FC.n_workers(name) > 700:
            continue
        sw, enabled, policy, x = FC.make_case(name)
        nodes, cfgs, tasks, _ = FC.orc.from_swarm(sw)
        pre = x["pre_enabled"]
        st = FC.orc.State(nodes, cfgs, enabled=enabled if pre is None else pre, tasks=tasks, reference_shaped=True, **policy)
        if pre is not None:
            st.try_form_new_groups()
            st.set_enabled(enabled)
        standing = len(oracle_groups(st))
        n = st.try_form_new_groups()
        _sw, model, _n, _groups, _x, _standing = _run(name)
        assert n == len(model.groups), name
        assert [(cfg, mem) for _gid, cfg, mem, _task in oracle_groups(st)[standing:]] == model.groups, name
        n_cases += 1
    assert n_cases >= 40
