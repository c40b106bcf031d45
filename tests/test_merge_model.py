"""The solo-group merge: a plain model written from the reference's Rust (tests/merge_model.py) against the CPU oracle on
every case of tests/merge_cases.py — a second, independent reading of mod.rs:631-873 beside oracle/pm_oracle.c — and the
coverage conditions that keep tests/test_gpu_merge_rules.py honest: conditions on the INPUTS, computed from the model
alone, that say which branches of the merge the cases reach.  No GPU."""
import numpy as np
import pytest

from oracle import oracle_ffi as orc
from helpers import oracle_groups
import merge_cases as MC
import merge_model

CREATED, DESTROYED = 1, 2

_results = {}


def _run(name):
    """(model result, oracle's n_merged, oracle's merge feed, ids of the solo groups before the merge)"""
    if name not in _results:
        sw, first, policy, x = MC.make_case(name)
        st, _held = MC.oracle_solo_pass(sw, first, policy, x)
        solo_ids = [g[0] for g in oracle_groups(st) if len(g[2]) == 1]
        model = MC.run_model(sw, st, policy, x)
        st.set_enabled(x["enabled_merge"])
        st.drain_events()
        n = st.try_merge_solo_groups()
        _results[name] = (model, n, st.drain_events(), solo_ids, x)
    return _results[name]


@pytest.mark.parametrize("name", list(MC.CASES))
def test_model_equals_oracle(name):
    """the merged groups — configuration and members — in creation order, the solo groups of every batch in batch
    order (the feed names them so: per merge, destroyed for every group of the batch, then created), the number returned"""
    model, n, events, _ids, _x = _run(name)
    assert n == len(model.merged)
    got, batch = [], []
    for kind, _gid, cfg, members in events:
        if kind == DESTROYED:
            assert len(members) == 1
            batch.append(members[0])
        else:
            got.append((cfg, batch, sorted(members)))
            batch = []
    assert batch == []
    want = [(cfg, b, sorted(b)) for cfg, b in model.merged]
    # (BTreeSet order is address order, not index order: compare the member SETS, and the batch order through the feed)
    assert [(c, b, sorted(m)) for c, b, m in got] == want


@pytest.mark.parametrize("name", [n for n in MC.CASES if MC.CASES[n].get("expect")])
def test_case_reaches_what_it_is_named_for(name):
    model, n, _events, _ids, x = _run(name)
    e = x["expect"]
    if e.get("zero_merges"):
        assert n == 0 and len(model.attempts) >= 1 and model.attempts[-1].label == "refused"
    if "cleared2" in e:
        assert sum(a.label == "cleared" and a.partial >= 2 for a in model.attempts) >= e["cleared2"]
    if "group_over" in e:
        assert max(len(b) for _c, b in model.merged) > e["group_over"]
    if "list_over" in e:
        assert max(n_list for _c, n_list in model.lists) > e["list_over"]
    if e.get("shrinks"):
        assert _shrinks(name)
    if e.get("blocked") or e.get("blocked_later"):
        assert model.count("blocked") >= 1
    if e.get("blocked_later"):
        assert _blocked_later(model)


def _shrinks(name):
    """a configuration's list is shorter than its compatible solos were before the pass: an earlier one took some"""
    model, _n, _events, _ids, x = _run(name)
    sw, first, policy, x = MC.make_case(name)
    st, _ = MC.oracle_solo_pass(sw, first, policy, x)
    masks = orc.compat_masks(st.nodes, st.cfgs)
    solos = [g[2][0] for g in oracle_groups(st) if len(g[2]) == 1]
    for cfg, n_list in model.lists:
        before = sum((int(masks[w]) >> cfg) & 1 for w in solos)
        if 0 < n_list < before and any(a.cfg == cfg and a.label not in ("refused", "blocked") for a in model.attempts):
            return True
    return False


def _blocked_later(model):
    """the blocked batch is not its configuration's first: batches applied before it, and a later configuration merged"""
    k = next(i for i, a in enumerate(model.attempts) if a.label == "blocked")
    cfg = model.attempts[k].cfg
    before = sum(a.cfg == cfg for a in model.attempts[:k])
    after = sum(a.cfg != cfg and a.label not in ("refused", "blocked") for a in model.attempts[k + 1:])
    return before >= 1 and after >= 1 and model.attempts[k].n_rem > 2 * len(model.attempts[k].batch)


def test_coverage_conditions():
    """What the GPU suite's cases reach, from the model alone."""
    reached = {label: [] for label in merge_model.LABELS}
    cleared2 = {}
    lone_seed, over65, over257, shrinking, later, short_ids = [], [], [], [], [], []
    for name in MC.CASES:
        model, n, _events, solo_ids, x = _run(name)
        for label in merge_model.LABELS:
            if model.count(label):
                reached[label].append(name)
        c2 = sum(a.label == "cleared" and a.partial >= 2 for a in model.attempts)
        if c2:
            cleared2[name] = c2
        sw = MC.make_case(name)[0]
        mins = {i: c[1] for i, c in enumerate(sw.configs)}
        # (the located seed alone is a valid batch of one where min = 1: kept, not refilled, refused)
        if n == 0 and model.attempts and all(a.label == "refused" and a.select in ("prox_full", "prox_short") and len(a.batch) == 1
                                             and mins[a.cfg] == 1 for a in model.attempts) \
                and any(sw.configs[a.cfg][2] > 1 and a.select == "prox_short" and a.n_rem > 100 for a in model.attempts):
            lone_seed.append(name)
        sizes = [len(b) for _c, b in model.merged]
        if sizes and max(sizes) > 65:
            over65.append(name)
        if sizes and max(sizes) > 257:
            over257.append(name)
        if x["expect"].get("shrinks") and _shrinks(name):
            shrinking.append(name)
        if model.count("blocked") and _blocked_later(model):
            later.append(name)
        # ids of fewer than 16 hex digits (format!("{:x}"): no padding) that change the list's order: the string order
        # of the solos' ids differs from the order of their values
        if any(i < (1 << 60) for i in solo_ids) and sorted(solo_ids, key=lambda i: "%x" % i) != sorted(solo_ids) \
                and len(model.merged) > 0:
            short_ids.append(name)
    print({k: len(v) for k, v in reached.items()}, "cleared2:", cleared2)
    for label in merge_model.LABELS:
        assert len(reached[label]) >= (1 if label == "blocked" else 5), (label, reached[label])
    assert sum(v >= 20 for v in cleared2.values()) >= 3, cleared2      # 20 times or more in at least 3 cases
    assert lone_seed, "no case with zero merges because of the lone located seed at min = 1"
    assert over65 and over257
    assert shrinking, "no configuration whose list shrinks because an earlier one took its solos"
    assert later, "no case where a later batch of a configuration is the blocked one"
    assert short_ids, "no case where short group ids change the order of the list"


def test_available_order_is_the_oracles():
    """min_group_size descending; equal min: with requirements first; otherwise as given (both sorts stable)"""
    configs = [("a", 2, 3, None), ("b", 4, 4, None), ("c", 2, 9, "gpu:count=1"), ("d", 4, 8, "gpu:count=2"), ("e", 1, 1, None),
               ("f", 2, 2, None), ("g", 4, 5, None)]
    cfgs = np.concatenate([orc.make_config(*c) for c in configs])
    code, order = orc.sort_configs(cfgs)
    assert code == 0
    for enabled in ([1] * 7, [1, 0, 1, 1, 0, 1, 1], [0, 1, 0, 0, 1, 0, 0]):
        want = [int(i) for i in order if enabled[int(i)]]
        assert merge_model.available_order(configs, enabled) == want
