"""Group formation (try_form_new_groups, mod.rs:478-628) on the engine against the oracle, over the cases of
tests/form_cases.py — located counts on every hand-over point of the streaming carve (stream_run_config: the chain, the
register paths stream_small_n / stream_small_rows, the first-come tail in one go and its serial form, exact steps over
compacted and over all positions), group sizes across the last one with a chain and across the staging area, the LDS and
the BIG instantiations, several configurations back to back, standing groups and ineligible workers between the
candidates, exact distance ties — and through every implementation of the selection: the engine as it ships, both other
carve variants, the host's own step in between (debug_uncertain_every), a streaming launch that gives up and continues
on the batch pipeline, candidate lists kept in HBM, and the streaming carve short of row makers.

Per case, all of it: the count form_groups() returns, the groups (ids, configurations, members, in creation order), the
life-cycle feed event by event, after one match every worker's task, and a second formation right behind the first.  It
is all integers: nothing is sampled, nothing tolerated.  tests/test_form_model.py (no GPU) holds the cases to the rules
and hand-over points they are named for.

The index walk (PM_CELL_MIN_N candidates and more, FAST_REPROPOSE) is tests/test_gpu_row_front.py::test_the_walk's."""
import pytest

from protocol_amd import engine as E
from protocol_amd import host
from helpers import engine_groups, oracle_groups
import form_cases as FC

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
TH = FC.THRESHOLDS
ALL = list(FC.CASES)
SMALL = [n for n in ALL if FC.n_workers(n) <= 2500]
LONG = [n for n in SMALL if FC.n_workers(n) > 150]
PRESSURE = ["large_to_tail", "loc%d_all" % (TH["STREAM_LA_ALL"] + 1), "multi_six_waves"]

_expected = {}


def _has_chain(cfg):
    _name, _mn, mx, _req = cfg
    return 1 < mx and mx - 1 < TH["PM_PROP_KMAX"]


def _oracle(name):
    """what the oracle says at every stage of the case, and the model's records (computed once per case: neither depends
    on the engine's path)"""
    if name in _expected:
        return _expected[name]
    sw, enabled, policy, x, model = FC.modelled(name)
    st = FC.oracle_state(sw, enabled, policy, x)
    o = dict(sw=sw, enabled=enabled, policy=policy, x=x, model=model)
    o["standing"] = oracle_groups(st)
    o["n"] = st.try_form_new_groups()
    o["groups"] = oracle_groups(st)
    o["events"] = st.drain_events()
    o["tasks"] = [st.get_task_for_node(w) for w in range(sw.W)]
    o["groups_matched"] = oracle_groups(st)
    o["n_again"] = st.try_form_new_groups()
    o["groups_again"] = oracle_groups(st)
    o["events_again"] = st.drain_events()
    # a member of every fifth group dies: the whole group dissolves (status_update_impl.rs:17-29), the survivors re-enter
    # between the standing groups at the next formation
    o["victims"] = [int(g[2][len(g[2]) // 2]) for g in o["groups_again"][::5]]
    for w in o["victims"]:
        st.set_node_status(w, 4)
    o["groups_dead"] = oracle_groups(st)
    o["n_reformed"] = st.try_form_new_groups()
    o["groups_reformed"] = oracle_groups(st)
    o["events_reformed"] = st.drain_events()
    o["tasks_reformed"] = [st.get_task_for_node(w) for w in range(sw.W)]
    assert o["n"] == len(model.groups)
    # ---- what the model says about the engine's path
    steps = [s for s in model.steps if s.group is not None]
    o["cross_ties"] = sum(s.tie == "cross" for s in steps)
    o["chain_steps"] = chain_steps(model, sw)
    run = longest = 0
    for s in steps:    # (a step is ordered by distance when its seed is located and it had somebody to choose from)
        run = run + 1 if s.label in ("prox_full", "prox_fill", "prox_short") else 0
        longest = max(longest, run)
    o["longest_run"] = longest
    _expected[name] = o
    return o


def chain_steps(model, sw):
    """steps the streaming carve's chain can commit: a full group of located candidates while more than STREAM_SMALL_START
    of them are left, in a configuration whose rows can list max - 1 neighbours"""
    return sum(s.label == "prox_full" and s.n_located > TH["STREAM_SMALL_START"] and _has_chain(sw.configs[s.cfg]) for s in model.steps)


def _may_chain(name):
    """(cheap, from the parameters alone: cases that cannot reach the chain are not modelled at collection)"""
    kw = FC.CASES[name]
    if not kw.get("policy", {}).get("proximity", True):
        return False
    if "n" not in kw:
        return True
    mm = kw.get("mm", (2, 8))
    return kw["n"] > TH["STREAM_SMALL_START"] and _has_chain(("", mm[0], mm[1], None))


def _abort_lists():
    at_1, at_third = [], []
    for name in ALL:
        if not _may_chain(name):
            continue
        sw, _enabled, _policy, _x, model = FC.modelled(name)
        k = chain_steps(model, sw)
        if k > 1:
            at_1.append(name)
        if k > max(len(model.groups) // 3, 1):
            at_third.append(name)
    return at_1, at_third


ABORT_AT_1, ABORT_AT_THIRD = _abort_lists()


def _tasks_of(eng):
    t, _count = eng.match()
    return [(-1 if v == NONE else int(v)) for v in t]


def _check(name, *, mem_above=0, abort_after=None, reform=False, **engine_kw):
    o = _oracle(name)
    sw, x = o["sw"], o["x"]
    eng = E.Engine(**o["policy"], **engine_kw)
    try:
        pre = x["pre_enabled"]
        host.load_swarm(eng, sw, enabled=FC.enabled_bits(o["enabled"] if pre is None else pre))
        if pre is not None:     # the standing groups, from a pass of their own
            eng.form_groups()
            eng.set_enabled_mask(FC.enabled_bits(o["enabled"]))
        assert engine_groups(eng) == o["standing"]
        eng.enable_group_events()
        if mem_above:
            eng.debug_mem_lists_above(mem_above)
        if abort_after is not None:
            eng.debug_stream_abort_after(max(o["n"] // 3, 1) if abort_after == "third" else abort_after)
        # ---- the formation
        n = eng.form_groups()
        stats, c = eng.last_stats(), eng.debug_carve_counters()
        print(f"{name}: formed {n} (oracle {o['n']}), host steps {stats['host_resolved_steps']}, launches {stats['carve_launches']}, "
              f"stream {c['stream']} tickets {c['stream_tickets']} timeouts {c['stream_timeouts']} listed {c['stream_listed']} walked {c['pruned_batches']} "
              f"aborts {c['stream_aborts']} slow {c['slow_steps']} refreshes {c['stream_refreshes']} batches {c['batches']}")
        assert n == o["n"]
        assert engine_groups(eng) == o["groups"]
        assert eng.drain_group_events() == o["events"]
        # ---- one match: every worker's task
        assert _tasks_of(eng) == o["tasks"]
        assert engine_groups(eng) == o["groups_matched"]
        # ---- a second formation right behind the first
        if abort_after is not None:
            eng.debug_stream_abort_after(0)
        assert eng.form_groups() == o["n_again"]
        assert engine_groups(eng) == o["groups_again"]
        assert eng.drain_group_events() == o["events_again"]
        if reform:
            flags = host.worker_flags(sw)
            for w in o["victims"]:
                eng.on_worker_status(w, int(flags[w]) & ~E.W_HEALTHY, True)
            assert sorted(engine_groups(eng)) == sorted(o["groups_dead"])
            assert eng.form_groups() == o["n_reformed"]
            assert sorted(engine_groups(eng)) == sorted(o["groups_reformed"])
            assert eng.drain_group_events() == o["events_reformed"]
            assert _tasks_of(eng) == o["tasks_reformed"]
        return o, stats, c
    finally:
        eng.close()


@pytest.mark.parametrize("name", ALL)
def test_form_rules_default_engine(name):
    """the engine as it ships: the streaming carve (with proximity off there are no rows to make: the proposal-free
    single launch, pm_engine_carve.inc `use_props`), nothing left to the host but a boundary in a tie between two sites;
    then deaths inside every fifth group and one more tick"""
    o, stats, c = _check(name, reform=True)
    model, sw = o["model"], o["sw"]
    assert c["stream"] == (1 if o["policy"].get("proximity", True) else 0) and c["stream_aborts"] == 0, c
    if not o["policy"].get("proximity", True):
        assert stats["carve_launches"] == 1 and c["batches"] == 0, (stats, c)
    if o["cross_ties"] == 0:
        assert stats["host_resolved_steps"] == 0
    else:
        assert stats["host_resolved_steps"] > 0
    if c["stream"] == 1 and stats["host_resolved_steps"] == 0:
        # configurations the launch enters (mod.rs:507, :517 at the entry): each is counted once, by how its rows are made
        entered = sum(total >= sw.configs[cfg][1] and n >= sw.configs[cfg][1] and n > 0 for cfg, total, n, _loc in model.entries)
        assert c["stream_listed"] + c["pruned_batches"] == entered, (c, model.entries)
    if len(model.entries) == 1 and o["policy"].get("proximity", True) and _has_chain(sw.configs[model.entries[0][0]]):
        # one configuration: carved in registers from the start (no seed is handed to a row maker) / the chain
        if model.entries[0][3] <= TH["STREAM_SMALL_START"]:
            assert c["stream_tickets"] == 0, c
        else:
            assert c["stream_tickets"] > 0, c
    if all(not _has_chain(sw.configs[en[0]]) and sw.configs[en[0]][2] > 1 for en in model.entries) and o["policy"].get("proximity", True):
        # no row lists PM_PROP_KMAX neighbours or more: every group with somebody to choose is an exact step's
        chosen = sum(s.group is not None and s.label.startswith("prox_") for s in model.steps)
        assert c["stream_tickets"] == 0 and c["slow_steps"] == chosen, c


@pytest.mark.parametrize("name,carve_variant", [(n, v) for v in (1, 3) for n in SMALL] + [("slots_p1", 1), ("tail%d" % (TH["STREAM_TAIL_MAX"] + 1), 3)])
def test_form_rules_carve_variants(name, carve_variant):
    """the single-workgroup kernel and the batch pipeline (one BIG case each: more eligible positions than the LDS form holds)"""
    _, _, c = _check(name, carve_variant=carve_variant)
    assert c["stream"] == 0, c


@pytest.mark.parametrize("every", [2, 3])
@pytest.mark.parametrize("name", SMALL)
def test_form_rules_host_steps_in_between(name, every):
    """debug_uncertain_every: every second / third distance-ordered step is the host's, the kernel continues behind it —
    more than `every` such steps in a row must reach it.  The hook switches the (1, 1) short-cut off: groups of one
    through the general path."""
    o, stats, _ = _check(name, debug_uncertain_every=every)
    if o["longest_run"] > every:
        assert stats["host_resolved_steps"] > 0


@pytest.mark.parametrize("name,after", [(n, 1) for n in ABORT_AT_1] + [(n, "third") for n in ABORT_AT_THIRD])
def test_form_rules_stream_abort(name, after):
    """the streaming launch gives up after 1 step / a third of the groups (what it committed stands) and the batch pipeline
    takes the rest; the hook switches the (1, 1) short-cut off too"""
    _, _, c = _check(name, abort_after=after)
    assert c["stream_aborts"] == 1 and c["batches"] >= 1, c


@pytest.mark.parametrize("name", LONG)
def test_form_rules_lists_kept_in_hbm(name):
    """debug_mem_lists_above(150) on the batch pipeline: carve_step_mem, the exact step with keys, bitmaps and selection in HBM"""
    _check(name, mem_above=150, carve_variant=3)


@pytest.mark.parametrize("env", [{"PM_STREAM_WGS": "1"}, {"PM_STREAM_ROW_SPINS": "1"}, {"PM_STREAM_LA": "24"}])
@pytest.mark.parametrize("name", PRESSURE)
def test_form_rules_streaming_carve_under_pressure(name, env, monkeypatch):
    """one row-making workgroup; a validator that gives a row up after one poll (such seeds become exact steps); a
    look-ahead of 24 tickets"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _, _, c = _check(name)
    assert c["stream"] == 1 and c["stream_aborts"] == 0, c
