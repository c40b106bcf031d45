"""The solo-group merge (try_merge_solo_groups, mod.rs:631-971) on the engine against the oracle, over the cases of
tests/merge_cases.py — min >= 3 (a partial proximity batch of 2..min-1 located groups is thrown away and the batch
refilled first-come), max up to 300 (the wide rounds of the exact step, members past the staging area), located shares
chosen to stress the rules, several merge configurations that consume each other's solos, a batch blocked in the middle
of a configuration — and through every implementation of the selection: the streaming carve's chain in merge mode, the
exact step in its LDS, BIG and all-in-HBM forms, both other carve variants, the host's own step in between
(debug_uncertain_every), the single-workgroup kernel after an abort of the streaming launch.

Per case, all of it: the groups after the solo pass, n_merged, the groups after the merge (ids, configurations, members,
tasks), the life-cycle feed event by event, after one more match every worker's task, and a second merge pass.  It is all
integers: nothing is sampled, nothing tolerated.  tests/test_merge_model.py (no GPU) holds the cases to the branches they
are named for."""
import pytest

from protocol_amd import engine as E
from protocol_amd import host
from helpers import engine_groups, oracle_groups
import merge_cases as MC

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
STREAM_MIN = 512          # PM_MERGE_STREAM_MIN's default
STREAM_KMAX = 63          # PM_PROP_KMAX: the streaming carve takes max_group_size - 1 < 63 neighbours from a row
STREAM_SMALL_START = 128  # located candidates up to which the chain leaves a merge list to exact steps
ALL = list(MC.CASES)
SMALL = [n for n in ALL if MC.CASES[n].get("n", 650) <= 2000]


def _streams_by_default(name):
    """cases whose merge configuration's list is long enough for the streaming merge as the engine ships"""
    c = MC.CASES[name]
    return ("mm" in c and c.get("n", 650) >= STREAM_MIN and 1 < c["mm"][1] <= STREAM_KMAX
            and c.get("policy", {}).get("proximity", True))


STREAMED = [n for n in ALL if _streams_by_default(n)]
LONG = [n for n in SMALL if MC.CASES[n].get("n", 650) > 150]

_expected = {}


def _oracle(name, keep_state=False):
    """what the oracle says at every stage of the case (computed once per case: it does not depend on the engine's path)"""
    if name in _expected and not keep_state:
        return _expected[name]
    sw, first, policy, x = MC.make_case(name)
    st, held = MC.oracle_solo_pass(sw, first, policy, x)
    o = dict(sw=sw, first=first, policy=policy, x=x, held=held)
    o["solo_groups"] = oracle_groups(st)
    o["solo_events"] = st.drain_events()
    o["model"] = MC.run_model(sw, st, policy, x)
    st.set_enabled(x["enabled_merge"])
    o["n_merged"] = st.try_merge_solo_groups()
    o["groups"] = oracle_groups(st)
    o["events"] = st.drain_events()
    o["tasks"] = [st.get_task_for_node(w) for w in range(sw.W)]
    o["groups_matched"] = oracle_groups(st)
    o["n_merged_again"] = st.try_merge_solo_groups()
    o["groups_again"] = oracle_groups(st)
    o["events_again"] = st.drain_events()
    assert o["n_merged"] == len(o["model"].merged)
    if keep_state:
        o = dict(o, st=st)
    else:
        _expected[name] = o
    return o


def _expected_streamed(o, stream_min, engine_kw, mem_above=0):
    """merge configurations whose selections go through the streaming carve (pm_engine_merge.inc run_merge), from the
    model's list lengths"""
    if engine_kw.get("carve_variant", 0) != 0 or not o["policy"].get("proximity", True) or mem_above:
        return 0
    n = 0
    for cfg, n_list in o["model"].lists:
        _name, mn, mx, _req = o["sw"].configs[cfg]
        if n_list >= max(mn, stream_min) and 1 < mx and mx - 1 < STREAM_KMAX:
            n += 1
    return n


def _tasks_of(eng):
    t, _count = eng.match()
    return [(-1 if v == NONE else int(v)) for v in t]


def _check(name, *, stream_min=STREAM_MIN, mem_above=0, abort_after=0, full=False, **engine_kw):
    o = _oracle(name, keep_state=full)
    sw, x = o["sw"], o["x"]
    eng = E.Engine(**o["policy"], **engine_kw)
    try:
        host.load_swarm(eng, sw, enabled=MC.enabled_bits(o["first"]))
        eng.enable_group_events()
        # ---- the solo pass
        eng.form_groups()
        if o["held"] is not None:
            assert _tasks_of(eng) == o["held"]
        assert engine_groups(eng) == o["solo_groups"]
        assert eng.drain_group_events() == o["solo_events"]
        # ---- the merge
        eng.set_enabled_mask(MC.enabled_bits(x["enabled_merge"]))
        if mem_above:
            eng.debug_mem_lists_above(mem_above)
        if abort_after:
            eng.debug_stream_abort_after(abort_after)
        n_merged = eng.merge_solo_groups()
        stats = eng.last_stats()
        print(f"{name}: merged {n_merged} (oracle {o['n_merged']}), lists {o['model'].lists}, streamed {eng.debug_merge_streamed()}, "
              f"launches {stats['carve_launches']}, host steps {stats['host_resolved_steps']}")
        assert n_merged == o["n_merged"]
        assert sorted(engine_groups(eng)) == sorted(o["groups"])
        assert eng.drain_group_events() == o["events"]
        n_streamed = _expected_streamed(o, stream_min, engine_kw, mem_above)
        assert eng.debug_merge_streamed() == n_streamed
        # ---- one more match: a dissolved solo's task is free again, a merged group holds what find_best_task_for_group picked
        assert _tasks_of(eng) == o["tasks"]
        assert sorted(engine_groups(eng)) == sorted(o["groups_matched"])
        # ---- a second merge pass right behind the first: the leftover solos
        if abort_after:
            eng.debug_stream_abort_after(0)
        assert eng.merge_solo_groups() == o["n_merged_again"]
        assert sorted(engine_groups(eng)) == sorted(o["groups_again"])
        assert eng.drain_group_events() == o["events_again"]
        if full:
            _deaths_and_a_tick(o, eng)
        return o, stats, n_streamed
    finally:
        eng.close()


def _deaths_and_a_tick(o, eng):
    """a member of every fifth merged group dies (the whole group dissolves, status_update_impl.rs:17-29); the next form +
    merge re-forms the survivors as the oracle does"""
    sw, st = o["sw"], o["st"]
    flags = host.worker_flags(sw)
    victims = [int(g[2][len(g[2]) // 2]) for g in [g for g in engine_groups(eng) if len(g[2]) >= 2][::5]]
    for w in victims:
        st.set_node_status(w, 4)
        eng.on_worker_status(w, int(flags[w]) & ~E.W_HEALTHY, True)
    assert sorted(engine_groups(eng)) == sorted(oracle_groups(st))
    assert eng.form_groups() == st.try_form_new_groups()
    assert eng.merge_solo_groups() == st.try_merge_solo_groups()
    assert sorted(engine_groups(eng)) == sorted(oracle_groups(st))
    assert eng.drain_group_events() == st.drain_events()
    assert _tasks_of(eng) == [st.get_task_for_node(w) for w in range(sw.W)]


@pytest.mark.parametrize("name", ALL)
def test_merge_rules_default_engine(name):
    """the engine as it ships: the streaming merge for lists of 512 and more with max <= 63, the exact step otherwise
    (LDS; BIG above 8,192 candidates); then deaths inside merged groups and one more tick"""
    _, _, n_streamed = _check(name, full=True)
    if "mm" in MC.CASES[name]:
        assert n_streamed == (1 if name in STREAMED else 0)


@pytest.mark.parametrize("name", SMALL)
def test_merge_rules_small_lists_down_the_streaming_merge(name, monkeypatch):
    monkeypatch.setenv("PM_MERGE_STREAM_MIN", "8")
    _check(name, stream_min=8)


# (the 12,500-solo list once: the two variants share the exact step)
@pytest.mark.parametrize("name,carve_variant", [(n, v) for v in (1, 3) for n in SMALL] + [("big_5_16_30", 1)])
def test_merge_rules_carve_variants(name, carve_variant):
    """no streaming merge: every selection is carve_exact_step's (the big case: its BIG form, more candidates than the
    LDS form's 8,192 slots)"""
    _check(name, carve_variant=carve_variant)


@pytest.mark.parametrize("every", [2, 3])
@pytest.mark.parametrize("name", SMALL)
def test_merge_rules_host_steps_in_between(name, every):
    """debug_uncertain_every: every second / third distance-ordered selection is host_merge_select's, the kernel continues
    behind it.  (The hook counts all steps and sends a step to the host when its number divides and the kept batch was
    ordered by distance — not the first-come ones: more than `every` such steps in a row must reach it.)"""
    o, stats, _ = _check(name, debug_uncertain_every=every)
    run = longest = 0
    for a in o["model"].attempts:
        run = run + 1 if a.label in ("prox_full", "prox_short") else 0
        longest = max(longest, run)
    if longest > every:
        assert stats["host_resolved_steps"] > 0


@pytest.mark.parametrize("name", LONG)
def test_merge_rules_lists_kept_in_hbm(name):
    """debug_mem_lists_above(150): carve_step_mem, the exact step with keys, bitmaps and selection in HBM"""
    _check(name, mem_above=150)


@pytest.mark.parametrize("after", [1, 40])
@pytest.mark.parametrize("name", STREAMED)
def test_merge_rules_stream_abort(name, after):
    """the streaming launch gives up after 1 / 40 committed steps (what it committed stands) and the single-workgroup
    kernel takes the rest of the list: one launch more than without the abort wherever the chain gets that far"""
    o, stats, n_streamed = _check(name, abort_after=after)
    assert n_streamed == 1
    cfg = 1
    chain_steps = sum(a.cfg == cfg and a.select == "prox_full" and a.n_loc > STREAM_SMALL_START for a in o["model"].attempts)
    others = sum(1 for c, n_list in o["model"].lists if c != cfg and n_list >= o["sw"].configs[c][1])
    if chain_steps > after + 8 and stats["host_resolved_steps"] == 0:
        assert stats["carve_launches"] == 3 + 1 + others       # (place + stream + wait) + the kernel that takes the rest
    elif chain_steps == 0 and stats["host_resolved_steps"] == 0:
        assert stats["carve_launches"] == 3 + others


@pytest.mark.parametrize("env", [{"PM_STREAM_WGS": "1"}, {"PM_STREAM_ROW_SPINS": "1"}])
def test_merge_rules_streaming_merge_under_pressure(env, monkeypatch):
    """one row-making workgroup; a validator that gives a row up after one poll (such seeds become exact steps)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _, _, n_streamed = _check("m3_8_30")
    assert n_streamed == 1
