"""A neighbour row lists no located candidate in front of its seed (FORM mode; protocol_amd/csrc: stream_bitmap_sweep's
mask, stream_drain, tile_keys, list_sweep_solo — the index walk leaves out the ones at the seed's own site only): such
a candidate is in a group by the seed's turn (mod.rs:526-530, the seed is the FIRST located compatible node), so
leaving it out changes no group — it spares its key and keeps late seeds' rows from running out.  The argument itself:
tests/test_row_front_model.py.

Every case forms its groups on the streaming carve, on the batch pipeline (carve_variant 3) and on a streaming launch
that gives up a third of the way in and continues on the batch pipeline; ids, configurations, members and order must
be oracle_ffi.State's with the same group_id_seed.
"""
import os
import re

import numpy as np
import pytest

from oracle import oracle_ffi as orc
from protocol_amd import engine as E
from protocol_amd import host
from helpers import engine_groups, oracle_groups
import row_front_cases as cases

pytestmark = pytest.mark.gpu

SEED = 7
# the parent commit's counters on the swarms of (a) and (b), measured on an MI355X (see the tests' docstrings)
PARENT_A_REFRESHES, PARENT_A_SLOW = 3, 0
PARENT_B_REFRESHES, PARENT_B_SLOW = 2, 0
PATHS = ["stream", "batch", "abort"]
_oracle = {}


def _want(name, sw):
    """the oracle's groups of a case, formed once and shared by the paths"""
    if name not in _oracle:
        nodes, cfgs, tasks, _enabled = orc.from_swarm(sw)  # (no tasks: every configuration enabled, as on the engine)
        st = orc.State(nodes, cfgs, tasks=tasks, reference_shaped=False, group_id_seed=SEED)
        n = st.try_form_new_groups()
        _oracle[name] = (n, oracle_groups(st))
    return _oracle[name]


def _form(name, sw, path, prune_mode=None):
    n_want, want = _want(name, sw)
    eng = E.Engine(group_id_seed=SEED, carve_variant=3 if path == "batch" else 0)
    host.load_swarm(eng, sw, enabled=cases.enabled_all(sw))
    if prune_mode is not None:
        eng.debug_prune_mode(prune_mode)
    if path == "abort":
        eng.debug_stream_abort_after(max(n_want // 3, 1))
    n_got = eng.form_groups()
    got = engine_groups(eng)
    c = eng.debug_carve_counters()
    stats = eng.last_stats()
    eng.close()
    assert n_got == n_want and got == want, (name, path)
    assert stats["host_resolved_steps"] == 0
    if path == "stream":
        assert c["stream"] == 1 and c["stream_aborts"] == 0, c
    elif path == "abort":
        assert c["stream_aborts"] == 1 and c["stream"] == 0 and c["batches"] >= 1, c
    return c, want


@pytest.mark.parametrize("path", PATHS)
def test_all_at_once_window(path):
    """(a) 1,500 located workers, one configuration (2, 8): all tickets at once, so a late seed's row — made while
    nearly every candidate in front of it was still free — used to be nearly all past by its turn.

    The streaming carve may not refresh or take exact steps more often than the parent commit does on this swarm.
    Measured on an MI355X, thirteen carves each (profiles/r11_row_front_bench.txt): the parent commit refreshes 3 times
    and takes 0 exact steps, every time (1,864 - 1,880 tickets); this commit 2 and 0 (1,452 - 1,468 tickets)."""
    c, _ = _form("a", cases.all_at_once(), path)
    if path == "stream":
        print("all_at_once counters:", c)
        assert c["stream_tickets"] > 0
        assert c["stream_refreshes"] <= PARENT_A_REFRESHES and c["slow_steps"] <= PARENT_A_SLOW, c


@pytest.mark.parametrize("path", PATHS)
def test_windowed(path):
    """(b) 2,400 located workers, the same configuration: more candidates than get their tickets at once — two
    look-ahead windows.

    The bound as in (a).  Measured on an MI355X, thirteen carves each: the parent commit refreshes 2 times and takes 0
    exact steps, every time; this commit the same — a window of a quarter of the candidates holds little of the past,
    so there was nothing to gain here, and nothing may be lost."""
    c, _ = _form("b", cases.windowed(), path)
    if path == "stream":
        print("windowed counters:", c)
        assert c["stream_tickets"] > 0
        assert c["stream_refreshes"] <= PARENT_B_REFRESHES and c["slow_steps"] <= PARENT_B_SLOW, c


@pytest.mark.parametrize("path", PATHS)
def test_location_less_candidates_in_front_of_the_seed_stay_in(path):
    """(c) every second worker without a location; the first configuration's located count is no multiple of 8, so its
    last located group is filled with location-less workers from positions IN FRONT of its seed: the rule must leave
    those in the row.  A second configuration takes what is left."""
    sw = cases.unlocated_in_front()
    _, want = _form("c", sw, path)
    # (checked on the oracle's groups: the case is what it is meant to be)
    loc = sw.has_loc.astype(bool)
    n_loc0 = sum(int(loc[m].sum()) for _id, cfg, m, _t in want if cfg == want[0][1])
    assert n_loc0 % 8 != 0
    mixed = [np.asarray(m) for _id, cfg, m, _t in want if cfg == want[0][1] and loc[m].any() and not loc[m].all()]
    assert len(mixed) == 1
    m = mixed[0]
    assert m[~loc[m]].min() < m[loc[m]].min()  # (the seed is the group's first located member in input order)
    assert len({cfg for _id, cfg, _m, _t in want}) == 2


@pytest.mark.parametrize("path", PATHS)
def test_cities(path):
    """(d) 5 shared sites of 60 workers among 900 scattered ones, groups of up to 9: candidates at the seed's own site in
    front of it — the rule's old special case — are left out as part of the general one, the ones behind the seed head
    its row in input order."""
    sw = cases.cities()
    _, want = _form("d", sw, path)
    site = {}
    for w in range(sw.W):
        site.setdefault((sw.lat[w], sw.lon[w]), []).append(w)
    assert sorted(len(v) for v in site.values() if len(v) > 1) == [60] * 5
    # (a city's seed takes its eight nearest from its own site, at distance 0: groups of one site exist)
    assert any(len({(sw.lat[w], sw.lon[w]) for w in m}) == 1 and len(m) == 9 for _id, _c, m, _t in want)


def _cell_min_n():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "protocol_amd", "csrc", "pm_device.h")).read()
    return int(re.search(r"PM_CELL_MIN_N\s*=\s*(\d+)", src).group(1))


@pytest.mark.parametrize("prune_mode", [2, 3])
@pytest.mark.parametrize("path", PATHS)
def test_the_walk(path, prune_mode):
    """(e) the smallest eligible count at which the engine builds a spatial index, every row from the index walk
    (prune mode 2: rows that still list candidates in front of their seed, beside swept rows that do not) and every
    row through the walk's whole-list fallback (3)."""
    n = _cell_min_n()
    c, _ = _form("e", cases.walk(n), path, prune_mode=prune_mode)
    if path == "stream":
        assert c["cell_g"] > 0 and c["n_indexed"] == n, c
        if prune_mode == 3:
            assert c["prune_fallbacks"] > 0, c
