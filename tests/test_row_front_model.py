"""The argument behind the row makers' rule, as a numpy model (no GPU): a neighbour row lists, of the located candidates,
only the ones BEHIND its seed.

A row is made early — against a superset of what is alive when its seed has its turn — and is used late: the
validator takes its first `want` entries that are still alive.  The rule drops every located candidate in front of
the seed from the row, wherever it sits: the seed of a step is the first located compatible node in input order
(node_groups/mod.rs:526-530), so by the time position s is a seed, a located candidate at a position below s is in a
group already (a live one would have been the seed instead).  Location-less candidates in front of the seed stay in:
they sort behind every located one and may well be alive at the seed's turn.

Checked here on random small swarms, against the reference rule restated in numpy (full filter + stable sort by the
oracle's own distance; the groups it forms are compared with oracle_ffi.State's):
  * whenever a row — made against a random earlier moment of the carve — still has `want` live entries at its seed's
    turn, its first `want` live entries are the reference's selection, in the reference's order;
  * a complete row (fewer candidates than it can list) lists every candidate that is alive at the seed's turn.
"""
import numpy as np
import pytest

from oracle import oracle_ffi as orc
from protocol_amd.swarm import make_swarm

ROW_K = 63  # neighbours a row can list (PM_PROP_KMAX)


def _swarm(seed, W, n_cfg, unlocated, n_sites, sizes):
    """W workers of make_swarm (specs, 3 % not healthy, 1 % without p2p id), locations redrawn: `unlocated` of them
    have none, n_sites shared sites hold a third of the located ones, the rest are scattered"""
    rng = np.random.default_rng(seed)
    sw = make_swarm(seed, 0, W)
    sw.has_loc[:] = rng.random(W) >= unlocated
    sw.lat[:] = np.round(rng.uniform(25.0, 60.0, W), 4)
    sw.lon[:] = np.round(rng.uniform(-125.0, 40.0, W), 4)
    if n_sites:
        s_lat, s_lon = np.round(rng.uniform(25.0, 60.0, n_sites), 4), np.round(rng.uniform(-125.0, 40.0, n_sites), 4)
        at = rng.random(W) < 1.0 / 3.0
        which = rng.integers(0, n_sites, W)
        sw.lat[:] = np.where(at, s_lat[which], sw.lat)
        sw.lon[:] = np.where(at, s_lon[which], sw.lon)
    reqs = ["gpu:count=8", None] if n_cfg == 2 else [None]
    sw.configs = [(f"c{k}", sizes[k][0], sizes[k][1], reqs[k]) for k in range(n_cfg)]
    return sw


def _reference_order(s, cand, loc, lat, lon):
    """mod.rs:538-542: the compatible nodes without the seed, stable-sorted by distance to the seed — nodes without a
    location behind every located one, ties in input order"""
    rest = cand[cand != s]
    d = orc.distance_column(float(lat[s]), float(lon[s]), lat[rest], lon[rest])
    d = np.where(loc[rest], d, np.inf)
    return rest[np.argsort(d, kind="stable")]


def _carve(sw, masks, cfg_order):
    """try_form_new_groups (mod.rs:478-628) with proximity on, restated: per step (configuration, seed, members in
    selection order, what was alive before the step)"""
    W = sw.W
    loc, lat, lon = sw.has_loc.astype(bool), sw.lat, sw.lon
    alive = (sw.status == 2) & sw.has_p2p.astype(bool)  # Healthy, p2p id known (mod.rs:492-497)
    steps = []
    for c in cfg_order:
        mn, mx = sw.configs[c][1], sw.configs[c][2]
        comp = ((masks >> np.uint64(c)) & np.uint64(1)) != 0
        while int(alive.sum()) >= mn:
            cand = np.nonzero(alive & comp)[0]
            if len(cand) < mn:
                break
            located = cand[loc[cand]]
            s = int(located[0]) if len(located) else int(cand[0])
            order = _reference_order(s, cand, loc, lat, lon) if loc[s] else cand[cand != s]
            members = [s] + order[:mx - 1].tolist()
            if len(members) < mn:
                break
            steps.append((c, s, members, alive.copy()))
            alive[members] = False
    return steps


def _row(s, superset, loc, lat, lon):
    """a row as a row maker builds it: the candidates of `superset` without the seed and without the located ones in
    front of it, the ROW_K nearest in (distance, position) order; complete = nothing was left out"""
    rest = superset[(superset != s) & ~(loc[superset] & (superset < s))]
    order = _reference_order(s, np.append(rest, s), loc, lat, lon)
    return order[:ROW_K], len(order) < ROW_K


CASES = [(W, n_cfg, unl, sites)
         for W, n_cfg in ((200, 1), (420, 2), (600, 1), (333, 2))
         for unl in (0.0, 0.3, 0.9)
         for sites in (0, 5)]


@pytest.mark.parametrize("W,n_cfg,unlocated,n_sites", CASES)
def test_rows_without_located_candidates_in_front_select_what_the_reference_selects(W, n_cfg, unlocated, n_sites):
    seed = W * 7 + n_cfg * 3 + int(unlocated * 10) + n_sites
    rng = np.random.default_rng(seed + 1000)
    lo = [int(rng.integers(2, 6)) for _ in range(n_cfg)]
    sizes = [(lo[k], int(rng.integers(lo[k], 10))) for k in range(n_cfg)]  # group sizes 2..9
    sw = _swarm(seed, W, n_cfg, unlocated, n_sites, sizes)
    nodes, cfgs, _tasks, _enabled = orc.from_swarm(sw)
    masks = orc.compat_masks(nodes, cfgs)
    st = orc.State(nodes, cfgs, reference_shaped=False)
    st.try_form_new_groups()
    want_groups = [(c, mem) for (_s, _id, c, mem, _t) in st.groups()]
    cfg_order = list(dict.fromkeys(c for c, _ in want_groups))
    cfg_order += [c for c in range(n_cfg) if c not in cfg_order]
    steps = _carve(sw, masks, cfg_order)
    rank = sw.addr_rank()
    got_groups = [(c, sorted(mem, key=lambda w: rank[w])) for c, _s, mem, _a in steps]
    assert got_groups == want_groups, "the numpy restatement of the reference rule forms other groups than the oracle"

    loc, lat, lon = sw.has_loc.astype(bool), sw.lat, sw.lon
    n_served = n_complete = n_dropped = 0
    for i, (c, s, members, alive_now) in enumerate(steps):
        if not loc[s]:
            continue  # (a seed without a location has no row: the first-come tail)
        comp = ((masks >> np.uint64(c)) & np.uint64(1)) != 0
        # the row is made at an earlier moment of the carve, drawn at random — this configuration's or an earlier one's
        # (tickets of the configuration expected next are issued ahead of its turn)
        j = int(rng.integers(0, i + 1))
        alive_then = steps[j][3]
        assert not (alive_now & ~alive_then).any()  # (a superset: candidates are only ever removed)
        superset = np.nonzero(alive_then & comp)[0]
        row, complete = _row(s, superset, loc, lat, lon)
        n_dropped += int((loc[superset] & (superset < s)).sum())
        # no located candidate in front of the seed is alive at its turn: what the rule rests on
        cand_now = np.nonzero(alive_now & comp)[0]
        assert not (loc[cand_now] & (cand_now < s)).any()
        want = min(sw.configs[c][2] - 1, len(cand_now) - 1)
        live = row[alive_now[row]]
        if complete:
            n_complete += 1
            assert set(cand_now.tolist()) - {s} <= set(row.tolist())
            assert len(live) >= want  # (a complete row never runs out)
        if len(live) >= want:
            n_served += 1
            assert live[:want].tolist() == members[1:], (c, s, j, i)
    assert n_served > 0
    if unlocated < 0.9:
        assert n_dropped > 0  # (the rule had something to drop)
    if unlocated == 0.0:
        assert n_complete > 0  # (every candidate located: the rows of a configuration's last seeds list fewer than ROW_K)
