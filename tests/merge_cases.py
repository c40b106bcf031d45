"""One case generator for tests/test_merge_model.py (CPU: the plain model against the oracle) and
tests/test_gpu_merge_rules.py (GPU: the engine against the oracle).

Every case starts like test_gpu_scale.py::test_solo_merge_at_baseline_size: the solo-making (1, 1) configuration(s) are
enabled alone and formed — every eligible node becomes a group of one — then the merge configurations are enabled too
and try_merge_solo_groups (mod.rs:631-971) runs.  A case is one named point; the list is explicit (CASES).

    make_case(name) -> (swarm, enabled_first, policy kwargs, expectations)

`expectations` carries what else a run needs (enabled_merge, hold_tasks) and what the case is named for (`expect`:
conditions on the INPUTS that tests/test_merge_model.py checks with the model, so that a case that stops reaching its
branch fails there, without a GPU).
"""
import numpy as np

from oracle import oracle_ffi as orc
from protocol_amd.swarm import ST_HEALTHY, ST_UNHEALTHY, make_swarm
from helpers import oracle_groups
import merge_model

SOLO = ("solo", 1, 1, None)

# name -> parameters of _single / a builder of its own
CASES = {}


def _case(name, **kw):
    assert name not in CASES
    CASES[name] = kw


# ---- (min, max) x located share: one merge configuration without requirement over 650 solo groups
_case("m1_2_one", mm=(1, 2), located=("count", 1), expect=dict(zero_merges=True))
_case("m1_2_all", mm=(1, 2), located="all")
_case("m1_1_1_3_all", mm=(1, 3), located="all", extra=[("single", 1, 1, "gpu:count=8")])
_case("m1_1_1_3_none", mm=(1, 3), located="none", extra=[("single", 1, 1, "gpu:count=8")])
_case("m2_8_all", mm=(2, 8), located="all")
_case("m2_8_30", mm=(2, 8), located=("share", 0.30), policy=dict(chooser=orc.CHOOSE_SEEDED, chooser_seed=77))
_case("m2_8_none", mm=(2, 8), located="none")
_case("m2_8_one", mm=(2, 8), located=("count", 1))
_case("m3_3_30", mm=(3, 3), located=("count", 194), expect=dict(cleared2=20))
_case("m3_3_min1", mm=(3, 3), located=("count", 2), expect=dict(cleared2=1))
_case("m3_3_all", mm=(3, 3), located="all")
_case("m3_8_30", mm=(3, 8), located=("share", 0.30))
_case("m3_8_1", mm=(3, 8), located=("share", 0.01))
_case("m3_8_all", mm=(3, 8), located="all")
_case("m3_8_sites", mm=(3, 8), located="all", sites=True)
_case("m5_16_1", mm=(5, 16), located=("count", 4), expect=dict(cleared2=5))
_case("m5_16_none", mm=(5, 16), located="none")
_case("m5_16_all", mm=(5, 16), located="all")
_case("m6_6_1", mm=(6, 6), located=("count", 9), expect=dict(cleared2=20))
_case("m6_6_30", mm=(6, 6), located=("share", 0.30), expect=dict(cleared2=20))
_case("m6_6_min1", mm=(6, 6), located=("count", 5), expect=dict(cleared2=20))
_case("m8_8_1", mm=(8, 8), located=("share", 0.01), expect=dict(cleared2=20))
_case("m8_8_30", mm=(8, 8), located=("share", 0.30), expect=dict(cleared2=20))
_case("m8_8_all", mm=(8, 8), located="all")
_case("m2_63_all", mm=(2, 63), located="all")
_case("m2_63_30", mm=(2, 63), located=("share", 0.30))
_case("m2_64_all", mm=(2, 64), located="all")
_case("m3_65_30", mm=(3, 65), located=("share", 0.30))
_case("m3_65_min1", mm=(3, 65), located=("count", 2), expect=dict(cleared2=1))
_case("m4_66_all", mm=(4, 66), located="all", expect=dict(group_over=65))
_case("m4_66_min1", mm=(4, 66), located=("count", 3), expect=dict(cleared2=1, group_over=65))
_case("m4_70_all", mm=(4, 70), located="all", expect=dict(group_over=65))
_case("m4_70_30", mm=(4, 70), located=("share", 0.30), expect=dict(group_over=65))
_case("m2_200_30", mm=(2, 200), located=("share", 0.30), expect=dict(group_over=65))
_case("m2_200_none", mm=(2, 200), located="none", expect=dict(group_over=65))
_case("m2_300_all", mm=(2, 300), located="all", n=700, expect=dict(group_over=257))
_case("m2_300_one", mm=(2, 300), located=("count", 1), n=700, expect=dict(group_over=257))
_case("m5_300_min1", mm=(5, 300), located=("count", 4), n=700, expect=dict(cleared2=1, group_over=257))

# ---- list length: around the streaming merge's threshold (512 by default, "8" in tests), around the point where the
# streaming carve's chain leaves the located candidates to exact steps (STREAM_SMALL_START = 128), n_rem around min and
# max, and more candidates than the LDS form of the exact step holds (PM_CARVE_SLOTS = 8,192)
for _n in (2, 3, 4, 7, 8, 9, 15):   # (3, 8): min - 1, min, min + 1, max - 1, max, max + 1, 2 max - 1
    _case(f"len{_n}_3_8_all", mm=(3, 8), located="all", n=_n)
    _case(f"len{_n}_3_8_half", mm=(3, 8), located=("share", 0.5), n=_n)
for _n in (511, 512, 513):
    _case(f"len{_n}_3_8_30", mm=(3, 8), located=("share", 0.30), n=_n)
for _k in (127, 128, 129, 140):
    _case(f"loc{_k}_3_8", mm=(3, 8), located=("count", _k), n=600)
_case("big_5_16_30", mm=(5, 16), located=("count", 3748), n=12500, expect=dict(cleared2=1, list_over=8192))

# ---- policies
_case("sw_off_3_8_30", mm=(3, 8), located=("share", 0.30), policy=dict(switching=False), expect=dict(zero_merges=True))
_case("prox_off_3_8_30", mm=(3, 8), located=("share", 0.30), policy=dict(proximity=False))
_case("hold_3_8_30", mm=(3, 8), located=("share", 0.30), hold_tasks=True)
_case("hold_8_8_all", mm=(8, 8), located="all", hold_tasks=True)

# ---- builders of their own (below)
_case("multi_30", builder="multi", located=("share", 0.30), expect=dict(shrinks=True, cleared2=1))
_case("multi_all", builder="multi", located="all", expect=dict(shrinks=True))
_case("multi_1", builder="multi", located=("share", 0.01), expect=dict(shrinks=True))
_case("multi_hold_all", builder="multi", located="all", hold_tasks=True, expect=dict(shrinks=True))
# (salt: which seeded swarm; chosen, with the model, so that the blocked batch is the seventh / the fifth / the first)
_case("blocked_later_all", builder="blocked", located="all", salt=3, expect=dict(blocked_later=True))
_case("blocked_later_30", builder="blocked", located=("share", 0.30), salt=3, expect=dict(blocked_later=True))
_case("blocked_first_all", builder="blocked", located="all", expect=dict(blocked=True))


def _seed_of(name):
    return 1000 + sum((i + 1) * ord(c) for i, c in enumerate(name)) % 9000


def _tasks_over(sw, names_cfg):
    """task i names configuration names_cfg[i % len]; every fifth task is unrestricted"""
    T = sw.T
    sw.topo[:] = -2
    sw.topo[:, 0] = np.asarray(names_cfg, dtype=np.int16)[np.arange(T) % len(names_cfg)]
    sw.n_topo[:] = 1
    sw.restricted[:] = True
    free = np.arange(T) % 5 == 4
    sw.restricted[free] = False
    sw.n_topo[free] = 0
    sw.topo[free] = -2


def _trim(sw, n):
    """exactly n nodes stay eligible (healthy, with a p2p id): the others a carve could take are made unhealthy"""
    elig = np.nonzero((sw.status == ST_HEALTHY) & sw.has_p2p)[0]
    assert len(elig) >= n, (len(elig), n)
    sw.status[elig[n:]] = ST_UNHEALTHY
    return elig[:n]


def _locate(sw, pool, located, seed, sites=False):
    rng = np.random.default_rng(seed)
    if located == "all":
        sw.has_loc[:] = True
    else:
        sw.has_loc[:] = False
        if located != "none":
            kind, v = located
            k = v if kind == "count" else max(1, int(round(v * len(pool))))
            sw.has_loc[rng.choice(pool, size=min(k, len(pool)), replace=False)] = True
    if sites:   # a handful of sites, two pairs of them mirrored about a meridian: exact distance ties inside a batch
        which = rng.integers(0, 5, sw.W)
        sw.lat[:] = np.where(which == 4, 14.0, 12.5)
        sw.lon[:] = np.array([30.0, 30.25, 29.75, 30.5, 29.5])[which]


def _single(name, mm, located, n=650, extra=(), sites=False):
    seed = _seed_of(name)
    sw = make_swarm(seed, 60, int(n * 1.15) + 60)
    sw.configs = [SOLO, ("merge-%d-%d" % mm, mm[0], mm[1], None)] + list(extra)
    _tasks_over(sw, list(range(len(sw.configs))))
    pool = _trim(sw, n)
    _locate(sw, pool, located, seed, sites)
    enabled_first = np.zeros(len(sw.configs), dtype=np.uint8)
    enabled_first[0] = 1
    for i, c in enumerate(sw.configs):      # (further (1, 1) configurations form solo groups too)
        if (c[1], c[2]) == (1, 1):
            enabled_first[i] = 1
    return sw, enabled_first, np.ones(len(sw.configs), dtype=np.uint8)


def _multi(name, located):
    """three merge configurations with different requirements and different min whose compatible sets overlap — the
    available order (min descending) decides who gets the shared solos — and a fourth that stays disabled"""
    seed = _seed_of(name)
    sw = make_swarm(seed, 80, 900)
    sw.configs = [SOLO, ("c-any", 2, 6, None), ("a-count1", 4, 8, "gpu:count=1"), ("d-off", 5, 9, "gpu:count=2"),
                  ("b-h100-a100", 3, 5, "gpu:model=h100,a100")]
    _tasks_over(sw, [0, 1, 2, 4])
    pool = _trim(sw, 700)
    _locate(sw, pool, located, seed)
    return sw, np.array([1, 0, 0, 0, 0], dtype=np.uint8), np.array([1, 1, 1, 0, 1], dtype=np.uint8)


def _blocked(name, located, salt=0):
    """prefer_larger_groups = false with tasks held by a few of the solos only (those of `solo-b`: every task names that
    configuration or a merge configuration), arranged so that the first batches of `m-any` apply and a LATER one holds
    a solo with a task: that batch is refused, the rest of `m-any` does not run, and the next configuration (`m-a`,
    over solos without tasks) still does"""
    seed = _seed_of(name) + salt
    sw = make_swarm(seed, 60, 1500)
    sw.configs = [("solo-a", 1, 1, "gpu:count=1"), ("solo-b", 1, 1, "gpu:count=2;gpu:model=h100"), ("m-any", 3, 4, None),
                  ("m-a", 2, 3, "gpu:count=1")]
    _tasks_over(sw, [1, 2, 3])
    free = ~sw.restricted                    # (no unrestricted task here: it would serve solo-a too)
    sw.restricted[free] = True
    sw.n_topo[free] = 1
    sw.topo[free, 0] = 1
    pool = _trim(sw, 1300)
    _locate(sw, pool, located, seed)
    return sw, np.array([1, 1, 0, 0], dtype=np.uint8), np.ones(4, dtype=np.uint8)


def make_case(name):
    """-> (swarm, enabled_first, policy kwargs (for orc.State and for Engine alike), expectations)"""
    kw = dict(CASES[name])
    builder = kw.pop("builder", "single")
    policy = dict(group_id_seed=_seed_of(name) % 97 + 1)
    policy.update(kw.pop("policy", {}))
    expect = kw.pop("expect", {})
    hold = kw.pop("hold_tasks", False)
    if builder == "single":
        sw, first, merge = _single(name, **kw)
    elif builder == "multi":
        sw, first, merge = _multi(name, **kw)
    else:
        sw, first, merge = _blocked(name, **kw)
        policy["prefer_larger"] = False
        hold = True
    return sw, first, policy, dict(enabled_merge=merge, hold_tasks=hold, expect=expect)


def enabled_bits(enabled) -> int:
    return sum(1 << i for i, e in enumerate(enabled) if e)


def oracle_solo_pass(sw, enabled_first, policy, x):
    """the oracle after the solo pass (and, where the case says so, after every node asked for its task: solo groups
    that hold tasks), its events drained -> (state, [task per worker] or None)"""
    nodes, cfgs, tasks, _ = orc.from_swarm(sw)
    st = orc.State(nodes, cfgs, enabled=enabled_first, tasks=tasks, reference_shaped=False, **policy)
    st.try_form_new_groups()
    held = [st.get_task_for_node(w) for w in range(sw.W)] if x["hold_tasks"] else None
    return st, held


def run_model(sw, st, policy, x):
    """the plain model over the oracle's groups as they are now (before the oracle's own merge)"""
    masks = orc.compat_masks(st.nodes, st.cfgs)
    avail = merge_model.available_order(sw.configs, x["enabled_merge"])
    return merge_model.merge_solo_groups(
        oracle_groups(st), sw.has_loc, sw.lat, sw.lon, lambda c, n: bool((int(masks[n]) >> c) & 1), avail,
        [(c[1], c[2]) for c in sw.configs], proximity=policy.get("proximity", True), switching=policy.get("switching", True),
        prefer_larger=policy.get("prefer_larger", True))
