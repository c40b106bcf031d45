"""One case generator for tests/test_form_model.py (CPU: the plain model of tests/form_model.py against the oracle) and
tests/test_gpu_form_rules.py (GPU: the engine against the oracle): group formation (try_form_new_groups, mod.rs:478-628)
rule by rule, and at every point where the streaming carve hands a configuration from one of its paths to the next.

    make_case(name) -> (swarm, enabled, policy kwargs, expectations)

A case is one named point; the list is explicit (CASES).  The hand-over points are read out of the kernel sources
(THRESHOLDS): a retuned constant moves the cases with it, and a constant that can no longer be read fails the import.
`expectations` carries what else a run needs (`pre_enabled`: configurations formed in a pass of their own first, so that
the case starts with standing groups) and what the case is named for (`expect`: conditions on the inputs and on the
model's records, checked in tests/test_form_model.py without a GPU).

Unless a case says otherwise every worker is eligible and located at a place of its own (no two distances from a seed are
equal: geometry alone decides), and there is one configuration without requirement, (2, 8).
"""
import os
import re

import numpy as np

from oracle import oracle_ffi as orc
from protocol_amd.swarm import ST_HEALTHY, ST_UNHEALTHY, make_swarm
from merge_cases import _seed_of, _tasks_over, enabled_bits  # noqa: F401  (enabled_bits: for the tests)
import form_model

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "protocol_amd", "csrc")


def _read_thresholds():
    stream = open(os.path.join(_CSRC, "pm_stream.inc")).read()
    device = open(os.path.join(_CSRC, "pm_device.h")).read()

    def define(name):
        m = re.search(r"^#define %s (\d+)u\b" % name, stream, re.M)
        assert m, f"{name} is no longer a plain #define in pm_stream.inc"
        return int(m.group(1))

    def constant(name):
        m = re.search(r"constexpr uint32_t %s\s*=\s*(\d+);" % name, device)
        assert m, f"{name} is no longer a plain constant in pm_device.h"
        return int(m.group(1))

    assert re.search(r"^#define STREAM_SMALL \(64u \* STREAM_SMALL_CPL\)", stream, re.M), "STREAM_SMALL is no longer 64 * STREAM_SMALL_CPL"
    small = 64 * define("STREAM_SMALL_CPL")
    m = re.search(r"^#define STREAM_SMALL_START (\w+)$", stream, re.M)
    assert m, "STREAM_SMALL_START is no longer a #define in pm_stream.inc"
    start = small if m.group(1) == "STREAM_SMALL" else int(re.fullmatch(r"(\d+)u", m.group(1)).group(1))
    assert re.search(r"const bool on_rows = n_cl <= 64u;", stream), "stream_small_rows is no longer taken at up to 64 located candidates"
    assert re.search(r"c\.steps - refresh_at >= 8u", stream), "the run-out rule is no longer `c.steps - refresh_at >= 8u`"
    return dict(STREAM_SMALL_AT=define("STREAM_SMALL_AT"), ROWS=64, STREAM_SMALL=small, STREAM_SMALL_START=start,
                STREAM_LA_ALL=define("STREAM_LA_ALL"), STREAM_SPARSE_MAX=define("STREAM_SPARSE_MAX"),
                STREAM_TAIL_MAX=define("STREAM_TAIL_MAX"), PM_CARVE_SLOTS=constant("PM_CARVE_SLOTS"),
                PM_PROP_KMAX=constant("PM_PROP_KMAX"), PM_CARVE_SEL_CAP=constant("PM_CARVE_SEL_CAP"))


THRESHOLDS = _read_thresholds()
TH = THRESHOLDS
assert TH["STREAM_SMALL"] == TH["STREAM_SMALL_START"], "the cases below take the two for one hand-over point"
C28 = ("c-2-8", 2, 8, None)

# name -> parameters of _single / a builder of its own
CASES = {}


def _case(name, **kw):
    assert name not in CASES
    CASES[name] = kw


# ---- located candidates at the configuration's entry, around every hand-over of stream_run_config: min - 1 .. max + 1,
# STREAM_SMALL_AT (the chain hands over to the register paths), 64 (stream_small_rows / stream_small_n), STREAM_SMALL_START
# (in registers from the start / the chain), STREAM_LA_ALL (all tickets at once / a window of a quarter).  `_all`: nobody
# else; `_half`: as many location-less candidates and five more, scattered among them — a first-come tail behind every
# located phase, and location-less members from in front of the seed where the last located group is filled up.
_LOCATED = sorted({0, 1, 2, 7, 8, 9, 63, 64, 65}
                  | {TH[k] + d for k in ("STREAM_SMALL_AT", "STREAM_SMALL_START", "STREAM_LA_ALL") for d in (-1, 0, 1)})
for _k in _LOCATED:
    _case(f"loc{_k}_all", n=_k, located="all", expect=dict(entry={0: _k}, eligible=_k))
    _case(f"loc{_k}_half", n=2 * _k + 5, located=("count", _k), expect=dict(entry={0: _k}, eligible=2 * _k + 5, tail=True))

# ---- exact steps over compacted positions (up to STREAM_SPARSE_MAX candidates) / over every position: no row lists 63
# neighbours, so every step of (2, 64) is an exact one; the second step sees one candidate fewer / exactly / one more
for _d, _tag in ((-1, "m1"), (0, "0"), (1, "p1")):
    _case(f"sparse_{_tag}", mm=(2, 64), n=TH["STREAM_SPARSE_MAX"] + 64 + _d, located="all",
          expect=dict(crosses=("STREAM_SPARSE_MAX", _d)))

# ---- entered large, ends small: the chain, FAST_TINY, stream_small_n, STEP_AGAIN, stream_small_rows, the tail
_case("large_to_tail", n=2437, located=("count", 2400), expect=dict(entry={0: 2400}, phases=True, last_located="prox_full", tail=True))
_case("large_to_short", n=2403, located="all", expect=dict(entry={0: 2403}, phases=True, last_located="prox_short"))

# ---- group size: the last size with a chain (max - 1 < PM_PROP_KMAX), the staging area's edge (PM_CARVE_SEL_CAP members)
_KM, _CAP = TH["PM_PROP_KMAX"], TH["PM_CARVE_SEL_CAP"]
_SIZES = [(1, 1), (1, 2), (2, 2), (3, 3), (2, _KM), (2, _KM + 1), (2, _KM + 2), (40, _KM + 1), (2, _CAP), (2, _CAP + 1), (100, 300)]
for _mm in _SIZES:
    _n = 750 if _mm[1] > 100 else 650
    _case("sz%d_%d_all" % _mm, mm=_mm, n=_n, located="all", expect=dict(group_max=min(_mm[1], _n)))
    _case("sz%d_%d_30" % _mm, mm=_mm, n=_n, located=("share", 0.30), expect=dict(group_max=min(_mm[1], _n), tail=True))
_case("sz2_%d_all" % (_CAP - 1), mm=(2, _CAP - 1), n=750, located="all", expect=dict(group_max=_CAP - 1))
# (groups of one in one go: up to STREAM_TAIL_MAX candidates / what takes over)
for _d in (-1, 0, 1):
    _n = TH["STREAM_TAIL_MAX"] + _d
    _case(f"sz1_1_n{_n}", mm=(1, 1), n=_n, located=("share", 0.30), expect=dict(entry_compatible={0: _n}, group_max=1))

# ---- first-come tails: what is left behind 40 located candidates (five full groups)
for _r in (0, 1, 2, 8, 9, TH["STREAM_TAIL_MAX"] - 1, TH["STREAM_TAIL_MAX"], TH["STREAM_TAIL_MAX"] + 1):
    _case(f"tail{_r}", n=40 + _r, located=("count", 40), expect=dict(entry={0: 40}, tail_len=_r))

# ---- eligible positions: the LDS form of the launch / its BIG instantiation (13 / 18 slot bits in the key, the wider
# tie band)
for _d, _tag in ((-1, "m1"), (0, "0"), (1, "p1")):
    _n = TH["PM_CARVE_SLOTS"] + _d
    _case(f"slots_{_tag}", n=_n, located=("share", 0.30), expect=dict(eligible=_n, tail=True))

# ---- several configurations, who is eligible, ties, proximity off (builders of their own, below)
_case("multi_req_stops", builder="req_stops", expect=dict(first_label="stop_compatible", order=[0, 1]))
_case("multi_leftovers", builder="leftovers", expect=dict(order=[0, 1], entry_total={1: 3}))
_case("multi_equal_min", builder="equal_min", expect=dict(order=[1, 0]))
_case("multi_disabled_mid", builder="disabled_mid", expect=dict(order=[0, 2]))
_case("multi_six_waves", builder="six_waves", expect=dict(order=[0, 1, 2, 3, 4, 5], wave_each=True))
_case("multi_stop_big", builder="stop_big", expect=dict(first_label="stop_compatible", order=[0, 1], big_stops=True))
_case("elig_interleaved", builder="elig", expect=dict(positions_differ=True, standing=True))
_case("tie_cities", builder="cities", located="all", expect=dict(tie="site"))
_case("tie_cities_half", builder="cities", located=("share", 0.5), expect=dict(tie="site"))
_case("tie_mirror", builder="mirror", expect=dict(tie="cross", first_tie="cross"))
_case("off_loc129_half", n=2 * (TH["STREAM_SMALL_START"] + 1) + 5, located=("count", TH["STREAM_SMALL_START"] + 1),
      policy=dict(proximity=False), expect=dict(only="first_come"))
_case("off_six_waves", builder="six_waves", policy=dict(proximity=False), expect=dict(only="first_come", order=[0, 1, 2, 3, 4, 5]))
_case("off_sz100_300_30", mm=(100, 300), n=750, located=("share", 0.30), policy=dict(proximity=False), expect=dict(only="first_come", group_max=300))


def _base(name, W, configs):
    """W workers, all Healthy with a p2p id, each located at a place of its own (distinct latitudes on the 0.0001-degree
    grid); 60 tasks over the configurations"""
    seed = _seed_of(name)
    sw = make_swarm(seed, 60, W)
    sw.configs = list(configs)
    _tasks_over(sw, list(range(len(configs))))
    sw.status[:] = ST_HEALTHY
    sw.has_p2p[:] = True
    rng = np.random.default_rng(seed)
    sw.lat[:] = np.round(25.0 + rng.permutation(350000)[:W] * 1e-4, 4)
    sw.lon[:] = np.round(rng.uniform(-125.0, 40.0, W), 4)
    sw.has_loc[:] = True
    return sw, rng


def _locate(sw, rng, pool, located):
    if located == "all":
        return
    kind, v = located
    k = v if kind == "count" else max(1, int(round(v * len(pool))))
    sw.has_loc[pool] = False
    if k:
        sw.has_loc[rng.choice(pool, size=k, replace=False)] = True


def _compat(sw):
    nodes, cfgs, _t, _e = orc.from_swarm(sw)
    return orc.compat_masks(nodes, cfgs)


def _single(name, n, located, mm=(2, 8)):
    cfg = C28 if mm == (2, 8) else ("c-%d-%d" % mm, mm[0], mm[1], None)
    W = max(n, 12)
    sw, rng = _base(name, W, [cfg])
    sw.status[n:] = ST_UNHEALTHY     # (n = 0: twelve workers, none eligible)
    _locate(sw, rng, np.arange(n), located)
    return sw, np.ones(1, dtype=np.uint8), None


def _keep_compatible(sw, cfg, n):
    """exactly n eligible workers stay compatible with configuration cfg: the others that are become unhealthy"""
    comp = np.nonzero(((_compat(sw) >> np.uint64(cfg)) & np.uint64(1) != 0) & (sw.status == ST_HEALTHY))[0]
    assert len(comp) >= n, (len(comp), n)
    sw.status[comp[n:]] = ST_UNHEALTHY
    return comp[:n]


def _req_stops(name):
    """the first configuration (min 4) has three compatible nodes among 600 free ones: it stops at once, and (2, 8) runs"""
    sw, rng = _base(name, 600, [("rare", 4, 8, "gpu:model=mi300x;gpu:count=8"), C28])
    _keep_compatible(sw, 0, 3)
    _locate(sw, rng, np.arange(600), ("share", 0.5))
    return sw, np.ones(2, dtype=np.uint8), None


def _leftovers(name):
    """(5, 8) without requirement takes 648 of 651 nodes; its leftovers — three, fewer than its min — are all (2, 2) gets"""
    sw, rng = _base(name, 651, [("c-5-8", 5, 8, None), ("c-2-2", 2, 2, None)])
    _locate(sw, rng, np.arange(651), ("share", 0.5))
    return sw, np.ones(2, dtype=np.uint8), None


def _equal_min(name):
    """two configurations of equal min: the template order (with requirements first, mod.rs:150-164) decides, not the
    order they were given in; the one without requirement takes what the other leaves"""
    sw, rng = _base(name, 700, [("b-any", 2, 5, None), ("a-count8", 2, 8, "gpu:count=8")])
    _locate(sw, rng, np.arange(700), ("share", 0.7))
    return sw, np.ones(2, dtype=np.uint8), None


def _disabled_mid(name):
    """three configurations, the middle one (which everybody would fit) is not enabled"""
    sw, rng = _base(name, 700, [("a-count8", 4, 8, "gpu:count=8"), ("b-off", 3, 6, None), ("c-any", 2, 5, None)])
    _locate(sw, rng, np.arange(700), ("share", 0.7))
    return sw, np.array([1, 0, 1], dtype=np.uint8), None


def _six_waves(name):
    """six configurations over disjoint model classes, 40 to 64 compatible nodes each, back to back in min order: each is
    carved in registers, and while one is the next two get their tickets"""
    models = ["h200", "v100", "mi300x", "l40s", "a6000", "rtx4090"]
    sw, rng = _base(name, 1100, [("m-%s" % m, 7 - i, 8, "gpu:model=%s" % m) for i, m in enumerate(models)])
    for i in range(6):
        _keep_compatible(sw, i, 64 - 4 * i)
    anyone = _compat(sw) != 0
    sw.status[~anyone] = ST_UNHEALTHY
    _locate(sw, rng, np.nonzero(sw.status == ST_HEALTHY)[0], ("share", 0.8))
    return sw, np.ones(6, dtype=np.uint8), None


def _stop_big(name):
    """min above STREAM_SMALL_START: (150, 200) over the nodes with eight GPUs has 140 compatible, all located, among 540
    free: it stops with more than 128 located candidates in hand; then (150, 200) without requirement makes two groups
    and stops for want of nodes, with 140 located ones left"""
    sw, rng = _base(name, 900, [("w-count8", 150, 200, "gpu:count=8"), ("w-any", 150, 200, None)])
    kept = _keep_compatible(sw, 0, 140)
    others = np.setdiff1d(np.nonzero(sw.status == ST_HEALTHY)[0], kept)
    sw.status[others[400:]] = ST_UNHEALTHY
    return sw, np.ones(2, dtype=np.uint8), None


def _elig(name):
    """every fourth worker unhealthy (all the other statuses in turn), every seventh without a p2p id, and the workers
    with eight GPUs in standing groups of (2, 4) from a pass of their own: the candidates' list positions differ from
    their worker indices, and the new groups' members lie between members of standing ones"""
    sw, rng = _base(name, 1400, [("pre-count8", 2, 4, "gpu:count=8"), C28])
    other = np.array([0, 1, 3, 4, 5, 6, 7], dtype=np.uint8)
    bad = np.arange(3, 1400, 4)
    sw.status[bad] = other[np.arange(len(bad)) % 7]
    sw.has_p2p[np.arange(5, 1400, 7)] = False
    _locate(sw, rng, np.arange(1400), ("share", 0.7))
    return sw, np.array([0, 1], dtype=np.uint8), np.array([1, 0], dtype=np.uint8)


def _cities(name, located):
    """5 shared sites of 60 workers each among 900 scattered ones (as row_front_cases.cities), one configuration (2, 9): a
    city's seed finds more than max at its own site, at distance 0 — the boundary falls inside the site, input order decides"""
    sw, rng = _base(name, 1200, [("c-2-9", 2, 9, None)])
    at = rng.permutation(1200)[:300]
    s_lat, s_lon = np.round(rng.uniform(25.0, 60.0, 5), 4) + 0.00005, np.round(rng.uniform(-125.0, 40.0, 5), 4)
    sw.lat[at] = s_lat[np.arange(300) % 5]
    sw.lon[at] = s_lon[np.arange(300) % 5]
    _locate(sw, rng, np.arange(1200), located)
    return sw, np.ones(1, dtype=np.uint8), None


def _mirror(name):
    """worker 0, the first seed, at (12.5, 30); three workers a little north of it at distances of their own; then three at
    (12.75, 30.25) and three at (12.75, 29.75), alternating in the input: two sites mirrored about the seed's meridian, at
    exactly the same distance (delta_lon is +0.25 / -0.25 exactly, and only its sine's square enters).  A group of 8 takes
    the seed, the three and four of the six: the boundary falls inside the tie, between a worker of one site and a worker
    of the other.  Everybody else is far north."""
    sw, _rng = _base(name, 400, [C28])
    sw.lat[0], sw.lon[0] = 12.5, 30.0
    for i, dlat in enumerate((0.01, 0.02, 0.03)):
        sw.lat[1 + i], sw.lon[1 + i] = 12.5 + dlat, 30.0
    for i in range(6):
        sw.lat[4 + i], sw.lon[4 + i] = 12.75, (30.25 if i % 2 == 0 else 29.75)
    return sw, np.ones(1, dtype=np.uint8), None


_BUILDERS = dict(single=_single, req_stops=_req_stops, leftovers=_leftovers, equal_min=_equal_min, disabled_mid=_disabled_mid,
                 six_waves=_six_waves, stop_big=_stop_big, elig=_elig, cities=_cities, mirror=_mirror)


def make_case(name):
    """-> (swarm, enabled, policy kwargs (for orc.State and for Engine alike), expectations)"""
    kw = dict(CASES[name])
    builder = kw.pop("builder", "single")
    policy = dict(group_id_seed=_seed_of(name) % 97 + 1)
    policy.update(kw.pop("policy", {}))
    expect = kw.pop("expect", {})
    sw, enabled, pre = _BUILDERS[builder](name, **kw)
    return sw, enabled, policy, dict(expect=expect, pre_enabled=pre)


def n_workers(name):
    """the case's worker count, without building it"""
    kw = CASES[name]
    if "n" in kw:
        return max(kw["n"], 12)
    return dict(req_stops=600, leftovers=651, equal_min=700, disabled_mid=700, six_waves=1100, stop_big=900, elig=1400,
                cities=1200, mirror=400)[kw["builder"]]


def oracle_state(sw, enabled, policy, x):
    """the oracle at the case's start: the standing groups of `pre_enabled` formed, their events drained"""
    nodes, cfgs, tasks, _ = orc.from_swarm(sw)
    pre = x["pre_enabled"]
    st = orc.State(nodes, cfgs, enabled=enabled if pre is None else pre, tasks=tasks, reference_shaped=False, **policy)
    if pre is not None:
        st.try_form_new_groups()
        st.drain_events()
        st.set_enabled(enabled)
    return st


def run_model(sw, st, enabled, policy):
    """the plain model over the oracle's state as it is now (before the oracle's own formation)"""
    masks = [int(m) for m in orc.compat_masks(st.nodes, st.cfgs)]
    in_group = [g >= 0 for g in st.node_to_group.tolist()]
    return form_model.form_new_groups(
        sw.status.tolist(), sw.has_p2p.tolist(), sw.has_loc.tolist(), sw.lat, sw.lon, in_group, sw.address.tolist(), sw.configs,
        list(enabled), lambda c, n: bool((masks[n] >> c) & 1), proximity=policy.get("proximity", True))


_modelled = {}


def modelled(name):
    """-> (swarm, enabled, policy, expectations, the model's result), made once per case and shared: nobody changes them"""
    if name not in _modelled:
        sw, enabled, policy, x = make_case(name)
        _modelled[name] = (sw, enabled, policy, x, run_model(sw, oracle_state(sw, enabled, policy, x), enabled, policy))
    return _modelled[name]
