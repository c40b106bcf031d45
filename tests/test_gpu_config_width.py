"""The match path at the configuration width the ABI promises (PM_MAX_CONFIGS = 64) and at every launch regime of the pair
sweep (pm_launch.inc, launch_pair_sweep), against plain references: the oracle, or numpy over the oracle's compat masks.
Every check compares the whole output; nothing is sampled.

The regimes, by the sweep's row count R (rb = ceil(R / 256) row blocks):
  R <= 16,384           512 workgroups' worth of splits                 R = 16,384 / 16,385
  rb >= 256             four rows per thread (pair_sweep_planes_kernel<4>)  R = 65,280 / 65,281 / 65,283
  rb >= 1024            back to 2,048 workgroups' worth of splits        R = 261,888 / 261,889
  R >= 200,000          the per-task orientation interns distinct masks  R = 199,999 / 200,000
                        (not at 64 configurations: there every mask is a legal key)
At 64 configurations the OR-plane shortcut is off (a task with mask ~0 goes through the selector loop) and the LDS piece
is 93 words (6,144 words / 65 planes - 1), so a split of more words is staged in several pieces."""
import numpy as np
import pytest

from oracle import oracle_ffi as orc
from protocol_amd import engine as E
from protocol_amd import host
from protocol_amd.swarm import wide_config_swarm
from helpers import engine_groups, oracle_groups

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1


def _bits(mask: int, C: int) -> np.ndarray:
    return np.array([(mask >> i) & 1 for i in range(C)], dtype=np.uint8)


def _columns(sw) -> np.ndarray:
    """the swept axis of the per-task orientation: the oracle's compat masks of the eligible workers (healthy, with p2p,
    in no group), restricted to the enabled configurations"""
    nodes, cfgs, _t, _e = orc.from_swarm(sw)
    masks = orc.compat_masks(nodes, cfgs)
    elig = (sw.status == 2) & sw.has_p2p
    return np.where(elig, masks & np.uint64(sw.enabled_mask()), np.uint64(0))


def _per_task_reference(col: np.ndarray, tm: np.ndarray, price=None):
    """first hit and hit count per task, computed once per DISTINCT topology mask: hits = (col & mask) != 0 over the
    worker axis; with prices the axis is ordered by (price, index) and the first hit is reported as a worker index"""
    order = np.lexsort((np.arange(len(col)), price)) if price is not None else np.arange(len(col))
    colv = col[order]
    u, inv = np.unique(tm, return_inverse=True)
    first = np.full(len(u), NONE, dtype=np.uint32)
    count = np.zeros(len(u), dtype=np.uint32)
    for k0 in range(0, len(u), 64):
        hits = (colv[None, :] & u[k0:k0 + 64, None]) != 0
        cnt = hits.sum(axis=1)
        idx = order[hits.argmax(axis=1)] if len(col) else np.zeros(len(cnt), dtype=np.int64)
        first[k0:k0 + 64] = np.where(cnt > 0, idx, NONE)
        count[k0:k0 + 64] = cnt
    return first[inv.ravel()], count[inv.ravel()]


def _assert_per_task(eng, want_first, want_count, what):
    best, count = eng.match_per_task()
    bad = np.nonzero((best != want_first) | (count != want_count))[0]
    assert len(bad) == 0, (what, len(bad), [(int(t), int(best[t]), int(want_first[t]), int(count[t]), int(want_count[t]))
                                            for t in bad[:5]])


# ------------------------------------------------------------------ compat masks

@pytest.mark.parametrize("W", [1, 65, 257])
def test_compat_masks_at_every_width(W):
    """compat_sliced_kernel: four slices of ceil(C / 4) configurations — C % 4 != 0 and C < 4 leave slices short or
    empty; bits 31 / 32 and 63 of the mask"""
    eng = E.Engine()
    for C in (1, 2, 3, 4, 5, 31, 32, 33, 63, 64):
        sw = wide_config_swarm(100 + C, C + 2, W, C)
        nodes, cfgs, _t, _e = orc.from_swarm(sw)
        host.load_swarm(eng, sw)
        want = orc.compat_masks(nodes, cfgs)
        assert np.array_equal(eng.compat_masks(), want), (C, W)
    eng.close()


@pytest.mark.parametrize("W", [65535, 65536, 65537])
def test_compat_masks_at_the_kernel_switch(W):
    """below 65,536 workers compat_sliced_kernel, from there compat_kernel (one worker per lane, every configuration);
    65,537 leaves a last workgroup of one worker"""
    eng = E.Engine()
    for C in (1, 3, 64):
        sw = wide_config_swarm(200 + C, C + 2, W, C)
        nodes, cfgs, _t, _e = orc.from_swarm(sw)
        host.load_swarm(eng, sw)
        got, want = eng.compat_masks(), orc.compat_masks(nodes, cfgs)
        assert np.array_equal(got, want), (C, W, np.nonzero(got != want)[0][:5])
        if C == 64:
            assert (want >> np.uint64(63)).any()
    eng.close()


# ------------------------------------------------------------------ per-task orientation (rows = tasks)

REGIME_T = [16384, 16385, 65280, 65281, 65283, 199999, 200000, 261888, 261889]


@pytest.mark.parametrize("C", [24, 63, 64])
def test_match_per_task_at_every_sweep_regime(C):
    W = 3001                                   # (not a multiple of 64: the last plane word is partial)
    sw = wide_config_swarm(300 + C, REGIME_T[-1], W, C)
    tm = sw.task_masks()
    want_first, want_count = _per_task_reference(_columns(sw), tm)
    assert (want_count > 0).any() and (want_count == 0).any()
    for variant in (0, 1):
        eng = E.Engine(sweep_variant=variant)
        host.load_swarm(eng, sw)
        for T in REGIME_T:
            eng.upload_tasks(tm[:T], sw.created_at[:T], sw.task_uid[:T])
            _assert_per_task(eng, want_first[:T], want_count[:T], (C, variant, T))
        eng.close()


def test_match_per_task_split_staged_in_several_lds_pieces():
    """C = 64, T = 16,384 rows (rb = 64: 512 / 64 = 8 splits), W = 100,003 workers: 1,563 plane words, 196 words per
    split; the LDS holds 65 planes of 93 words (6,144 / 65 - 1), so every split is staged in pieces of 93, 93 and 10
    words"""
    sw = wide_config_swarm(401, 16384, 100003, 64)
    want_first, want_count = _per_task_reference(_columns(sw), sw.task_masks())
    for variant in (0, 1):
        eng = E.Engine(sweep_variant=variant)
        host.load_swarm(eng, sw)
        _assert_per_task(eng, want_first, want_count, variant)
        eng.close()


def test_match_per_task_single_plane_rows():
    """every task names exactly one configuration, so every wave takes the single-plane path (four plane words a step,
    the first hit located inside the step); with 4 % of the workers eligible a first hit often lies past the first word
    of its step.  W = 20,001: 313 plane words, 40 a split at 16,384 rows, 15 at 65,281 (four rows per thread)"""
    sw = wide_config_swarm(900, 65281, 20001, 64)
    sw.status[np.random.default_rng(1).random(sw.W) >= 0.04] = 3          # (ST_UNHEALTHY)
    sw.restricted[:] = True
    sw.n_topo[:] = 1
    sw.topo[:, 0] = np.random.default_rng(2).integers(0, 64, sw.T)
    sw.topo[:, 1:] = -2
    tm = sw.task_masks()
    want_first, want_count = _per_task_reference(_columns(sw), tm)
    assert (want_first[want_count > 0] >= 64).any()
    for variant in (0, 1):
        eng = E.Engine(sweep_variant=variant)
        host.load_swarm(eng, sw)
        for T in (16384, 65281):
            eng.upload_tasks(tm[:T], sw.created_at[:T], sw.task_uid[:T])
            _assert_per_task(eng, want_first[:T], want_count[:T], (variant, T))
        eng.close()


@pytest.mark.parametrize("C", [63, 64])
def test_match_per_task_with_prices_at_wide_regimes(C):
    """best bid = min (price, worker index) over the candidates, with four rows per thread (65,281 rows) and with the
    per-mask interning (200,000 rows at C = 63); prices 0 and 0xFFFFFFFF, and heavy ties"""
    sw = wide_config_swarm(500 + C, 200000, 3001, C)
    rng = np.random.default_rng(C)
    price = rng.integers(0, 12, sw.W).astype(np.uint32)
    price[rng.random(sw.W) < 0.2] = 0
    price[rng.random(sw.W) < 0.2] = 0xFFFFFFFF
    sw.price[:] = price
    tm = sw.task_masks()
    want_first, want_count = _per_task_reference(_columns(sw), tm, price=price.astype(np.int64))
    for variant in (0, 1):
        eng = E.Engine(sweep_variant=variant)
        host.load_swarm(eng, sw)
        for T in (65281, 200000):
            eng.upload_tasks(tm[:T], sw.created_at[:T], sw.task_uid[:T])
            _assert_per_task(eng, want_first[:T], want_count[:T], (C, variant, T))
        eng.close()


# ------------------------------------------------------------------ reference orientation (rows = workers)

def _delete_front(eng, uid: np.ndarray, k0: int) -> int:
    """delete the first k >= k0 tasks of the list `uid` so that the swept column range starts mid-word
    (t_lo % 64 != 0)"""
    lo = eng.debug_task_space()["t_lo"]
    k = k0
    while (lo + k) % 64 == 0 or k % 64 == 0:
        k += 1
    assert k < len(uid) and eng.tasks_delete(uid[:k]) == k
    ts = eng.debug_task_space()
    assert ts["t_lo"] % 64 != 0 and ts["T"] == len(uid) - k
    return k


@pytest.mark.parametrize("C, W", [(64, 65300), (63, 3001)])
@pytest.mark.parametrize("variant", [0, 1])
def test_match_reference_orientation_with_front_deletes(C, W, variant):
    """first applicable task and count per worker (rows = workers: 65,300 of them take four rows per thread) over a
    task range that starts mid-word, against the oracle's heartbeat sweep with the engine's own groups"""
    sw = wide_config_swarm(600 + C, 700, W, C)
    eng = E.Engine(sweep_variant=variant)
    host.load_swarm(eng, sw)
    eng.form_groups()
    k = _delete_front(eng, sw.task_uid, 37)
    task, count = eng.match()
    gow, groups, members = eng.get_groups()
    cfg_of_node = np.full(sw.W, -1, dtype=np.int32)
    for g in groups:
        b, n = int(g["member_begin"]), int(g["n_members"])
        cfg_of_node[members[b:b + n]] = int(g["config"])
    assert np.array_equal(cfg_of_node >= 0, gow >= 0)
    _nodes, cfgs, tasks, _en = orc.from_swarm(sw)
    first_o, count_o = orc.pair_sweep_per_worker(tasks[k:], cfgs, cfg_of_node, threads=16)
    assert np.array_equal(count, count_o)
    assert np.array_equal(task, first_o)                       # (CHOOSE_FIRST: the first applicable task)
    assert (count_o > 0).sum() > sw.W // 4
    eng.close()


def test_seeded_chooser_at_64_configurations():
    """CHOOSE_SEEDED at C = 64 after front deletes: every worker's task, GROUP_INDEX, GROUP_SIZE and next worker against
    the oracle's filter_tasks"""
    sw = wide_config_swarm(701, 900, 2500, 64)
    kw = dict(chooser=E.CHOOSE_SEEDED, chooser_seed=99)
    nodes, cfgs, tasks, enabled = orc.from_swarm(sw)
    st = orc.State(nodes, cfgs, enabled=enabled, tasks=tasks, reference_shaped=False, **kw)
    eng = E.Engine(**kw)
    host.load_swarm(eng, sw)
    assert st.try_form_new_groups() == eng.form_groups() > 0
    assert oracle_groups(st) == engine_groups(eng)
    k = _delete_front(eng, sw.task_uid, 101)
    st.set_tasks(tasks[k:])
    _check_every_worker(eng, st, sw.W)
    eng.close()


def _check_every_worker(eng, st, W):
    task, _count = eng.match()
    served = 0
    for w in range(W):
        t, gi, gs, nxt = st.filter_tasks(w)
        a = eng.lookup(w)
        assert (-1 if a.task == NONE else a.task) == t == (-1 if task[w] == NONE else int(task[w])), w
        if t >= 0:
            assert (a.group_index, a.group_size, a.next_worker) == (gi, gs, nxt), w
            served += 1
    assert served > W // 4
    return served


# ------------------------------------------------------------------ end to end

@pytest.mark.parametrize("carve_variant", [0, 1])
@pytest.mark.parametrize("C", [33, 63, 64])
def test_form_merge_match_at_wide_configurations(C, carve_variant):
    """carve with only the top configuration (a (1, 1) one at index C - 1) enabled, merge the solos with every
    configuration enabled, carve the rest with the top bit clear, match: groups bit-exact and every worker's row"""
    sw = wide_config_swarm(800 + C, 400, 2500, C)
    sw.configs[C - 1] = ("solo-top", 1, 1, "gpu:count=8")
    nodes, cfgs, tasks, enabled = orc.from_swarm(sw)
    st = orc.State(nodes, cfgs, enabled=enabled, tasks=tasks, reference_shaped=False)
    eng = E.Engine(carve_variant=carve_variant)
    host.load_swarm(eng, sw)
    full, top = (1 << C) - 1, 1 << (C - 1)
    for mask, step in ((top, "form"), (full, "merge"), (full & ~top, "form")):
        eng.set_enabled_mask(mask)
        st.set_enabled(_bits(mask, C))
        if step == "form":
            n_e, n_o = eng.form_groups(), st.try_form_new_groups()
        else:
            n_e, n_o = eng.merge_solo_groups(), st.try_merge_solo_groups()
        assert n_e == n_o > 0, (step, hex(mask))
        assert oracle_groups(st) == engine_groups(eng), (step, hex(mask))
        if mask == top:                            # (the solos of the top configuration, for the merge to take)
            assert all(cfg == C - 1 for _i, cfg, _m, _t in engine_groups(eng))
    _check_every_worker(eng, st, sw.W)
    assert oracle_groups(st) == engine_groups(eng)
    eng.close()


# ------------------------------------------------------------------ newest_task

def _newest_ref(ca: np.ndarray) -> int:
    """Iterator::max_by_key: the LAST maximum"""
    if len(ca) == 0:
        return NONE
    return len(ca) - 1 - int(np.argmax(ca[::-1]))


@pytest.mark.parametrize("T", [1, 255, 256, 257, 65537, 300001])
def test_newest_task_ties_extremes_and_front_deletes(T):
    """created_at of INT64_MIN / INT64_MAX, ties of the maximum on both sides of a 256-row block boundary, and (300,001
    rows: more than the 1,024 x 256 threads of the launch) two maxima in one thread's rows"""
    rng = np.random.default_rng(T)
    eng = E.Engine()
    uid = np.arange(1, T + 1, dtype=np.uint64) * np.uint64(7919)
    masks = np.full(T, 2 ** 64 - 1, dtype=np.uint64)
    cases = []
    cases.append(np.full(T, INT64_MIN, dtype=np.int64))                       # everyone at the minimum: the last
    ca = rng.integers(-1000, 1000, T).astype(np.int64)
    ca[rng.random(T) < 0.1] = INT64_MIN
    cases.append(ca)
    ca = ca.copy()
    ca[rng.integers(0, T)] = INT64_MAX                                         # one task at the maximum
    cases.append(ca)
    ca = rng.integers(-50, 50, T).astype(np.int64)
    for p in (250, 255, 256, 260, 5, 5 + 262144, 262144 + 300):               # ties around a block boundary / one thread
        if p < T:
            ca[p] = INT64_MAX
    cases.append(ca)
    ca = ca.copy()
    if T > 262149:
        ca[262149:] = INT64_MIN                                                 # the thread's second maximum gone
    cases.append(ca)
    for ca in cases:
        eng.upload_tasks(masks, ca, uid)
        assert eng.newest_task() == _newest_ref(ca)
        live, live_uid = ca, uid
        if T > 1:                                  # front deletes: the scan starts mid-word
            k = _delete_front(eng, uid, 1)
            live, live_uid = ca[k:], uid[k:]
            assert eng.newest_task() == _newest_ref(live), k
            p = _newest_ref(live)                  # the newest goes: a hole in the live bitmap
            assert eng.tasks_delete(live_uid[p:p + 1]) == 1
            live, live_uid = np.delete(live, p), np.delete(live_uid, p)
            assert eng.newest_task() == _newest_ref(live), p
        assert eng.tasks_delete(live_uid) == len(live_uid)
        assert eng.debug_task_space()["T"] == 0
        assert eng.newest_task() == NONE
    eng.close()


# ------------------------------------------------------------------ the width limit

def test_sixty_five_configurations_are_refused_and_nothing_changes():
    sw = wide_config_swarm(901, 500, 2000, 64)
    eng = E.Engine()
    cfg_rows, alt_rows, _req = host.load_swarm(eng, sw)
    eng.form_groups()
    task, count = eng.match()
    before = engine_groups(eng)
    rows65 = np.concatenate([cfg_rows, cfg_rows[:1]])
    with pytest.raises(E.EngineError) as ex:
        eng.set_configs(rows65, alt_rows)
    assert ex.value.code == E.PM_EINVAL
    assert engine_groups(eng) == before
    task2, count2 = eng.match()
    assert np.array_equal(task, task2) and np.array_equal(count, count2)
    eng.form_groups()
    assert np.array_equal(eng.match()[0], task)
    eng.close()
