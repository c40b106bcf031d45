"""What every carve on the batch pipeline starts from, against references of its own: the eligible list and the candidate list
of the first configuration (carve_elig_*, carve_prep_count_kernel / carve_prep_place_kernel), the batch's seeds (prop_limit_scan,
prop_seed_slots), the spatial index of the located positions (cell_count_kernel, cell_scan_sums_kernel, cell_scan_apply_kernel,
cell_place_kernel) and a neighbour row per seed (carve_propose_kernel: tile_keys over the whole list, cell_walk over the index,
list_sweep_solo as the walk's fallback) — read back by pm_debug_first_batch_arm, which copies the buffers out behind the first
propose launch and lets the carve run on; every formation's groups are held to the oracle as well.

The references and the swarm families are tests/first_batch_cases.py's; every family is first shown to reach what it exists for
(tests/test_first_batch_model.py asserts the same on the CPU).  Keys are the device's own, from candidate_key through
pm_debug_distance_keys; a row is a function of the SET of keys its path counts (near_row_cases.Reference).  Whether a seed of a
walked batch walked or fell back the kernel does not say: the model walk (cell_walk_model.stop_ring) predicts it from the same
keys, prune_fallbacks is the count of its run-outs, and every row is held to the path it predicts.  No tolerance anywhere: whole
arrays of integers."""
import numpy as np
import pytest

import cell_walk_model as M
import first_batch_cases as F
import near_row_cases as N
from helpers import engine_groups, oracle_groups, oracle_state_for
from protocol_amd import engine as E
from protocol_amd import host

pytestmark = pytest.mark.gpu

U = np.uint64
NONE32 = 0xFFFFFFFF


def _form(sw, mode, eng=None):
    """one armed formation -> (engine, groups formed, the groups, the snapshot, the carve's counters)"""
    if eng is None:
        eng = E.Engine(carve_variant=3)
        eng.debug_prune_mode(mode)
        host.load_swarm(eng, sw)
    eng.debug_first_batch_arm()
    n = eng.form_groups()
    return eng, n, engine_groups(eng), eng.debug_first_batch(), eng.debug_carve_counters()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(U)


def _eq(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero(got != want)[0] if got.ndim == 1 else np.argwhere(got != want)
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), [(got[tuple(np.atleast_1d(b))], want[tuple(np.atleast_1d(b))]) for b in bad[:5]])


# ------------------------------------------------------------------------------------------------------------ lists and seeds
def check_lists(sw, L, s):
    n = len(L.order)
    assert (s["planned"], s["valid"], s["none"], s["ci0"]) == (1, 1, 0, 0), s
    assert (s["n_eligible"], s["total_available"]) == (n, n)
    _eq(s["order"], L.order, "order")
    cfg_bits = U((1 << len(sw.configs)) - 1)
    _eq(s["c_compat"] & cfg_bits, L.compat & cfg_bits, "c_compat")
    _eq(_bits(s["c_lat"]), _bits(np.asarray(sw.lat)[L.order]), "c_lat")
    _eq(_bits(s["c_lon"]), _bits(np.asarray(sw.lon)[L.order]), "c_lon")
    _eq(s["loc_g"], F.bitmap(L.loc), "loc_g")
    _eq(s["alive_snap"], F.bitmap(np.ones(n, dtype=bool)), "alive_snap")
    # sites: equal ids <=> equal coordinates, bit 31 <=> two or more located rows of the table there (located positions)
    want = F.model_sites(sw)[L.order]
    got = s["c_site"]
    _eq(got[L.loc] >> 31, want[L.loc] >> 31, "c_site: shared bit")
    pairs = np.stack([got[L.loc] & 0x7FFFFFFF, want[L.loc] & 0x7FFFFFFF], axis=1)
    assert len(np.unique(pairs, axis=0)) == len(np.unique(pairs[:, 0])) == len(np.unique(pairs[:, 1])), "c_site: ids"
    # the candidate list of the configuration mod.rs:505-519 picks
    assert (s["ci"], s["n_list"]) == (L.ci, L.n_list)
    _eq(s["slot_wid"], L.slot_wid, "slot_wid")
    _eq(s["slot_pos"], L.pos.astype(np.uint32) | (L.slot_loc.astype(np.uint32) << 31), "slot_pos")
    _eq(s["cc_site"], got[L.pos], "cc_site")
    _eq(s["slot_loc"], F.bitmap(L.slot_loc), "slot loc bitmap")
    _eq(s["slot_alive"], F.bitmap(np.ones(L.n_list, dtype=bool)), "slot alive bitmap")
    # the batch
    assert (s["prop_k"], s["prop_limit"], s["n_seeds"], s["cell_g"]) == (L.prop_k, L.limit, L.n_seeds, L.batch_g), s
    assert s["pruned_batches"] == (1 if L.batch_g else 0)
    _eq(s["seed_slots"], L.seed_slots, "seed_slots")
    _eq(s["seed_map"], L.seed_map, "seed_map")
    _eq(s["seed_prefix"], L.seed_prefix, "seed_prefix")


# -------------------------------------------------------------------------------------------------------------------- index
def check_index(L, s):
    g = L.index_g
    assert s["index_g"] == g
    if not g:
        assert s["n_indexed"] == 0 and all(s[k].size == 0 for k in ("cell_start", "cell_cnt", "pos_cell", "cs_of_pos", "cs_slot"))
        return
    n, loc = len(L.order), L.loc
    n_loc = int(loc.sum())
    at = np.nonzero(loc)[0]
    _, lin, _, start = M.cell_index(s["c_ux"][at], s["c_uy"][at], s["c_uz"][at], g)
    _eq(s["cell_start"], start, "cell_start")
    assert s["cell_start"][g ** 3] == s["n_indexed"] == n_loc
    assert not s["cell_cnt"].any() and s["scan_ticket"] == 0, "the scan leaves its counts and its ticket zero"
    want_cell = np.full(n, NONE32, dtype=np.int64)
    want_cell[at] = lin
    _eq(s["pos_cell"], want_cell, "pos_cell")
    e = s["cs_of_pos"].astype(np.int64)
    assert (e[~loc] == NONE32).all()
    el = e[at]
    _eq(np.sort(el), np.arange(n_loc), "cs_of_pos: one to one onto [0, n_indexed)")
    assert ((el >= start[lin]) & (el < start[lin + 1])).all(), "every position inside its own cell's range"
    for k in ("ux", "uy", "uz"):
        _eq(_bits(s["cs_" + k][el]), _bits(s["c_" + k][at]), "cs_" + k)
    _eq(s["cs_site"][el], s["c_site"][at], "cs_site")
    if L.batch_g:    # (carve_prep_place_kernel writes the entries' slots for a batch that walks)
        slot_of = np.full(n, NONE32, dtype=np.int64)
        slot_of[L.pos] = np.arange(L.n_list)
        _eq(s["cs_slot"][el], slot_of[at], "cs_slot")


# --------------------------------------------------------------------------------------------------------------------- rows
def device_keys(eng, L, s):
    """-> keys_of(seed slots): candidate_key of every (seed, slot) pair, from the positions' own coordinates"""
    lat, lon = s["c_lat"][L.pos], s["c_lon"][L.pos]

    def keys_of(seeds):
        seeds = np.asarray(seeds)
        k, n = len(seeds), L.n_list
        return eng.debug_candidate_keys(np.repeat(lat[seeds], n), np.repeat(lon[seeds], n), np.tile(lat, k), np.tile(lon, k)).reshape(k, n)
    return keys_of


def device_pair_keys(eng, L, s, chunk=1 << 22):
    """-> keys_of(seed slots, slots): candidate_key of each pair"""
    lat, lon = s["c_lat"][L.pos], s["c_lon"][L.pos]

    def keys_of(a, b):
        out = np.zeros(len(a), dtype=U)
        for c0 in range(0, len(a), chunk):
            i, j = a[c0:c0 + chunk], b[c0:c0 + chunk]
            out[c0:c0 + chunk] = eng.debug_candidate_keys(lat[i], lon[i], lat[j], lon[j])
        return out
    return keys_of


def check_rows(eng, fam, L, s, mode):
    K, ns, n_list = L.prop_k, L.n_seeds, L.n_list
    prop = s["prop"]
    assert prop.shape == (ns, E.PROP_ROW)
    if not K:
        assert ns == 0
        return None
    if not ns:          # (no located candidate: nothing proposes)
        return prop
    g = F.geometry(n_list)
    site = s["cc_site"]
    keys_of = device_keys(eng, L, s)
    # which way every seed's row was made
    if mode == 2 and L.batch_g:
        ux, uy, uz = s["c_ux"], s["c_uy"], s["c_uz"]
        if ns * n_list > F.SPARSE_ABOVE:
            stop = F.walk_stops(L, ux, uy, uz, site, device_pair_keys(eng, L, s))
        else:
            stop = F.walks(L, ux, uy, uz, site, keys_of).stop
        walked = stop != 0
        assert s["prune_fallbacks"] == int((~walked).sum()), ("prune_fallbacks", s["prune_fallbacks"], np.unique(stop, return_counts=True))
    else:
        walked = np.zeros(ns, dtype=bool)
        assert s["prune_fallbacks"] == (ns if L.batch_g else 0)

    def counted_of(idx):
        seeds = L.seed_slots[idx]
        return np.where(walked[idx][:, None], F.counted_walk(L, seeds, site), F.counted_sweep(L, seeds))

    # every seed: the entries are counted slots, strictly ascending as packed keys; n_k = min(K, |counted|); the 32-bit half
    meta, ent = prop[:, 0], prop[:, 1:64]
    half = np.ascontiguousarray(prop[:, 64:]).view("<u4").reshape(ns, 64)
    assert (meta >> U(32) == 0).all()
    _eq(half[:, 0], meta.astype(np.uint32), "the 32-bit half's flags word")
    _eq(half[:, 1:], (ent & U(g.mask)).astype(np.uint32), "the 32-bit half's slots")
    n_k = (meta & U(0xFF)).astype(np.int64)
    lanes = np.arange(63)[None, :]
    listed = lanes < n_k[:, None]
    assert (ent[~listed] == U(N.EMPTY)).all(), "nothing behind a row's entries"
    assert ((ent[:, :-1] < ent[:, 1:]) | ~listed[:, 1:]).all(), "entries strictly ascending"
    for c0 in range(0, ns, 256):
        idx = np.arange(c0, min(c0 + 256, ns))
        counted = counted_of(idx)
        _eq(n_k[idx], np.minimum(K, counted.sum(axis=1)), "n_k = min(K, |counted|)")
        slots = (ent[idx] & U(g.mask)).astype(np.int64)
        ok = np.take_along_axis(counted, np.where(listed[idx], slots, 0), axis=1) | ~listed[idx]
        assert ((slots < n_list) | ~listed[idx]).all() and ok.all(), "every entry is a counted slot"
    # the sample: the whole row against brute force over the device's keys
    idx = F.sample(fam, L)
    seeds = L.seed_slots[idx]
    want = F.expected_rows(L, F.pack(L, keys_of(seeds), counted_of(idx), site, seeds), site)
    _eq(prop[idx], want, f"rows of seeds {idx.tolist()}")
    return prop


# ----------------------------------------------------------------------------------------------------------------- the test
@pytest.mark.parametrize("gi", F.all_members(), ids=F.member_id)
def test_first_batch(gi):
    fam = F.family(gi[0])[gi[1]]
    by_mode = F.reaches(fam)                      # (before any call of the engine)
    st = oracle_state_for(fam.sw, reference_shaped=fam.sw.W <= 3000)
    n_o = st.try_form_new_groups()
    g_o = oracle_groups(st)
    rows = {}
    for mode in fam.modes:
        L = by_mode[mode]
        eng, n, groups, s, c = _form(fam.sw, mode)
        # the snapshot's own checks first, each on its own, the groups last: a fault is reported by every reference that sees it,
        # not by the group parity alone
        fired = []

        def stage(name, fn):
            try:
                return fn()
            except Exception as e:      # (a wrong list can also break the shapes the later stages index with)
                fired.append(f"mode {mode} {name}: {type(e).__name__}: {str(e)[:400]}")
                return None
        try:
            assert s["prune_mode"] == mode
            stage("lists", lambda: check_lists(fam.sw, L, s))
            stage("index", lambda: check_index(L, s))
            rows[mode] = stage("rows", lambda: check_rows(eng, fam, L, s, mode))

            def same_groups():
                assert (n, groups) == (n_o, g_o), "the snapshot disturbs nothing: the oracle's groups"
            stage("groups", same_groups)
        finally:
            eng.close()
        assert not fired, "\n".join(fired)
    if rows.get(0) is not None and rows.get(3) is not None:
        # (a batch that walks is capped by another divisor: the seeds of the shorter batch are the first of the longer one's)
        m = min(len(rows[0]), len(rows[3]))
        assert m == min(by_mode[0].n_seeds, by_mode[3].n_seeds)
        _eq(by_mode[0].seed_slots[:m], by_mode[3].seed_slots[:m], "the seeds both batches have")
        _eq(rows[0][:m], rows[3][:m], "the rows of the tiled sweep and of the walk's fallback, bit for bit")


def test_a_second_formation_snapshots_a_valid_index_again():
    """the scan's counts and ticket are left zero for the next carve: a second formation on the same engine builds the same
    index, lists and rows, and a third, unarmed one leaves no snapshot behind"""
    fam = F.family("two_configs")[0]
    L = F.lists(fam.sw, 2)
    eng, n1, g1, s1, _ = _form(fam.sw, 2)
    try:
        eng.reset_groups()
        _, n2, g2, s2, _ = _form(fam.sw, 2, eng)
        assert (n1, [g[1:] for g in g1]) == (n2, [g[1:] for g in g2])       # (the ids go on from where the first carve left them)
        check_lists(fam.sw, L, s2)
        check_index(L, s2)
        _eq(s2["prop"], s1["prop"], "the second formation's rows")
        _eq(s2["cell_start"], s1["cell_start"], "cell_start")
        eng.reset_groups()
        assert eng.form_groups() == n1
        s3 = eng.debug_first_batch()                      # (unarmed: the second formation's snapshot stands as it was)
        assert all(np.array_equal(s3[k], s2[k]) for k in s2), "an unarmed formation touches no snapshot"
        eng.debug_first_batch_arm()                       # arming drops the old one; until a formation runs there is none
        with pytest.raises(E.EngineError) as ei:
            eng.debug_first_batch()
        assert ei.value.code == E.PM_ESTATE
    finally:
        eng.close()


def test_the_streaming_carve_refuses_the_snapshot():
    eng = E.Engine(carve_variant=0)
    try:
        with pytest.raises(E.EngineError) as ei:
            eng.debug_first_batch_arm()
        assert ei.value.code == E.PM_ESTATE
    finally:
        eng.close()


def test_an_arm_ends_with_its_formation():
    """a formation that has nothing to carve (no configuration enabled) takes no snapshot, and the arm is not carried over to
    the formation behind it"""
    fam = F.family("caps")[0]
    eng = E.Engine(carve_variant=3)
    try:
        host.load_swarm(eng, fam.sw, enabled=0)
        eng.debug_first_batch_arm()
        assert eng.form_groups() == 0
        with pytest.raises(E.EngineError) as ei:
            eng.debug_first_batch()
        assert ei.value.code == E.PM_ESTATE
        eng.set_enabled_mask(fam.sw.enabled_mask())
        assert eng.form_groups() > 0
        with pytest.raises(E.EngineError) as ei:
            eng.debug_first_batch()
        assert ei.value.code == E.PM_ESTATE
    finally:
        eng.close()
