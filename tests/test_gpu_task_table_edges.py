"""The task table's deltas at every word, pass and rebuild edge, against tests/task_table_model.py: a plain list
of (mask, created_at, uid) rows that knows nothing of handles, live words, prefixes or planes.

After EVERY operation Rig.check compares, for every worker and every task (nothing is sampled):
  pm_debug_carve_prof's view of the index space with the model's shadow (the proof that the case stood on its edge);
  the standing groups — which survived the deletes, and the position of the task each one holds;
  pm_task_report (before any match of the check: its own scratch prefix while the table's is stale; and again behind it);
  pm_newest_task; pm_lookup_task_for_worker of every worker, before the match (the rows a delta patched) and behind it;
  pm_match_per_task of every task; pm_match's count and task of every worker — on two engines, sweep_variant 0 and 1.
Where a case is about the planes every group is dissolved and carved again first (one configuration at a time, so that every
one of the 24 planes is read by some worker's row), and every group reaches the sweep unclaimed; the rebuild cases keep
their claims.

The masks are detectors (task_table_model.detector_masks): neighbours in the index space, and rows a word apart, name
different single configurations, and the swarm's per-configuration candidate counts are pairwise distinct and non-zero
(asserted on the reference before any GPU call) — a plane bit one handle off, or an output row one position off, cannot
coincide with its neighbour's."""
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import oracle_ffi as orc
from protocol_amd import engine as E
from protocol_amd import host
import task_table_model as M
from helpers import engine_groups, oracle_groups

pytestmark = pytest.mark.gpu

NONE = M.NONE
C = 24
W = 1501
FULL = (1 << C) - 1
SHADOW_KEYS = ("t_lo", "t_cap", "T", "t_dead", "regrowths", "compactions")


@pytest.fixture(scope="module")
def ctx():
    sw = M.detector_swarm(17, W, C)     # (a seed with which the carve below gives every configuration a group: check() asserts it)
    # (small groups, so that a carve of one configuration at a time leaves workers for the next)
    sw.configs = [(name, 1, 1 + c % 3, req) for c, (name, _mn, _mx, req) in enumerate(sw.configs)]
    col = M.eligible_columns(sw)
    counts = M.candidate_counts(col, C)
    assert (counts > 0).all() and len(set(counts.tolist())) == C, counts          # before any GPU call
    _nodes, cfgs, _tasks, _en = orc.from_swarm(sw)
    cfg_rows, alt_rows, req_models = host.pack_configs(sw.configs)
    return SimpleNamespace(sw=sw, col=col, counts=counts, cfgs=cfgs, order=np.argsort(counts, kind="stable"),
                           cfg_rows=cfg_rows, alt_rows=alt_rows, bits=host.build_model_table(req_models, sw.model_names),
                           n_req=len(req_models), workers=host.pack_workers(sw), memo={})


class Rig:
    """engines (one per sweep variant) and the model, moved together"""

    def __init__(self, ctx, variants=(0, 1), **kw):
        self.ctx, self.C = ctx, C
        self.engines = [E.Engine(sweep_variant=v, **kw) for v in variants]
        for e in self.engines:
            e.set_configs(ctx.cfg_rows, ctx.alt_rows)
            e.set_model_table(ctx.bits, ctx.n_req, len(ctx.sw.model_names))
            e.upload_workers(ctx.workers)
            e.set_enabled_mask(FULL)
        self.tab = M.Table(self.engines)
        self.claims = [dict() for _ in self.engines]          # group id -> claim (see _claim), per engine
        self.published = [False] * len(self.engines)
        self.g_lo, self.next_uid, self.clock = 0, 1 << 32, 1_000_000
        self._otasks = None

    def close(self):
        for e in self.engines:
            e.close()

    @property
    def list(self):
        return self.tab.list

    @property
    def shadow(self):
        return self.tab.shadow

    # ---- operations (detector rows; g counts downwards for rows inserted in front)
    def _stamps(self, n):
        created = self.clock + 1 + (n - 1 - np.arange(n)) // 2            # descending, in tied pairs
        self.clock += n + 1
        return created.astype(np.int64)

    def _uids(self, n, ids):
        if not ids:
            return None
        self.next_uid += n
        return np.arange(self.next_uid - n, self.next_uid, dtype=np.uint64)

    def upload(self, n, ids=True, masks=None, g0=0):
        assert ids or not any(self.claims), "a table without ids is uploaded under no standing claim here"
        self.g_lo = g0
        masks = M.detector_masks(np.arange(g0, g0 + n), self.C) if masks is None else masks
        self.tab.upload(masks, self._stamps(n), self._uids(n, ids))
        self._otasks = None

    def insert(self, n, ids=True, masks=None):
        self.g_lo -= n
        masks = M.detector_masks(np.arange(self.g_lo, self.g_lo + n), self.C) if masks is None else masks
        self.tab.insert_front(masks, self._stamps(n), self._uids(n, ids))
        self._otasks = None

    def delete(self, uids):
        n = self.tab.delete(uids)
        self._otasks = None
        return n

    def delete_positions(self, positions):
        positions = np.asarray(positions, dtype=np.int64)
        assert self.delete(self.list.uid[positions]) == len(positions)

    def delete_handles(self, handles):
        """tombstones into these cells of the index space (the shadow says which rows stand there)"""
        self.delete_positions(self.shadow.positions_of_handles(handles))

    def build_planes(self):
        """a match with the groups as they are: the planes and the prefix are built"""
        for k, e in enumerate(self.engines):
            e.match()
            self.published[k] = True
            self._note_claims(k, e)

    # ---- claims: a task's identity is its id, or (a table without ids only grows in front) its distance from the end
    def _claim(self, pos):
        if pos == NONE:
            return None
        return ("uid", int(self.list.uid[pos])) if self.list.uid is not None else ("end", len(self.list) - pos)

    def _claimed_pos(self, claim):
        if claim is None:
            return NONE
        return self.list.position_of(claim[1]) if claim[0] == "uid" else len(self.list) - claim[1]

    def _note_claims(self, k, eng):
        _gow, groups, _m = eng.get_groups()
        for g in groups:
            gid, t = int(g["id"]), int(g["task"])
            if self.claims[k].get(gid) is None:
                self.claims[k][gid] = self._claim(t)

    def _oracle_tasks(self):
        if self._otasks is None:
            self._otasks = self.list.oracle_tasks(self.ctx.cfgs[:self.C])
        return self._otasks

    def carve_every_configuration(self, eng):
        for c in self.ctx.order:
            if c < self.C:
                eng.set_enabled_mask(1 << int(c))
                eng.form_groups()
        eng.set_enabled_mask((1 << self.C) - 1)

    # ---- the checks
    def check(self, replane=True, what=""):
        lst, sh, ctx, Cn = self.list, self.shadow, self.ctx, self.C
        T = len(lst)
        col_all = ctx.col & np.uint64((1 << Cn) - 1)
        sweeps = {}
        for k, eng in enumerate(self.engines):
            tag = (what, "variant", k)
            ts = eng.debug_task_space()
            assert {key: ts[key] for key in SHADOW_KEYS} == sh.state(), tag
            assert eng.T == T
            claims = self.claims[k]
            # -- the groups that stand, and the task each holds, by the list
            gow, groups, members = eng.get_groups()
            want_ids = {gid for gid, cl in claims.items() if cl is None or self._claimed_pos(cl) != NONE}
            assert {int(g["id"]) for g in groups} == want_ids, tag
            glist, task_of_w = [], np.full(W, NONE, dtype=np.int64)
            for g in groups:
                pos = self._claimed_pos(claims[int(g["id"])])
                assert int(g["task"]) == pos, tag
                b, n = int(g["member_begin"]), int(g["n_members"])
                glist.append((int(g["config"]), n, -1 if pos == NONE else pos))
                task_of_w[members[b:b + n]] = pos
            self._check_report(eng, glist, tag)                       # (the table's prefix is stale behind a delta)
            assert eng.newest_task() == lst.newest(), tag
            if self.published[k]:
                for w in range(W):
                    assert eng.lookup(w).task == task_of_w[w], (tag, w)
            # -- per task
            if replane:
                eng.reset_groups()
                claims.clear()
                col, memo = col_all, ctx.memo.setdefault(Cn, {})
            else:
                col, memo = np.where(gow < 0, col_all, np.uint64(0)), None
            best, count = eng.match_per_task()
            want_best, want_count = lst.per_task(col, memo)
            bad = np.nonzero((best != want_best) | (count != want_count))[0]
            assert len(bad) == 0, (tag, len(bad), [(int(t), int(best[t]), int(want_best[t]), int(count[t]), int(want_count[t]))
                                                   for t in bad[:5]])
            # -- per worker
            if replane:
                self.carve_every_configuration(eng)
            task, cnt = eng.match()
            self.published[k] = True
            gow, groups, members = eng.get_groups()
            cfg_of_node = np.full(W, -1, dtype=np.int32)
            for g in groups:
                b, n = int(g["member_begin"]), int(g["n_members"])
                cfg_of_node[members[b:b + n]] = int(g["config"])
            assert np.array_equal(cfg_of_node >= 0, gow >= 0)
            if replane:
                assert set(cfg_of_node[cfg_of_node >= 0].tolist()) == set(range(Cn)), tag   # every plane has a reader
            key = cfg_of_node.tobytes()
            if key not in sweeps:
                sweeps[key] = orc.pair_sweep_per_worker(self._oracle_tasks(), ctx.cfgs[:Cn], cfg_of_node, threads=16)
            first_o, cnt_o = sweeps[key]
            assert np.array_equal(cnt, cnt_o), (tag, np.nonzero(cnt != cnt_o)[0][:5])
            want_task = first_o.astype(np.int64)
            glist = []
            for g in groups:
                gid = int(g["id"])
                b, n = int(g["member_begin"]), int(g["n_members"])
                if claims.get(gid) is not None:                       # (a claim is kept: SETNX)
                    want_task[members[b:b + n]] = self._claimed_pos(claims[gid])
                pos = int(want_task[members[b]])
                assert int(g["task"]) == pos, (tag, gid)
                claims[gid] = self._claim(pos)
                glist.append((int(g["config"]), n, -1 if pos == NONE else pos))
            bad = np.nonzero(task != want_task)[0]
            assert len(bad) == 0, (tag, len(bad), [(int(w), int(task[w]), int(want_task[w])) for w in bad[:5]])
            for w in range(W):
                assert eng.lookup(w).task == want_task[w], (tag, w)
            self._check_report(eng, glist, tag)
        return self

    def _check_report(self, eng, glist, tag):
        got = eng.task_report()
        want = self.list.task_report(glist, self.C)
        for name, g, w in zip(("groups_running", "workers_running", "groups_allowed"), got, want):
            assert np.array_equal(g, w), (tag, name, np.nonzero(g != w)[0][:5])


@pytest.fixture
def rig(ctx):
    r = Rig(ctx)
    yield r
    r.close()


# ------------------------------------------------------------------ hole patterns

PATTERNS = ("single", "all_but_63", "all_but_0", "dead_word")


def _holes(pattern, word, first_live_bit=None):
    """the cells of 64-handle word `word` a pattern kills; first_live_bit: the bit of t_lo when the word holds it (that cell
    and the ones in front of it are left alone: a dead t_lo would be trimmed, not a tombstone)"""
    bits = {"single": [37], "all_but_63": range(0, 63), "all_but_0": range(1, 64), "dead_word": range(0, 64)}[pattern]
    lo = -1 if first_live_bit is None else first_live_bit
    return [word * 64 + b for b in bits if b > lo]


# ------------------------------------------------------------------ the insertion's patched words

@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("r", [0, 1, 63])
def test_insertion_patches_words_with_tombstones(rig, r, pattern):
    """planes built by a match over a LARGER table first (so the plane words in front of the table hold another table's
    bits), then front deletes to t_lo % 64 == r, tombstones in the word of t_lo and in the next one, and n rows in front"""
    for n in (1, 2, 63, 64, 65, 127, 128, 129):
        rig.upload(640, g0=1000)
        rig.build_planes()
        rig.upload(448)
        rig.build_planes()
        lo = rig.shadow.t_lo
        assert lo % 64 == 0
        if r:
            rig.delete_positions(np.arange(r))
        lo += r
        assert rig.shadow.t_lo == lo and lo % 64 == r
        rig.delete_handles(_holes(pattern, lo // 64, r) + _holes(pattern, lo // 64 + 1))
        assert rig.shadow.t_lo == lo and rig.shadow.t_dead > 0
        for e in rig.engines:                                      # (the deletes alone, before the patch)
            assert {k: e.debug_task_space()[k] for k in SHADOW_KEYS} == rig.shadow.state()
        rig.insert(n)
        assert rig.shadow.t_lo == lo - n
        rig.check(what=(r, pattern, n))


def test_insertion_before_any_match_skips_the_patch(rig):
    rig.upload(200)
    rig.delete_positions([0, 1, 2, 70, 71])
    rig.insert(65)
    rig.check(what="no planes yet")
    rig.insert(3)                                                  # (and one with planes, into the same word)
    rig.check(what="patched")


def test_insertion_after_the_configurations_changed(rig):
    """pm_set_configs between a match and the insertion: the planes are stale as a whole, the patch is skipped, and the next
    match builds them for the new width — bits 20 .. 23 of every mask are bits at or above C now"""
    rig.upload(300)
    rig.check(what="24 configurations")
    for e in rig.engines:
        e.reset_groups()
    rig.claims = [dict() for _ in rig.engines]
    rig.C = 20
    for e in rig.engines:
        e.set_configs(rig.ctx.cfg_rows[:20], rig.ctx.alt_rows)
        e.set_enabled_mask((1 << 20) - 1)
    rig._otasks = None
    rig.delete_positions([5, 64, 65])
    rig.insert(70)
    rig.check(what="20 configurations")
    assert ((rig.list.mask & np.uint64(FULL)) >> np.uint64(20) != 0).sum() > 30


# ------------------------------------------------------------------ the delete kernel

def test_delete_kernel_words_and_odd_calls(rig):
    rig.upload(64 * 6)
    rig.delete_positions([3, 4])                                   # before any match: no planes yet
    rig.check(what="delete before any match")
    lo = rig.shadow.t_lo
    assert lo % 64 == 0
    rig.delete_handles(range(lo + 128, lo + 192))                  # all 64 handles of one word, one call
    assert rig.shadow.t_dead == 66
    rig.check(what="a whole word")
    rig.delete_handles(range(lo + 193, lo + 256))                  # 63 of the next
    rig.check(what="63 of a word")
    u = rig.list.uid
    assert rig.delete([u[10], u[10], u[11], u[10]]) == 2           # the same id twice
    assert rig.delete([7, 8, 9]) == 0                              # ids nobody holds
    assert rig.delete([u[20], 7, u[20]]) == 1
    assert rig.delete([]) == 0
    rig.check(what="odd calls")


def test_delete_the_only_unrestricted_task_of_a_word(rig):
    """one ~0 task among single-configuration ones of which none names configuration 5: it is the only bit of the whole
    table in plane 5 (and sets its bit in every other plane and in the OR plane); then it goes, and the workers of
    configuration 5's groups go from one hit to none.  (The task table's OR plane itself has no reader: the reference
    orientation's rows select one plane each — DESIGN 3.1.)"""
    n = 256
    cfg = M.detector_config(np.arange(n), C)
    masks = (np.uint64(1) << np.where(cfg == 5, 6, cfg).astype(np.uint64)).astype(np.uint64)
    masks[100] = M.ALL
    rig.upload(n, masks=masks)
    rig.check(what="with the unrestricted task")
    rig.delete_positions([100])
    rig.check(what="without it")
    assert not ((rig.list.mask >> np.uint64(5)) & np.uint64(1)).any()


# ------------------------------------------------------------------ prefix passes

@pytest.mark.parametrize("L", [63, 64, 65, 127, 128, 129])
def test_prefix_passes(rig, L):
    """a live range of L words that starts at a word index that is no multiple of 64 (the capacity comes from a first upload
    of 64 L + 544 rows: 1,024 + 2 L + 17 words) and so ends inside a pass of task_prefix_kernel; tombstones in its first
    word, in words 63 and 64 and in the last one"""
    for k, pattern in enumerate(PATTERNS):
        rig.upload(64 * L + 544, g0=77)
        rig.upload(64 * L)
        sh = rig.shadow
        assert sh.t_cap // 64 == 1024 + 2 * L + 17 and (sh.t_lo // 64) % 64 != 0 and sh.t_lo % 64 == 0
        w0 = sh.t_lo // 64
        r = None
        if k % 2:
            rig.delete_positions([0, 1, 2])                        # (the range starts mid-word)
            r = 3
        cells = []
        for w in sorted({0, 63, 64, L - 1} & set(range(L))):
            cells += _holes(pattern, w0 + w, (r if r is not None else 0) if w == 0 else None)
        rig.delete_handles(cells)
        assert rig.shadow.t_lo == w0 * 64 + (r or 0)
        rig.check(what=(L, pattern))                               # (pm_task_report first: its scratch prefix)


# ------------------------------------------------------------------ rebuild thresholds

def test_compaction_threshold_with_claims_behind_the_tombstones(rig):
    """claims on a tail of 102 rows, 4,200 rows inserted in front of it, then all but the newest of those deleted:
    t_dead == T + 4,096 exactly stands; one more delete compacts.  Positions, claims and published rows do not move."""
    rig.upload(102)
    rig.check(what="the tail")
    for n in (129, 4071):
        rig.insert(n)
    rig.check(replane=False, what="rows in front")
    assert any(rig.claims[0].values())
    rig.delete_positions(np.arange(1, 2000))
    rig.delete_positions(np.arange(1, 2201))
    sh = rig.shadow
    assert (sh.T, sh.t_dead, sh.compactions) == (103, 103 + 4096, 0)
    rig.check(replane=False, what="at the threshold")
    assert sum(cl is not None for cl in rig.claims[0].values()) > 20           # claims behind 4,199 tombstones
    claimed = {cl[1] for cl in rig.claims[0].values() if cl} | {cl[1] for cl in rig.claims[1].values() if cl}
    free = [p for p in range(1, 103) if int(rig.list.uid[p]) not in claimed]
    rig.delete_positions(free[-1:])
    assert (sh.T, sh.t_dead, sh.compactions, sh.t_lo) == (102, 0, 1, sh.t_cap - 102)
    rig.check(replane=False, what="compacted")
    rig.insert(5)                                                  # (a patch into the rebuilt space)
    rig.check(replane=False, what="compacted, then grown")
    rig.check(what="carved again")


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("extra", [0, 1])
def test_insertion_that_fits_exactly_and_one_that_regrows(ctx, variant, extra):
    """exactly t_lo new rows fit and leave t_lo == 0; t_lo + 1 rows move everything into task_capacity_for(T + n)"""
    rig = Rig(ctx, variants=(variant,))
    rig.upload(300)
    rig.delete_positions([1, 2, 3, 100])
    rig.check(what="before")
    lo, cap, T = rig.shadow.t_lo, rig.shadow.t_cap, len(rig.list)
    rig.insert(lo + extra)
    sh = rig.shadow
    if extra:
        want_cap = M.task_capacity_for(T + lo + 1)
        assert (sh.t_cap, sh.regrowths, sh.t_dead, sh.t_lo) == (want_cap, 1, 0, want_cap - T - lo - 1)
    else:
        assert (sh.t_cap, sh.regrowths, sh.t_dead, sh.t_lo) == (cap, 0, 4, 0)
    rig.check(replane=False, what="after")
    rig.close()


# ------------------------------------------------------------------ empty and back

@pytest.mark.parametrize("ids_back", [True, False])
def test_emptied_by_deletes_and_filled_again(rig, ids_back):
    rig.upload(200)
    rig.check(what="full")
    rig.delete(rig.list.uid.copy())
    sh = rig.shadow
    assert (sh.T, sh.t_dead, sh.t_lo) == (0, 0, sh.t_cap)
    rig.check(what="empty")
    for k, e in enumerate(rig.engines):
        e.tick()
        assert all(e.lookup(w).task == NONE for w in range(W))
        e.reset_groups()
        rig.claims[k].clear()
    rig.insert(70, ids=ids_back)
    rig.check(what="filled again")
    if ids_back:
        rig.delete_positions([0, 69])
        rig.check(what="and deleted from")


@pytest.mark.parametrize("ids", [True, False])
def test_uploaded_empty_without_ids_and_filled(rig, ids):
    rig.upload(0, ids=False)
    rig.check(what="empty")
    rig.insert(130, ids=ids)
    rig.check(what="filled")
    rig.insert(1, ids=ids)
    rig.check(what="one more")
    if ids:
        rig.delete_positions([64])
        rig.check(what="a hole")


# ------------------------------------------------------------------ the interned sweep with holes

N_INTERN = 201000


def _intern_masks(n_classes):
    """201,000 masks of exactly n_classes distinct valid classes: the values 1 .. n_classes - 1 three times over and ~0 (the
    class of all 24 bits); the second time over a row carries bits at or above C beside its value (the same class), and
    sprinkled in are 0 and masks of such bits only (no class)"""
    i = np.arange(N_INTERN, dtype=np.uint64)
    m = i % np.uint64(n_classes - 1) + np.uint64(1)
    second = i // np.uint64(n_classes - 1) == 1
    m = np.where(second, m | (np.uint64(1) << np.uint64(40)) | (np.uint64(1) << np.uint64(C)), m)
    m[::997] = 0
    m[5::997] = np.uint64(1) << np.uint64(50)
    m[7::997] = M.ALL
    return m.astype(np.uint64)


def _classes(masks):
    v = np.unique(masks & np.uint64(FULL))
    return len(v) - int(v[0] == 0)


def _check_per_task(rig, memo, want_path, what):
    lst = rig.list
    for eng in rig.engines:
        ts = eng.debug_task_space()
        assert {key: ts[key] for key in SHADOW_KEYS} == rig.shadow.state(), what
        assert eng.newest_task() == lst.newest()
    want_best, want_count = lst.per_task(rig.ctx.col, memo)
    for k, eng in enumerate(rig.engines):
        best, count = eng.match_per_task()
        bad = np.nonzero((best != want_best) | (count != want_count))[0]
        assert len(bad) == 0, (what, k, len(bad), bad[:5])
        assert eng.debug_per_task_path() == (want_path if k == 0 else (0, False)), (what, k)


@pytest.fixture(scope="module")
def intern_memo():
    return {}


def _punch_interior(rig, n_classes):
    """1,200 tombstones inside, every one a row whose class two other live rows carry (the same value one and two periods on,
    or before)"""
    p = n_classes - 1 + 5000 + 40 * np.arange(1200)
    assert p.max() + n_classes - 1 < N_INTERN
    rig.delete_positions(p)


def test_interned_sweep_row_edges_with_holes(rig, intern_memo):
    """R = t_cap - t_lo counts tombstones: 200,001 and 200,000 rows are swept once per distinct mask, 199,999 row by row,
    while fewer than 200,000 tasks are alive"""
    n_classes = 60000
    masks = _intern_masks(n_classes)
    assert _classes(masks) == n_classes
    rig.upload(N_INTERN, masks=masks)
    _punch_interior(rig, n_classes)
    for front, R in ((999, 200001), (1, 200000), (1, 199999)):
        rig.delete_positions(np.arange(front))
        sh = rig.shadow
        assert sh.t_cap - sh.t_lo == R and sh.t_dead >= 1000 and sh.T < 200000
        n_now = _classes(rig.list.mask)
        assert n_now == n_classes
        _check_per_task(rig, intern_memo, (n_now, True) if R >= 200000 else (0, False), R)


@pytest.mark.parametrize("n_classes", [65535, 65536, 65537])
def test_interned_sweep_fill_edge_with_holes(rig, intern_memo, n_classes):
    """65,536 distinct valid masks are still interned, 65,537 fall back to a row per task; masks that differ only in bits at
    or above C are one class"""
    masks = _intern_masks(n_classes)
    assert _classes(masks) == n_classes and len(np.unique(masks)) > n_classes + 1000
    rig.upload(N_INTERN, masks=masks)
    _punch_interior(rig, n_classes)
    rig.delete_positions(np.arange(37))
    sh = rig.shadow
    assert sh.t_cap - sh.t_lo == N_INTERN - 37 and sh.t_dead == 1200 and sh.t_lo % 64 != 0
    assert _classes(rig.list.mask) == n_classes
    _check_per_task(rig, intern_memo, (n_classes, n_classes <= 65536), n_classes)


# ------------------------------------------------------------------ the merge path's running counts

def test_merge_counts_follow_the_deltas(ctx):
    """pm_merge_solo_groups picks a merged group's task as the rank-th applicable one, from per-configuration counts the
    engine keeps across deltas once a merge has made them (cfg_app_count): merge, insert and delete (unrestricted tasks and
    bits at or above C among them), carve new solo groups, merge again — groups and their tasks against the oracle's
    try_merge_solo_groups on the model's list"""
    from protocol_amd.swarm import wide_config_swarm
    sw = wide_config_swarm(823, C + 2, 2500, C)
    sw.configs[C - 1] = ("solo-top", 1, 1, "gpu:count=8")
    kw = dict(chooser=E.CHOOSE_SEEDED, chooser_seed=4242)
    nodes, cfgs, _tasks, _en = orc.from_swarm(sw)
    eng = E.Engine(**kw)
    host.load_swarm(eng, sw)
    tab = M.Table([eng])
    tab.shadow.upload(sw.T, True)                                  # (load_swarm uploaded the swarm's own few tasks)
    n0 = 700
    tab.upload(M.detector_masks(np.arange(n0), C), 5000 - np.arange(n0), np.arange(1, n0 + 1, dtype=np.uint64))
    st = orc.State(nodes, cfgs, enabled=np.ones(C, dtype=np.uint8), tasks=tab.list.oracle_tasks(cfgs), reference_shaped=False, **kw)
    top = 1 << (C - 1)

    def bits(mask):
        return np.array([(mask >> i) & 1 for i in range(C)], dtype=np.uint8)

    def form_solos_then_merge(what):
        for mask, step in ((top, "form"), (FULL, "merge")):
            eng.set_enabled_mask(mask)
            st.set_enabled(bits(mask))
            if step == "form":
                n_e, n_o = eng.form_groups(), st.try_form_new_groups()
            else:
                n_e, n_o = eng.merge_solo_groups(), st.try_merge_solo_groups()
            assert n_e == n_o, (what, step)
            assert sorted(oracle_groups(st)) == sorted(engine_groups(eng)), (what, step)
            done[step] += n_e
        assert any(t >= 0 for _i, _c, _m, t in engine_groups(eng)), what

    done = dict(form=0, merge=0)
    form_solos_then_merge("first")                                 # (the counts are valid from here on)
    assert done["form"] > 0 and done["merge"] > 0
    first = dict(done)
    g_lo, uid, clock = 0, 10 ** 6, 10 ** 4
    for rnd in range(3):
        claimed = sorted({t for _i, _c, _m, t in engine_groups(eng) if t >= 0})
        victims = np.array(claimed[:: 2] + [len(tab.list) - 1 - rnd], dtype=np.int64)
        tab.delete(tab.list.uid[victims])
        keep = np.ones(len(tab.list) + len(tab.last_gone), dtype=bool)
        keep[tab.last_gone] = False
        n_new = (65, 1, 130)[rnd]
        g_lo -= n_new
        tab.insert_front(M.detector_masks(np.arange(g_lo, g_lo + n_new), C), clock + n_new - np.arange(n_new),
                         np.arange(uid, uid + n_new, dtype=np.uint64))
        uid += n_new
        clock += n_new + 1
        st.set_tasks(tab.list.oracle_tasks(cfgs))
        st.remap_tasks(np.where(keep, n_new + np.cumsum(keep) - 1, -1))
        ts = eng.debug_task_space()
        assert {k: ts[k] for k in SHADOW_KEYS} == tab.shadow.state()
        assert sorted(oracle_groups(st)) == sorted(engine_groups(eng)), rnd
        form_solos_then_merge(rnd)
    assert done["form"] > first["form"] and done["merge"] > first["merge"]   # (merges on counts the deltas have moved)
    assert (tab.list.mask == M.ALL).any() and ((tab.list.mask != M.ALL) & (tab.list.mask >> np.uint64(C) != 0)).any()
    eng.close()


# ------------------------------------------------------------------ a duplicated id

@pytest.mark.parametrize("map_first", [True, False])
def test_duplicated_id_names_the_first_row_in_list_order(rig, map_first):
    """include/pm_engine.h: an id two live rows carry names the first of them in list order, whether or not an earlier delete
    had built the engine's id map before the second row arrived"""
    rig.upload(150)
    rig.check(what="before")
    old = int(np.nonzero(rig.list.mask == 0)[0][-1])                # (a row no group can hold)
    assert 64 < old < 149
    x = rig.list.uid[old]
    if map_first:
        rig.delete_positions([149])                                # builds the map
    rig.g_lo -= 1
    rig.tab.insert_front(np.zeros(1, dtype=np.uint64), rig._stamps(1), np.array([x], dtype=np.uint64))   # (no group holds it either)
    rig._otasks = None
    assert rig.list.position_of(x) == 0
    rig.check(what="two rows with one id")
    assert rig.delete([x]) == 1                                    # the new row goes, the old one stays
    assert rig.list.position_of(x) == old
    rig.check(what="the first is gone")
    assert rig.delete([x, x]) == 1
    assert rig.list.position_of(x) == NONE
    rig.check(what="both are gone")
    assert rig.delete([x]) == 0
