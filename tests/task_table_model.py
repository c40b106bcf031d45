"""A plain model of the task table for tests/test_gpu_task_table_edges.py.

TaskList      the caller's list — (mask, created_at, uid) rows in get_all_tasks order — with upload / insert_front / delete,
              and every answer the engine gives about tasks derived from that list alone: the newest task, per worker the hit
              count and the first applicable position, per task (best, count), the position of a claimed uid.  No handles,
              no prefix, no planes.
IndexShadow   beside it, a shadow of the engine's index space — t_lo, t_cap, T, t_dead, regrowths, compactions — predicted
              from the rules as DESIGN 3.1 states them.  It answers nothing about tasks; it steers a test onto an edge and
              proves, against Engine.debug_task_space(), that the test stood there.
detector_masks  masks under which a plane bit one handle off, or an output row one position off, cannot pass for its
              neighbour.
"""
import numpy as np

from oracle import oracle_ffi as orc

NONE = 0xFFFFFFFF
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)
DEAD_SLACK = 4096


def task_capacity_for(n: int) -> int:
    """room for about as many insertions as there are tasks: 2 n + 65,536, rounded up to whole words"""
    return min((2 * n + 65536 + 63) & ~63, 0xFFFFFFC0)


# ------------------------------------------------------------------ detector masks

def detector_config(g, C: int):
    """the single configuration of detector row g (g: any integers, negative ones for rows inserted in front): rows g and
    g + 1 differ (by 1 or, across a multiple of 64, by 2 modulo C), rows g and g + 64 differ (by 65 modulo C); C >= 3 and
    65 % C != 0"""
    g = np.asarray(g, dtype=np.int64)
    return (g + g // 64) % C


def detector_masks(g, C: int) -> np.ndarray:
    """masks of detector rows g: one configuration each, and sprinkled in (by a hash of g) ~0 — the OR-plane shortcut —, 0,
    a mask whose only bits are at or above C (the last two give no bidder and hit nothing) and a single configuration
    with bits at or above C beside it (one class with the plain single configuration)"""
    assert 3 <= C < 64 and 65 % C != 0 and 2 % C != 0
    g = np.asarray(g, dtype=np.int64)
    m = np.uint64(1) << detector_config(g, C).astype(np.uint64)
    h = (g.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(58)          # 0..63
    high = (np.uint64(1) << np.uint64(C)) | (np.uint64(1) << np.uint64(63))
    m = np.where(h == 1, ALL, m)
    m = np.where(h == 2, np.uint64(0), m)
    m = np.where(h == 3, high, m)
    m = np.where(h == 4, m | high, m)
    return m.astype(np.uint64)


def eligible_columns(sw) -> np.ndarray:
    """the swept axis of the per-task orientation with no groups standing: the oracle's compat mask of every worker that is
    healthy and has a p2p id, 0 for the others"""
    nodes, cfgs, _t, _e = orc.from_swarm(sw)
    elig = (sw.status == 2) & sw.has_p2p
    return np.where(elig, orc.compat_masks(nodes, cfgs), np.uint64(0))


def candidate_counts(col: np.ndarray, C: int) -> np.ndarray:
    return np.array([int(((col >> np.uint64(c)) & np.uint64(1)).sum()) for c in range(C)])


def detector_swarm(seed: int, n_workers: int, C: int):
    """a wide_config_swarm (no tasks of its own worth keeping) whose per-configuration candidate counts are non-zero and
    pairwise distinct: a configuration whose count another one has already (the ones without a requirement all count
    every eligible worker) gets a ram or storage floor beside its requirement, raised until its count is new.  Then a
    per-task row written one position off cannot pass for its neighbour's: neighbours name different configurations."""
    from protocol_amd.swarm import wide_config_swarm
    sw = wide_config_swarm(seed, C + 2, n_workers, C)
    elig = (sw.status == 2) & sw.has_p2p
    seen = set()
    for c in range(C):
        name, mn, mx, req = sw.configs[c]
        key, col_v, some = ("storage_gb", sw.storage_gb, sw.storage_some) if req and "ram_mb" in req else ("ram_mb", sw.ram_mb, sw.ram_some)
        floors = np.unique(col_v[elig & some])
        j = 0
        while True:
            cnt = candidate_counts(eligible_columns(sw) >> np.uint64(c), 1)[0]
            if cnt > 0 and cnt not in seen:
                break
            assert j < len(floors), "no floor gives configuration %d a count of its own" % c
            sw.configs[c] = (name, mn, mx, (req + ";" if req else "") + "%s=%d" % (key, int(floors[j])))
            j += max(1, len(floors) // 97)
        seen.add(int(cnt))
    return sw


# ------------------------------------------------------------------ the list

class TaskList:
    def __init__(self):
        self.mask = np.zeros(0, dtype=np.uint64)
        self.created = np.zeros(0, dtype=np.int64)
        self.uid = None                                   # None: the table carries no ids

    def __len__(self):
        return len(self.mask)

    def upload(self, mask, created, uid=None):
        self.mask = np.array(mask, dtype=np.uint64)
        self.created = np.array(created, dtype=np.int64)
        self.uid = None if uid is None else np.array(uid, dtype=np.uint64)
        assert len(self.mask) == len(self.created) and (uid is None or len(self.uid) == len(self.mask))

    def insert_front(self, mask, created, uid=None):
        """new rows, newest first, in front of the list; every one newer than the newest row of the list"""
        mask, created = np.asarray(mask, dtype=np.uint64), np.asarray(created, dtype=np.int64)
        if len(mask) == 0:
            return
        assert (np.diff(created) <= 0).all()
        assert len(self) == 0 or created[-1] > self.created.max()
        if len(self) == 0:
            self.uid = None if uid is None else np.zeros(0, dtype=np.uint64)
        assert (uid is None) == (self.uid is None)
        self.mask = np.concatenate([mask, self.mask])
        self.created = np.concatenate([created, self.created])
        if uid is not None:
            self.uid = np.concatenate([np.asarray(uid, dtype=np.uint64), self.uid])

    def delete(self, uids) -> np.ndarray:
        """-> the list positions (ascending, in the list BEFORE the call) of the rows that went: per id the FIRST row in list
        order that carries it; unknown ids are ignored, an id named twice counts once"""
        assert self.uid is not None
        ids, first = np.unique(self.uid, return_index=True)          # (the first row of every id)
        want = np.unique(np.asarray(uids, dtype=np.uint64))
        k = np.searchsorted(ids, want)
        known = (k < len(ids)) & (ids[np.minimum(k, max(len(ids) - 1, 0))] == want) if len(ids) else np.zeros(len(want), dtype=bool)
        gone = np.sort(first[k[known]]).astype(np.int64)
        keep = np.ones(len(self), dtype=bool)
        keep[gone] = False
        self.mask, self.created, self.uid = self.mask[keep], self.created[keep], self.uid[keep]
        return gone

    # ---- answers
    def newest(self) -> int:
        """Iterator::max_by_key: the LAST maximum of created_at"""
        if len(self) == 0:
            return NONE
        return len(self) - 1 - int(np.argmax(self.created[::-1]))

    def position_of(self, uid: int) -> int:
        """the list index a claimed task has now (the first row that carries the id), NONE if it is gone"""
        hit = np.nonzero(self.uid == np.uint64(uid))[0]
        return int(hit[0]) if len(hit) else NONE

    def oracle_tasks(self, cfgs: np.ndarray) -> np.ndarray:
        """the list as the oracle's task rows: ~0 = no allowed_topologies key; otherwise the names of the configurations
        whose bits are set (at most four: the detector masks name one) and one name no configuration has for bits at or
        above C"""
        C, T = len(cfgs), len(self)
        t = np.zeros(T, dtype=orc.task_dt)
        t["created_at"] = self.created
        t["restricted"] = self.mask != ALL
        valid = (1 << C) - 1
        low = self.mask & np.uint64(valid)
        plain = (self.mask == low) & (low != 0) & ((low & (low - np.uint64(1))) == 0)      # one configuration, nothing else
        if plain.any():
            c = np.log2(low[plain].astype(np.float64)).astype(np.int64)
            t["n_topologies"][plain] = 1
            tp = t["topologies"]
            tp[plain, 0] = cfgs["name"][c]
            t["topologies"] = tp
        for i in np.nonzero((self.mask != ALL) & ~plain)[0]:
            m = int(self.mask[i])
            names = [cfgs["name"][c] for c in range(C) if (m >> c) & 1]
            if m & ~valid:
                names.append(b"ghost-topology")
            assert len(names) <= orc.MAX_TOPO
            t["n_topologies"][i] = len(names)
            for k, nm in enumerate(names):
                t["topologies"][i][k] = nm
        return t

    def per_worker(self, cfgs: np.ndarray, cfg_of_node: np.ndarray):
        """(first applicable position, hit count) per worker from the configuration of the worker's group (-1: in no group),
        by the oracle's heartbeat sweep"""
        return orc.pair_sweep_per_worker(self.oracle_tasks(cfgs), cfgs, cfg_of_node, threads=8)

    def per_task(self, col: np.ndarray, memo: dict = None):
        """(best worker, candidate count) per task: col[w] = the compat mask of worker w if it may bid, else 0; computed once
        per distinct mask.  memo (a dict the caller keeps per column): distinct masks answered before are not swept again"""
        col = np.asarray(col, dtype=np.uint64)
        u, inv = np.unique(self.mask, return_inverse=True)
        known = memo.get("mask", np.zeros(0, dtype=np.uint64)) if memo is not None else np.zeros(0, dtype=np.uint64)
        new = np.setdiff1d(u, known)
        first = np.full(len(new), NONE, dtype=np.uint32)
        count = np.zeros(len(new), dtype=np.uint32)
        for k0 in range(0, len(new), 256):
            hits = (col[None, :] & new[k0:k0 + 256, None]) != 0
            cnt = hits.sum(axis=1)
            idx = hits.argmax(axis=1) if len(col) else np.zeros(len(cnt), dtype=np.int64)
            first[k0:k0 + 256] = np.where(cnt > 0, idx, NONE)
            count[k0:k0 + 256] = cnt
        if len(known):
            allm = np.concatenate([known, new])
            order = np.argsort(allm, kind="stable")
            allm = allm[order]
            first = np.concatenate([memo["first"], first])[order]
            count = np.concatenate([memo["count"], count])[order]
        else:
            allm = new
        if memo is not None:
            memo.update(mask=allm, first=first, count=count)
        k = np.searchsorted(allm, u)[inv.ravel()]
        return first[k], count[k]

    def task_report(self, groups, n_cfgs: int):
        """groups: [(config, n_members, task position or -1)] -> (groups_running, workers_running, groups_allowed) by position"""
        T = len(self)
        running = np.zeros(T, dtype=np.uint32)
        workers = np.zeros(T, dtype=np.uint32)
        per_cfg = np.zeros(64, dtype=np.int64)
        for cfg, n, t in groups:
            per_cfg[cfg] += 1
            if t >= 0:
                running[t] += 1
                workers[t] += n
        allowed = np.zeros(T, dtype=np.int64)
        for c in range(n_cfgs):
            if per_cfg[c]:
                allowed += ((self.mask >> np.uint64(c)) & np.uint64(1)).astype(np.int64) * per_cfg[c]
        return running, workers, allowed.astype(np.uint32)


# ------------------------------------------------------------------ the shadow of the index space

class IndexShadow:
    """[t_lo, t_cap) with its live cells and tombstones, by the rules of DESIGN 3.1:
      upload        a fresh space of task_capacity_for(n) when the old one has fewer than n + 64 cells, more than
                    8 n + 2^20, or the table changes between carrying ids and not; the rows at the top, no tombstones
      insert_front  n rows in front of t_lo; if t_lo < n the live rows move into task_capacity_for(T + n) (a regrowth)
      delete        tombstones; those in front are trimmed at once; more than T + 4,096 of them left in the range and the
                    live rows move to the top of the same capacity (a compaction)"""

    def __init__(self):
        self.t_cap = 0
        self.cells = np.zeros(0, dtype=bool)              # the cells of [t_lo, t_cap): live or tombstone
        self.regrowths = 0
        self.compactions = 0
        self.has_uid = False

    @property
    def t_lo(self) -> int:
        return self.t_cap - len(self.cells)

    @property
    def T(self) -> int:
        return int(self.cells.sum())

    @property
    def t_dead(self) -> int:
        return len(self.cells) - self.T

    def state(self) -> dict:
        return dict(t_lo=self.t_lo, t_cap=self.t_cap, T=self.T, t_dead=self.t_dead, regrowths=self.regrowths,
                    compactions=self.compactions)

    def upload(self, n: int, has_uid: bool):
        if self.t_cap < n + 64 or self.t_cap > 8 * n + (1 << 20) or has_uid != self.has_uid:
            self.t_cap = task_capacity_for(n)
        self.has_uid = has_uid
        self.cells = np.ones(n, dtype=bool)

    def insert_front(self, n: int, has_uid: bool):
        if n == 0:
            return
        if self.T == 0 and self.t_dead == 0:
            self.has_uid = has_uid
        if self.t_lo < n:
            self.t_cap = task_capacity_for(self.T + n)
            self.cells = np.ones(self.T, dtype=bool)
            self.regrowths += 1
        self.cells = np.concatenate([np.ones(n, dtype=bool), self.cells])

    def delete(self, positions):
        """positions: list positions (live rows in front) of the rows that go"""
        positions = np.asarray(positions, dtype=np.int64)
        if len(positions) == 0:
            return
        self.cells[np.nonzero(self.cells)[0][positions]] = False
        live = np.nonzero(self.cells)[0]
        self.cells = self.cells[live[0]:] if len(live) else self.cells[:0]
        if self.t_dead > self.T + DEAD_SLACK:
            self.cells = np.ones(self.T, dtype=bool)
            self.compactions += 1

    def positions_of_handles(self, handles) -> np.ndarray:
        """the list positions of the live rows in these index-space cells (for steering only: which rows a test has to
        delete to put tombstones into a given word)"""
        k = np.asarray(handles, dtype=np.int64) - self.t_lo
        assert (k >= 0).all() and (k < len(self.cells)).all() and self.cells[k].all()
        return (np.cumsum(self.cells) - 1)[k]


class Table:
    """the list and the shadow moved together, and the same calls made on any number of engines"""

    def __init__(self, engines=()):
        self.list, self.shadow, self.engines = TaskList(), IndexShadow(), list(engines)

    def upload(self, mask, created, uid=None):
        self.list.upload(mask, created, uid)
        self.shadow.upload(len(self.list), uid is not None)
        for e in self.engines:
            e.upload_tasks(mask, created, uid)

    def insert_front(self, mask, created, uid=None):
        self.list.insert_front(mask, created, uid)
        self.shadow.insert_front(len(mask), uid is not None)
        for e in self.engines:
            e.tasks_insert_front(mask, created, uid)

    def delete(self, uids) -> int:
        """-> rows that went; self.last_gone: their positions in the list before the call"""
        gone = self.last_gone = self.list.delete(uids)
        self.shadow.delete(gone)
        for e in self.engines:
            assert e.tasks_delete(uids) == len(gone)
        return len(gone)
