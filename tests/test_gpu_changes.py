"""The assignment change feed (include/pm_engine.h "assignment change feed": pm_enable_assignment_changes /
pm_drain_assignment_changes; kernels in protocol_amd/csrc/pm_changes.inc) against the model of tests/changes_model.py.

The expected list never comes from the code under test: after every publish each worker's published row is read with
Engine.lookup (the seqlock path), its task position is turned into the task's uid with the test's own task list, and the
successive tables go to the model.

Chunk sizes of the kernels, with a W below, at and above each: 64 rows a wave (= one bitmap word: 63, 64, 65), 256 rows a
workgroup of assign_diff_kernel and of change_expand_kernel (4 words: 255, 256, 257), 4 words = 256 rows a thread of
change_scan_kernel per pass (the same three), 1024 words = 65,536 rows a pass of its one workgroup (65535, 65536, 65537)."""
import ctypes as C

import numpy as np
import pytest

from protocol_amd import engine as E
from protocol_amd import host
from protocol_amd.churn import ChurnStream

import changes_model as M

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
ON = E.W_HEALTHY | E.W_HAS_P2P
PM_ESTATE, PM_ERANGE = -4, -5


def cols(n, flags=ON):
    z = np.zeros(n, dtype=np.uint32)
    return dict(flags=np.full(n, flags, dtype=np.uint32), gpu_count=z, gpu_mem_mb=z, gpu_model_class=z, cpu_cores=z, ram_mb=z,
                storage_gb=z, price=z, lat=np.zeros(n), lon=np.zeros(n))


def table(eng, W, uids):
    """the published rows as the model's table"""
    out = []
    for w in range(W):
        a = eng.lookup(w)
        out.append(M.row_of(a.group_slot, a.group_id, a.group_index, a.group_size, a.next_worker,
                            None if a.task == NONE else uids[a.task]))
    return out


def drained(eng):
    workers, what, resync = eng.drain_assignment_changes()
    return list(zip(workers.tolist(), what.tolist())), resync


class Rig:
    """an engine with requirement-free configurations [(min, max)], W workers, tasks [(mask, uid)] newest first, the feed on,
    and `groups` [(config, [members])] installed with pm_adopt_groups; the model follows every publish"""

    def __init__(self, W, sizes=((1, 1),), tasks=((1, 101), (1, 102)), groups=None, feed=True):
        self.eng = eng = E.Engine(group_id_seed=5)
        cfg_rows, alt_rows, _ = host.pack_configs([("c%d" % i, mn, mx, None) for i, (mn, mx) in enumerate(sizes)])
        eng.set_configs(cfg_rows, alt_rows)
        self.W = W
        self.flags = np.full(W, ON, dtype=np.uint32)
        eng.upload_workers(cols(W))
        self.masks = [m for m, _ in tasks]
        self.uids = [u for _, u in tasks]
        self.t_next = 1000
        self.upload_tasks()
        if groups is None:
            groups = [(0, [w]) for w in range(W)]
        self.adopt(groups)
        self.feed = M.Feed()
        if feed:
            eng.enable_assignment_changes()

    def upload_tasks(self):
        n = len(self.uids)
        self.eng.upload_tasks(np.array(self.masks, dtype=np.uint64), np.arange(n, 0, -1, dtype=np.int64) + self.t_next,
                              np.array(self.uids, dtype=np.uint64))
        self.t_next += n + 1

    def insert_front(self, mask, uids, republish=False):
        n = len(uids)
        self.eng.tasks_insert_front(np.full(n, mask, dtype=np.uint64), np.arange(n, 0, -1, dtype=np.int64) + self.t_next,
                                    np.array(uids, dtype=np.uint64), republish=republish)
        self.t_next += n + 1
        self.masks = [mask] * n + self.masks
        self.uids = list(uids) + self.uids

    def adopt(self, groups):
        g = np.zeros(len(groups), dtype=E.group_dt)
        members = []
        for i, (c, ms) in enumerate(groups):
            g[i] = (0x7000 + i, c, len(ms), len(members), NONE)
            members += ms
        self.eng.adopt_groups(g, np.array(members, dtype=np.uint32), 77)

    def status(self, workers, healthy):
        workers = np.array(sorted(workers), dtype=np.uint32)
        if not len(workers):
            return
        self.flags[workers] = ON if healthy else ON & ~E.W_HEALTHY
        self.eng.on_worker_status_many(workers, self.flags[workers], np.full(len(workers), 0 if healthy else 1, dtype=np.uint32))

    def append(self, n, healthy=True):
        f = ON if healthy else ON & ~E.W_HEALTHY
        self.eng.append_workers(cols(n, f))
        self.flags = np.concatenate([self.flags, np.full(n, f, dtype=np.uint32)])
        self.W += n

    def published(self):
        """a publish happened: the model sees the table"""
        self.feed.publish(table(self.eng, self.W, self.uids))

    def tick(self):
        self.eng.tick()
        self.published()

    def check_drain(self, tag=""):
        got, resync = drained(self.eng)
        want, want_resync = self.feed.drain()
        print(f"{tag}: W {self.W}, {len(got)} rows drained, {len(want)} expected, resync {resync}/{want_resync}")
        assert resync == want_resync, tag
        assert got == want, (tag, got[:8], want[:8])
        return got

    def close(self):
        self.eng.close()


# ------------------------------------------------------------------ 1. exact patterns

def _patterns(W):
    rng = np.random.default_rng(W)
    cand = {
        "empty": [], "all": range(W), "row 0": [0], "row W-1": [W - 1], "every 64th": range(0, W, 64), "63 and 64": [63, 64],
        "one whole word": range(64, 128) if W >= 128 else range(min(W, 64)),
        "1 %": np.flatnonzero(rng.random(W) < 0.01), "50 %": np.flatnonzero(rng.random(W) < 0.5),
    }
    return [(k, sorted({int(w) for w in v if w < W})) for k, v in cand.items()]


@pytest.mark.parametrize("W", [1, 2, 63, 64, 65, 255, 256, 257, 1025, 4097])
def test_exact_patterns(W):
    """every worker its own group; kill exactly S, tick: the list is S, ascending, GROUP | RING | TASK each; then S comes back
    Healthy and is listed again, with the group the carve gave it"""
    r = Rig(W)
    r.tick()
    assert r.check_drain("resync") == [(w, M.ALL) for w in range(W)]
    for name, S in _patterns(W):
        r.status(S, healthy=False)
        r.tick()
        got = r.check_drain(name)
        assert got == [(w, M.ALL) for w in S], name            # (each held a task: all three bits)
        assert drained(r.eng) == ([], False), name             # a second drain is empty
        r.status(S, healthy=True)
        r.tick()
        got = r.check_drain(name + ", back")
        assert [w for w, _ in got] == S and all(b & M.GROUP for _, b in got), name
    r.close()


@pytest.mark.parametrize("W", [65535, 65536, 65537])
def test_exact_patterns_around_a_pass_of_the_scanning_workgroup(W):
    r = Rig(W)
    r.tick()
    assert r.check_drain("resync") == [(w, M.ALL) for w in range(W)]
    rng = np.random.default_rng(W)
    dead = set()
    for name, S in (("around 65536", [w for w in (65471, 65472, 65534, 65535, 65536) if w < W]),
                    ("every 64th", list(range(0, W, 64))),
                    ("1 % and the last row", sorted(set(np.flatnonzero(rng.random(W) < 0.01).tolist()) | {W - 1}))):
        fresh = [w for w in S if w not in dead]                # (a row that died under an earlier pattern stays as it is)
        dead.update(S)
        r.status(S, healthy=False)
        r.tick()
        assert r.check_drain(name) == [(w, M.ALL) for w in fresh] and len(fresh) > len(S) // 2, name
    assert drained(r.eng) == ([], False)
    r.close()


# ------------------------------------------------------------------ 2. each bit alone

def test_task_bit_alone():
    """two configurations, tasks for configuration 0 only: the groups of configuration 1 stand idle.  One task for
    configuration 1 goes in front: its groups' members are listed with TASK alone; every published position of the others
    moved by one and none of them is listed"""
    W = 130
    r = Rig(W, sizes=((1, 1), (1, 1)), tasks=((1, 101), (1, 102)), groups=[(w % 2, [w]) for w in range(W)])
    r.tick()
    r.check_drain("resync")
    before = [r.eng.lookup(w).task for w in range(W)]
    assert all((t == NONE) == (w % 2 == 1) for w, t in enumerate(before))
    r.insert_front(2, [201])
    r.tick()
    got = r.check_drain("task")
    assert got == [(w, M.TASK) for w in range(1, W, 2)]
    after = [r.eng.lookup(w).task for w in range(W)]
    assert all(after[w] == before[w] + 1 for w in range(0, W, 2)) and all(after[w] == 0 for w in range(1, W, 2))
    # the republish of pm_tasks_insert_front_ex is a publish too: nothing new to claim, nothing listed, positions move again
    r.insert_front(2, [202], republish=True)
    r.published()
    assert r.check_drain("republish") == []
    r.close()


def test_ring_bit_alone():
    """groups of 1, 2, 3 and 5 members; the address ranks are reversed: every member of the larger groups is listed with RING
    alone (the middle one of three keeps its index, not its next), the single one is not listed"""
    groups = [(0, [0]), (1, [1, 2]), (2, [3, 4, 5]), (3, [6, 7, 8, 9, 10])]
    W = 11
    r = Rig(W, sizes=((1, 1), (2, 2), (3, 3), (5, 5)), tasks=((15, 101),), groups=groups)
    r.tick()
    r.check_drain("resync")
    mid = r.eng.lookup(4)
    assert (mid.group_index, mid.group_size, mid.next_worker) == (1, 3, 5)
    r.eng.set_addr_ranks(np.arange(W - 1, -1, -1, dtype=np.uint32))
    r.tick()
    got = r.check_drain("ring")
    assert got == [(w, M.RING) for w in range(1, W)]
    mid = r.eng.lookup(4)
    assert (mid.group_index, mid.group_size, mid.next_worker) == (1, 3, 3)
    r.close()


def test_group_bit():
    """a group dissolved by id whose members stay Healthy: the next tick forms them again under a new id"""
    groups = [(0, [0, 1]), (0, [2, 3]), (0, [4, 5])]
    r = Rig(6, sizes=((2, 2),), tasks=((1, 101),), groups=groups)
    r.tick()
    r.check_drain("resync")
    old = r.eng.lookup(2).group_id
    assert r.eng.dissolve_group_by_id(old)
    r.tick()
    got = r.check_drain("group")
    assert [w for w, _ in got] == [2, 3] and all(b & M.GROUP for _, b in got)
    assert r.eng.lookup(2).group_id not in (0, old) and r.eng.lookup(2).group_id == r.eng.lookup(3).group_id
    r.close()


# ------------------------------------------------------------------ 3. accumulation and the drain protocol

def test_accumulation_and_the_drain_protocol():
    W = 300
    r = Rig(W)
    L = E.lib()
    n, flags = C.c_uint32(7), C.c_uint32(7)
    r.tick()                                                   # enable, tick: all W rows and RESYNC — asked for one too small first
    rows = np.zeros(W, dtype=E.change_row_dt)
    assert L.pm_drain_assignment_changes(r.eng._h, rows.ctypes.data, W - 1, C.byref(n), C.byref(flags)) == PM_ERANGE
    assert (n.value, flags.value) == (W, E.CHANGES_RESYNC)
    assert L.pm_drain_assignment_changes(r.eng._h, None, W, C.byref(n), C.byref(flags)) == PM_ERANGE
    assert (n.value, flags.value) == (W, E.CHANGES_RESYNC)
    assert r.check_drain("resync, nothing lost") == [(w, M.ALL) for w in range(W)]
    # three ticks, different kills, one drain: the union, bits OR-ed
    r.status([5, 64, 299], healthy=False)
    r.tick()
    r.status([5], healthy=True)
    r.status([6, 128], healthy=False)
    r.tick()
    r.status([200], healthy=False)
    r.tick()
    n_want = len([b for b in r.feed.pending if b])
    assert L.pm_drain_assignment_changes(r.eng._h, rows.ctypes.data, n_want - 1, C.byref(n), C.byref(flags)) == PM_ERANGE
    assert (n.value, flags.value) == (n_want, 0)
    got = r.check_drain("three ticks")
    assert [w for w, _ in got] == [5, 6, 64, 128, 200, 299]
    assert drained(r.eng) == ([], False)
    # off clears and refuses; on again resyncs again
    r.status([7], healthy=False)
    r.tick()
    r.eng.enable_assignment_changes(False)
    with pytest.raises(E.EngineError) as ex:
        r.eng.drain_assignment_changes()
    assert ex.value.code == PM_ESTATE
    r.eng.tick()
    r.eng.enable_assignment_changes(True)
    r.feed = M.Feed()
    assert drained(r.eng) == ([], False)                       # (nothing until the next publish)
    r.tick()
    assert r.check_drain("on again") == [(w, M.ALL) for w in range(W)]
    r.close()


# ------------------------------------------------------------------ 4. growth

def test_growth_across_bitmap_words_and_past_the_buffers_capacity():
    """W crosses a bitmap word between two publishes without a drain in between (60 -> 70, 250 -> 260), and once the table
    outgrows the feed's buffers with marks pending (they were sized for 60 rows: 60 + 60 / 4 + 64 = 139; 250 is past that).
    One drain at the end: the model's union.  Appended rows that got no group (not Healthy) are not listed."""
    r = Rig(60)
    r.tick()
    r.check_drain("resync")
    r.status([3, 59], healthy=False)
    r.tick()
    r.append(6)
    r.append(4, healthy=False)
    r.tick()                                                   # W = 70
    r.append(180)
    r.status([64, 69, 100], healthy=False)
    r.tick()                                                   # W = 250: past the capacity, marks pending
    r.append(5, healthy=False)
    r.append(5)
    r.tick()                                                   # W = 260
    got = dict(r.check_drain("growth"))
    # (100 died before the tick that would have grouped it: never in a group, never listed)
    assert {3, 59, 60, 64, 65, 70, 249, 255, 259} <= set(got) and not {66, 67, 68, 69, 100, 250, 254} & set(got)
    r.status([259], healthy=False)
    r.tick()
    assert r.check_drain("after") == [(259, M.ALL)]
    r.close()


# ------------------------------------------------------------------ 5, 6. churn against the model

class Churn:
    def __init__(self):
        self.cs = cs = ChurnStream(1, 6, W0=3000, n_churn=30, n_new=50, T0=200)
        sw = cs.sw_all
        self.packed = host.pack_workers(sw)
        self.eng = eng = E.Engine(group_id_seed=1)
        cfg_rows, alt_rows, req_models = host.pack_configs(sw.configs)
        eng.set_configs(cfg_rows, alt_rows)
        eng.set_model_table(host.build_model_table(req_models, sw.model_names), len(req_models), len(sw.model_names))
        eng.upload_workers(self.rows(np.arange(cs.W0)))
        eng.upload_tasks(cs.masks, cs.created, cs.uid)
        eng.set_enabled_mask(sw.enabled_mask())
        self.uids = [int(u) for u in cs.uid]
        self.flags = self.packed["flags"].astype(np.int64)
        self.feed = M.Feed()

    def rows(self, idx):
        return {k: np.ascontiguousarray(v[idx]) for k, v in self.packed.items()}

    def step(self):
        leave, idx_new, new_tasks = self.cs.step()
        self.eng.on_worker_status_many(leave, self.flags[leave] & ~E.W_HEALTHY, np.ones(len(leave), dtype=np.uint32))
        self.eng.append_workers(self.rows(idx_new))
        self.eng.tasks_insert_front(*new_tasks[:3])
        self.uids = [int(u) for u in new_tasks[2]] + self.uids

    def published(self):
        self.feed.publish(table(self.eng, self.cs.W, self.uids))


def test_churn_stream_against_the_model():
    c = Churn()
    c.eng.enable_assignment_changes()
    c.eng.tick()
    c.published()
    assert drained(c.eng) == c.feed.drain()
    seen = 0
    for k in range(6):
        c.step()
        c.eng.tick()
        c.published()
        got, resync = drained(c.eng)
        want, _ = c.feed.drain()
        print(f"tick {k}: W {c.cs.W}, {len(got)} rows changed")
        assert not resync and got == want, k
        assert 0 < len(got) < c.cs.W // 4, k
        for _, b in got:
            seen |= b
    assert seen == M.ALL
    c.eng.close()


def test_an_abandoned_match_leaves_no_trace():
    """the same churn for three ticks with debug_stream_abort_after(5): a streaming carve that gives up has its queued match
    abandoned, and the batch pipeline publishes — the lists are the model's still, no row twice.  The cold match gives up for
    certain (asserted).  The hook counts steps of the validator's chain only: a churn tick of this small stream carves its
    handful of groups in registers and need not reach it (the counter is printed) — the test below abandons a match at a tick
    that is no resync."""
    c = Churn()
    c.eng.enable_assignment_changes()
    c.eng.debug_stream_abort_after(5)
    c.eng.tick()
    assert c.eng.debug_carve_counters()["stream_aborts"] == 1
    c.published()
    assert drained(c.eng) == c.feed.drain()
    for k in range(3):
        c.step()
        stats = c.eng.tick()
        aborts = c.eng.debug_carve_counters()["stream_aborts"]
        print(f"tick {k}: {stats['n_formed']} groups formed, {stats['carve_steps']} steps, launches given up: {aborts}")
        c.published()
        got, resync = drained(c.eng)
        want, _ = c.feed.drain()
        assert not resync and got == want and len({w for w, _ in got}) == len(got) > 0, k
    c.eng.close()


def test_a_match_abandoned_for_the_merge_pass_leaves_no_trace():
    """pm_tick queues the match behind the streaming carve when the tick before it left fewer than two single-node groups, and
    abandons it when the carve then leaves two or more (the merge pass has to run first).  One standing group, everybody else
    not Healthy: that tick leaves one.  Then everybody comes back: the carve makes 129 single-node groups, the queued match is
    abandoned, the general path publishes — exactly the rows that came back are listed, once."""
    W = 130
    r = Rig(W, groups=[(0, [0])])
    r.status(range(1, W), healthy=False)
    r.tick()
    r.check_drain("resync")
    r.tick()
    assert r.check_drain("nothing happened") == []
    r.status(range(1, W), healthy=True)
    stats = r.eng.tick()
    assert stats["n_formed"] == W - 1
    r.published()
    assert r.check_drain("abandoned for the merge pass") == [(w, M.ALL) for w in range(1, W)]
    assert drained(r.eng) == ([], False)
    r.close()


# ------------------------------------------------------------------ 7. resync events

@pytest.mark.parametrize("event", ["upload_tasks", "reset_groups", "upload_workers", "regrowth"])
def test_resync_events(event):
    W = 200
    r = Rig(W, tasks=((1, 101), (1, 102), (1, 103)))
    r.tick()
    r.check_drain("first")
    r.status([9], healthy=False)
    r.tick()
    assert r.check_drain("exact before") == [(9, M.ALL)]
    if event == "upload_tasks":
        r.uids, r.masks = [301, 102, 101], [1, 1, 1]
        r.upload_tasks()
    elif event == "reset_groups":
        r.eng.reset_groups()
    elif event == "upload_workers":
        r.W = 150
        r.flags = np.full(r.W, ON, dtype=np.uint32)
        r.eng.upload_workers(cols(r.W))
    else:
        before = r.eng.debug_task_space()["regrowths"]
        r.insert_front(1, list(range(10**6, 10**6 + 70000)))
        assert r.eng.debug_task_space()["regrowths"] == before + 1
    r.feed.resync()
    r.tick()
    assert r.check_drain(event) == [(w, M.ALL) for w in range(r.W)]   # (check_drain compares the RESYNC flag too)
    r.status([11, 64], healthy=False)
    r.tick()
    assert r.check_drain("exact after") == [(11, M.ALL), (64, M.ALL)]
    r.close()


def test_upload_workers_keeping_the_groups_is_no_resync():
    W = 100
    r = Rig(W)
    r.tick()
    r.check_drain("first")
    r.status([4], healthy=False)
    r.flags = np.concatenate([r.flags, np.full(10, ON, dtype=np.uint32)])
    r.W = W + 10
    c = cols(r.W)
    c["flags"] = r.flags.copy()
    r.eng.upload_workers(c, keep_groups=True)
    r.tick()
    got = r.check_drain("keep_groups")
    assert [w for w, _ in got] == [4] + list(range(W, W + 10))
    r.close()


# ------------------------------------------------------------------ 8, 9. tick_many; multi-GPU engines

def test_tick_many_with_the_feed_on_in_one_engine_only():
    a, b = Rig(130), Rig(130, feed=False)
    E.tick_many([a.eng, b.eng])
    a.published()
    a.check_drain("resync")
    for r in (a, b):
        r.status([0, 64, 129], healthy=False)
    E.tick_many([a.eng, b.eng])
    a.published()
    assert a.check_drain("tick_many") == [(0, M.ALL), (64, M.ALL), (129, M.ALL)]
    with pytest.raises(E.EngineError) as ex:
        b.eng.drain_assignment_changes()
    assert ex.value.code == PM_ESTATE
    assert [b.eng.lookup(w).group_id for w in range(130)] == [a.eng.lookup(w).group_id for w in range(130)]
    a.close(), b.close()


def test_multi_gpu_engines_are_refused():
    r = Rig(8, feed=False)
    shard = np.arange(8, dtype=np.uint8) % 2
    r.eng.dist_configure(0, 2, shard)
    with pytest.raises(E.EngineError) as ex:
        r.eng.enable_assignment_changes()
    assert ex.value.code == PM_ESTATE
    r.eng.dist_configure(0, 1)
    r.eng.enable_assignment_changes()
    with pytest.raises(E.EngineError) as ex:
        r.eng.dist_configure(0, 2, shard)
    assert ex.value.code == PM_ESTATE
    r.tick()                                                   # (still a one-GPU engine with the feed on)
    assert r.check_drain("resync") == [(w, M.ALL) for w in range(8)]
    r.close()
