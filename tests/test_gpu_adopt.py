"""pm_adopt_groups / pm_group_id_state (include/pm_engine.h "Restart and switch-over"): an engine that takes over the groups
another one formed — or that a store holds — must go on exactly as the one that formed them would have: the same rows
published after its first match, the oracle's digests through the churn stream, the oracle through the soak schedule
(also with ids that never came from the id stream), the same claims from the seeded chooser, the same ticks on two
ranks, and every refusal leaving the engine as it was."""
import json
import os
import sys
import threading
import time

import numpy as np
import pytest
import torch

from oracle import oracle_ffi as orc
from protocol_amd import engine as E
from protocol_amd import host
from protocol_amd.churn import ChurnStream
from protocol_amd.dist import EngineLocal, ShardedEngine
from protocol_amd.swarm import make_swarm
from soak import GROUP_ID_SEED, Soak, engine_groups, oracle_groups, rows_of

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from make_golden_churn import CHURN_SEED, CHURN_TICKS_PINNED, CHURN_TICKS_PLANNED, events_digest, groups_digest, sha  # noqa: E402

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "churn_digests.json")))


def mix64(x):
    """pm_internal.h splitmix64_mix: the seeded chooser's hash"""
    z = (x + GOLDEN) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _row(a):
    return (a.task, a.group_slot, a.group_index, a.group_size, a.next_worker, a.group_id)


def _adopt_from(src, dst):
    _, groups, members = src.get_groups()
    dst.adopt_groups(groups, members, src.group_id_state())
    return groups, members


# ------------------------------------------------------------------ 1. round trip

def test_round_trip_of_a_cold_match():
    sw = make_swarm(61, 3000, 20000)
    a = E.Engine(group_id_seed=7)
    host.load_swarm(a, sw)
    a.enable_group_events()
    a.tick()
    a.drain_group_events()
    b = E.Engine(group_id_seed=7)
    host.load_swarm(b, sw)
    b.tick()                                                   # (a table of its own published, then the groups dropped)
    b.reset_groups()
    b.enable_group_events()
    _adopt_from(a, b)
    assert engine_groups(b) == engine_groups(a)
    assert b.group_id_state() == a.group_id_state()
    assert all(b.lookup(w).task == NONE and b.lookup(w).group_slot == NONE for w in range(sw.W))  # until the next publish
    b.match()
    assert [_row(b.lookup(w)) for w in range(sw.W)] == [_row(a.lookup(w)) for w in range(sw.W)]
    assert b.drain_group_events() == []
    # ... and the next tick after the same deaths is the same on both
    rng = np.random.default_rng(3)
    dead = rng.choice(sw.W, 400, replace=False)
    flags = host.pack_workers(sw)["flags"][dead] & ~np.uint32(E.W_HEALTHY)
    for e in (a, b):
        e.on_worker_status_many(dead, flags, np.ones(len(dead), dtype=np.uint32))
        e.tick()
    assert engine_groups(b) == engine_groups(a)
    assert b.drain_group_events() == a.drain_group_events()
    assert [_row(b.lookup(w)) for w in range(sw.W)] == [_row(a.lookup(w)) for w in range(sw.W)]
    a.close(), b.close()


# ------------------------------------------------------------------ 2. restart inside the churn stream

def _check_tick(eng, W, gold, stats, tag):
    assert stats["n_formed"] == gold["n_formed"] and stats["n_merged"] == gold["n_merged"], (tag, stats)
    groups = [(g[0], g[1], g[2]) for g in engine_groups(eng)]
    assert len(groups) == gold["n_groups"] and groups_digest(groups) == gold["groups_sha256"], f"{tag}: groups"
    assert sha(np.array([eng.lookup(w).task for w in range(W)], dtype=np.uint32)) == gold["task_sha256"], f"{tag}: tasks"
    ev = eng.drain_group_events()
    assert len(ev) == gold["n_events"] and events_digest(ev) == gold["events_sha256"], f"{tag}: life-cycle feed"


@pytest.mark.parametrize("k_restart", [0, 3, 6])
def test_restart_inside_the_churn_stream(k_restart):
    gold = GOLD["churn"]
    assert k_restart < CHURN_TICKS_PINNED
    cs = ChurnStream(CHURN_SEED, CHURN_TICKS_PLANNED)
    sw_all = cs.sw_all
    packed = host.pack_workers(sw_all)
    cfg_rows, alt_rows, req_models = host.pack_configs(sw_all.configs)
    bits = host.build_model_table(req_models, sw_all.model_names)

    def fresh():
        e = E.Engine(group_id_seed=1)
        e.set_configs(cfg_rows, alt_rows)
        e.set_model_table(bits, len(req_models), len(sw_all.model_names))
        return e

    flags = packed["flags"].copy()
    masks, created, uid = cs.masks.copy(), cs.created.copy(), cs.uid.copy()
    a = fresh()
    a.upload_workers(rows_of(packed, np.arange(cs.W0)))
    a.upload_tasks(masks, created, uid)
    a.set_enabled_mask(sw_all.enabled_mask())
    a.tick()
    b, tick_ms = None, []
    for k in range(CHURN_TICKS_PINNED):
        if k == k_restart:  # B: the tables as they stand (leavers' flags, every row in order, the current task list)
            b = fresh()
            cur = rows_of(packed, np.arange(cs.W))
            cur["flags"] = np.ascontiguousarray(flags[:cs.W])
            b.upload_workers(cur)
            b.upload_tasks(masks, created, uid)
            b.set_enabled_mask(sw_all.enabled_mask())
            b.enable_group_events()
            t0 = time.perf_counter()
            _adopt_from(a, b)
            print(f"\nadopt at tick {k}: {len(engine_groups(b))} groups over {cs.W} workers, "
                  f"{(time.perf_counter() - t0) * 1e3:.2f} ms (with get_groups)")
            a.close()
            a = None
        leave, idx_new, new_tasks = cs.step()
        flags[leave] &= ~np.uint32(E.W_HEALTHY)
        nm, nc, nu = new_tasks[:3]
        masks, created, uid = np.concatenate([nm, masks]), np.concatenate([nc, created]), np.concatenate([nu, uid])
        e = b if b is not None else a
        e.on_worker_status_many(leave, flags[leave], np.ones(len(leave), dtype=np.uint32))
        e.append_workers(rows_of(packed, idx_new))
        e.tasks_insert_front(nm, nc, nu)
        t0 = time.perf_counter()
        stats = e.tick()
        ms = (time.perf_counter() - t0) * 1e3
        tick_ms.append(ms)
        if b is not None:
            if k == k_restart:
                print(f"first tick after the adoption (full upload): {ms:.3f} ms")
            _check_tick(b, cs.W, gold["ticks"][k], stats, f"tick {k} (restart at {k_restart})")
    print(f"churn ticks (ms): {' '.join(f'{t:.3f}' for t in tick_ms)}")
    b.close()


# ------------------------------------------------------------------ 3. + 4. restart against the oracle over a long run

class IdMapped:
    """an engine seen through an id map: the oracle's ids in, the engine's ids out (and back)"""

    def __init__(self, eng, fwd):
        self.eng, self.fwd = eng, fwd
        self.back = {v: k for k, v in fwd.items()}

    def __getattr__(self, name):
        return getattr(self.eng, name)

    def f(self, gid):
        return self.fwd.get(int(gid), int(gid))

    def b(self, gid):
        return self.back.get(int(gid), int(gid))

    def get_groups(self):
        gow, groups, members = self.eng.get_groups()
        groups = groups.copy()
        groups["id"] = np.array([self.b(g) for g in groups["id"]], dtype=np.uint64)
        return gow, groups, members

    def drain_group_events(self):
        return [(k, self.b(g), c, m) for (k, g, c, m) in self.eng.drain_group_events()]

    def _back_one(self, r):
        if r is not None:
            r["id"] = self.b(r["id"])
        return r

    def get_group_by_id(self, gid):
        return self._back_one(self.eng.get_group_by_id(self.f(gid)))

    def get_group_of_worker(self, w):
        return self._back_one(self.eng.get_group_of_worker(w))

    def dissolve_group_by_id(self, gid):
        return self.eng.dissolve_group_by_id(self.f(gid))


def _order_keeping_map(live, others, rng):
    """live ids -> other u64 values, many of them short, whose "{:x}" text orders like the originals' among `live` and
    `others` (every id the oracle's stream will draw): a unique prefix of the text, then random digits or none"""
    texts = sorted({"%x" % x for x in list(live) + list(others)})
    pos = {t: i for i, t in enumerate(texts)}

    def common(a, b):
        n = 0
        while n < min(len(a), len(b)) and a[n] == b[n]:
            n += 1
        return n

    out = {}
    for x in live:
        t = "%x" % x
        i = pos[t]
        lcp = max(common(t, texts[i - 1]) if i else 0, common(t, texts[i + 1]) if i + 1 < len(texts) else 0)
        L = min(lcp + 1, len(t))
        extra = int(rng.integers(0, 16 - L + 1)) if rng.random() < 0.5 else 0
        out[x] = int(t[:L] + "".join("0123456789abcdef"[int(d)] for d in rng.integers(0, 16, extra)), 16)
    assert len(set(out.values())) == len(out)
    return out


@pytest.mark.parametrize("remap", [False, True], ids=["stream_ids", "foreign_ids"])
def test_restart_in_the_soak_against_the_oracle(remap):
    ticks, k_restart = 260, 110
    s = Soak(3, ticks)
    a = E.Engine(group_id_seed=GROUP_ID_SEED)
    s.load(a)
    n_created = 0
    adopted, adopted_solo, merges0, cov0 = set(), set(), 0, {}
    destroyed = []
    for k in range(ticks):
        if k == k_restart:
            b = E.Engine(group_id_seed=GROUP_ID_SEED)
            host.load_swarm(b, s.take_sw(s.W))
            b.upload_workers(rows_of(s.packed, np.arange(s.W)))
            b.upload_tasks(s.masks, s.created, s.uid)
            b.set_enabled_mask(s.enabled_mask & ~(1 << s.disabled[0]) if s.disabled else s.enabled_mask)
            b.enable_group_events()
            _, groups, members = a.get_groups()
            groups = groups.copy()
            assert a.group_id_state() == (GROUP_ID_SEED + n_created * GOLDEN) & M64
            fwd = {}
            if remap:
                stream = orc.splitmix64_stream(GROUP_ID_SEED, n_created + 40000)
                fwd = _order_keeping_map([int(g) for g in groups["id"]], [int(x) for x in stream],
                                         np.random.default_rng(9))
                assert sum(len("%x" % v) <= 8 for v in fwd.values()) >= len(fwd) // 4
                groups["id"] = np.array([fwd[int(g)] for g in groups["id"]], dtype=np.uint64)
            b.adopt_groups(groups, members, a.group_id_state())
            a.close()
            s.engines = [IdMapped(b, fwd)]
            adopted = {int(g) for g in groups["id"]}
            adopted_solo = {int(g["id"]) for g in groups if g["n_members"] == 1}
            merges0, cov0 = s.cov["merges"], dict(s.cov)
        e = s.engines[0]
        s.interval(k)
        stats = e.tick()
        tasks, want, events = s.oracle_tick()
        n_created += sum(1 for ev in events if ev[0] == E.GROUP_CREATED)
        if k >= k_restart:
            destroyed += [e.f(ev[1]) for ev in events if ev[0] == E.GROUP_DESTROYED]
        s.compare(e, k, tasks, want, events, stats)
        if k >= k_restart:
            assert b.group_id_state() == (GROUP_ID_SEED + n_created * GOLDEN) & M64, f"tick {k}: id stream"
    gone = adopted & set(destroyed)
    print(f"\nadopted {len(adopted)} groups ({len(adopted_solo)} solo), {len(gone)} of them dissolved after the restart; "
          f"merges after it {s.cov['merges'] - merges0}; coverage {s.cov}")
    assert s.cov["merges"] > merges0 and adopted_solo & set(destroyed), "no merge of adopted solo groups"
    assert len(gone) >= 20
    for key in ("deaths", "claimed_deletes", "dissolve_hits"):
        assert s.cov[key] > cov0[key], key
    b.close()


def test_seeded_chooser_over_foreign_ids():
    """taskless adopted groups under PM_CHOOSE_SEEDED claim the rank-th applicable task, rank = mix64(seed ^ id) % n
    (the oracle's chooser, pm_oracle.c) — for ids that are not the engine's own"""
    sw = make_swarm(62, 1500, 6000)
    a = E.Engine(group_id_seed=11)
    host.load_swarm(a, sw)
    a.tick()
    _, groups, members = a.get_groups()
    rng = np.random.default_rng(4)
    groups = groups.copy()
    ids = set()
    while len(ids) < len(groups):
        ids.add(int(rng.integers(1, 1 << int(rng.integers(4, 64)), dtype=np.uint64)))
    groups["id"] = np.array(sorted(ids), dtype=np.uint64)
    groups["task"] = NONE
    seed = 0xC0FFEE
    b = E.Engine(group_id_seed=11, chooser=E.CHOOSE_SEEDED, chooser_seed=seed)
    host.load_swarm(b, sw)
    b.adopt_groups(groups, members, 12345)
    task, count = b.match()
    masks = sw.task_masks()
    claimed = 0
    for g in groups:
        cfg, w0 = int(g["config"]), int(members[int(g["member_begin"])])
        app = np.nonzero((masks >> np.uint64(cfg)) & np.uint64(1))[0]   # (filter_tasks: the group's configuration, enabled or not)
        assert int(count[w0]) == len(app), (g, len(app))
        want = NONE if len(app) == 0 else int(app[mix64(seed ^ int(g["id"])) % len(app)])
        for j in range(int(g["n_members"])):
            assert int(task[int(members[int(g["member_begin"]) + j])]) == want
        claimed += want != NONE
    assert claimed >= len(groups) // 2
    a.close(), b.close()


# ------------------------------------------------------------------ 5. two in-process ranks

def test_two_ranks_adopt_the_same_list():
    from test_gpu_dist import _InProcExchanger, _InProcGroup
    sw = make_swarm(63, 2000, 12000)
    a = E.Engine(group_id_seed=5)
    host.load_swarm(a, sw)
    a.tick()
    _, groups, members = a.get_groups()
    state = a.group_id_state()
    rng = np.random.default_rng(8)
    dead = rng.choice(sw.W, 600, replace=False)
    flags = host.pack_workers(sw)["flags"][dead] & ~np.uint32(E.W_HEALTHY)
    one = E.Engine(group_id_seed=5)
    host.load_swarm(one, sw)
    one.adopt_groups(groups, members, state)
    one.on_worker_status_many(dead, flags, np.ones(len(dead), dtype=np.uint32))
    one.tick()
    want_groups, want_rows = engine_groups(one), [_row(one.lookup(w)) for w in range(sw.W)]
    world, grp, errs, got = 2, _InProcGroup(2), [], {}

    def rank_main(r):
        try:
            eng = E.Engine(group_id_seed=5)
            host.load_swarm(eng, sw)
            eng.adopt_groups(groups, members, state)
            eng.on_worker_status_many(dead, flags, np.ones(len(dead), dtype=np.uint32))
            se = ShardedEngine(EngineLocal(eng, torch.device("cuda", 0)), sw.address, exchanger=_InProcExchanger(grp, r))
            se.tick()
            got[r] = (engine_groups(eng), [_row(eng.lookup(w)) for w in range(sw.W)])
            eng.close()
        except BaseException as ex:  # a dead rank must not leave the other at the barrier
            errs.append((r, repr(ex)))
            grp.barrier.abort()

    th = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for r in range(world):
        assert got[r][0] == want_groups, r
        assert got[r][1] == want_rows, r
    a.close(), one.close()


# ------------------------------------------------------------------ 6. refusals

def _rows_after_cold(sw):
    e = E.Engine(group_id_seed=21)
    host.load_swarm(e, sw)
    e.tick()
    out = (engine_groups(e), [_row(e.lookup(w)) for w in range(sw.W)])
    e.close()
    return out


def test_refusals_leave_the_engine_as_it_was():
    sw = make_swarm(64, 800, 4000)
    want = _rows_after_cold(sw)
    a = E.Engine(group_id_seed=3)
    host.load_swarm(a, sw)
    a.tick()
    _, groups, members = a.get_groups()
    T, W, C = sw.T, sw.W, len(sw.configs)
    cfg_rows = host.pack_configs(sw.configs)[0]
    big = next(i for i, g in enumerate(groups) if g["n_members"] >= 2)
    solo_cfg = int(groups[big]["config"])

    def field(i, name, v):
        def fn(g, m):
            g[name][i] = v
        return fn

    def member(k_of, v_of):
        def fn(g, m):
            m[k_of(g)] = v_of(g, m)
        return fn

    def doctored(fn):
        g, m = groups.copy(), members.copy()
        fn(g, m)
        return g, m

    b0 = int(groups[big]["member_begin"])
    cases = {
        "config >= n_cfgs": doctored(field(0, "config", C)),
        "n_members 0": doctored(field(big, "n_members", 0)),
        "n_members > max": doctored(field(big, "n_members", int(cfg_rows[solo_cfg]["max_group_size"]) + 1)),
        "member_begin past the end": doctored(field(len(groups) - 1, "member_begin", len(members))),
        "member >= W": doctored(member(lambda g: b0, lambda g, m: W)),
        "worker twice": doctored(member(lambda g: b0 + 1, lambda g, m: m[b0])),
        "worker in two groups": doctored(member(lambda g: int(g[1]["member_begin"]), lambda g, m: m[int(g[0]["member_begin"])])),
        "duplicate id": doctored(field(len(groups) - 1, "id", groups[0]["id"])),
        "task >= T": doctored(field(0, "task", T)),
    }
    for name, (g, m) in cases.items():
        b = E.Engine(group_id_seed=21)
        host.load_swarm(b, sw)
        s0 = b.group_id_state()
        with pytest.raises(E.EngineError) as ex:
            b.adopt_groups(g, m, 999)
        assert ex.value.code == E.PM_EINVAL and "group " in str(ex.value), (name, ex.value)
        assert b.get_groups()[1].size == 0 and b.group_id_state() == s0, name
        b.tick()                                               # the next cold tick is a fresh engine's
        assert (engine_groups(b), [_row(b.lookup(w)) for w in range(W)]) == want, name
        b.close()
    # PM_ESTATE: groups standing, no workers / configs yet, a group naming a task before the task table
    b = E.Engine(group_id_seed=21)
    host.load_swarm(b, sw)
    b.tick()
    with pytest.raises(E.EngineError) as ex:
        b.adopt_groups(groups, members, 1)
    assert ex.value.code == E.PM_ESTATE
    b.close()
    b = E.Engine(group_id_seed=21)
    with pytest.raises(E.EngineError) as ex:
        b.adopt_groups(groups, members, 1)
    assert ex.value.code == E.PM_ESTATE
    cfg, alt, req = host.pack_configs(sw.configs)
    b.set_configs(cfg, alt)
    b.set_model_table(host.build_model_table(req, sw.model_names), len(req), len(sw.model_names))
    b.upload_workers(host.pack_workers(sw))
    with_task = groups.copy()
    with_task["task"][0] = 0
    with pytest.raises(E.EngineError) as ex:
        b.adopt_groups(with_task, members, 1)
    assert ex.value.code == E.PM_ESTATE
    b.close()
    a.close()


def test_adoption_time():
    """wall time of pm_adopt_groups at BASELINE configs[2] (100k workers, 1M tasks), next to a cold match of the same
    swarm and to the first tick after the adoption (a full upload of the group list)"""
    from protocol_amd.swarm import baseline_config
    size = "configs[2]"
    sw = baseline_config(2, seed=1)
    a = E.Engine(group_id_seed=1)
    host.load_swarm(a, sw)
    t0 = time.perf_counter()
    a.tick()
    cold = (time.perf_counter() - t0) * 1e3
    _, groups, members = a.get_groups()
    state = a.group_id_state()
    a.close()
    b = E.Engine(group_id_seed=1)
    host.load_swarm(b, sw)
    t0 = time.perf_counter()
    b.adopt_groups(groups, members, state)
    adopt = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    b.tick()
    first = (time.perf_counter() - t0) * 1e3
    print(f"\n{size}: {len(groups)} groups over {sw.W} workers: adopt {adopt:.2f} ms, first tick after it "
          f"{first:.2f} ms, cold match {cold:.2f} ms")
    assert b.drain_group_events() == [] and len(engine_groups(b)) >= len(groups)
    b.close()
