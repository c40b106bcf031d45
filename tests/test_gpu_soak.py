"""The engine against the oracle for a long run: 1,000 ticks (PM_SOAK_TICKS) of the mixed schedule in tests/soak.py
(PM_SOAK_SEED), with everything compared after every tick — groups in creation order, the event feed, every worker's
task, the rows of sampled workers — and the incremental state bounded: task tombstones inside the swept range, the
task index space's capacity, the group list's tombstones, retired snapshot buffers.  The longest checked run before
this was 8 ticks: task-space regrowth and compaction, retired buffers and the group id stream live beyond that.

Also the stepwise (multi-GPU) tick driven phase by phase with reads in the middle of it, and the schedule on two
in-process ranks."""
import statistics
import threading
import time

import numpy as np
import pytest
import torch

from oracle import oracle_ffi as orc
from protocol_amd import engine as E
from protocol_amd import host
from protocol_amd.dist import EngineLocal, ShardedEngine
from protocol_amd.swarm import make_swarm
from soak import GROUP_ID_SEED, Soak, engine_groups, env_int, oracle_groups
from test_gpu_dist import _InProcExchanger, _InProcGroup

pytestmark = pytest.mark.gpu


def test_soak_against_the_oracle():
    ticks, seed = env_int("PM_SOAK_TICKS", 1000), env_int("PM_SOAK_SEED", 1)
    s = Soak(seed, ticks)
    eng = E.Engine(group_id_seed=GROUP_ID_SEED)
    s.load(eng)
    t_start = time.perf_counter()
    tick_ms, deltas = [], [0, 0]
    buffers0 = eng.debug_task_space()["retired_buffers"]
    for k in range(ticks):
        s.interval(k)
        d0 = eng.debug_delta_pushes()
        t0 = time.perf_counter()
        stats = eng.tick()
        tick_ms.append((time.perf_counter() - t0) * 1e3)
        deltas[eng.debug_delta_pushes() > d0] += 1
        s.check_bounds(eng, k)
        tasks, want, events = s.oracle_tick()
        s.compare(eng, k, tasks, want, events, stats)
        s.check_bounds(eng, k)                                # (the reads compact the group list: still bounded)
    wall = time.perf_counter() - t_start
    ts = eng.debug_task_space()
    c = s.cov
    first = statistics.median(tick_ms[100:200]) if ticks >= 200 else float("nan")
    print(f"\nsoak: {ticks} ticks, seed {seed}, {wall:.1f} s; median tick {first:.3f} ms (ticks 100-200), "
          f"{statistics.median(tick_ms[-100:]):.3f} ms (last 100); ticks with / without a delta push {deltas[1]} / "
          f"{deltas[0]}; task space {ts}; coverage {c}")
    if ticks >= 1000:                                          # (what the default schedule is built to reach)
        assert c["min_groups"] >= 400, c
        assert deltas[0] >= 50 and deltas[1] >= 50, deltas
        assert c.get("regrowths_claimed", 0) >= 1, (c, ts)
        assert c.get("compactions_claimed", 0) >= 2, (c, ts)
        assert ts["retired_buffers"] > buffers0, ts
        assert c["merges"] >= 20, c
    eng.close()


def _read_all(eng, ids, workers):
    return ([eng.get_group_by_id(g) for g in ids], [eng.get_group_of_worker(w) for w in workers], engine_groups(eng))


def test_reads_inside_a_stepwise_tick_leave_the_tick_alone():
    """pm_get_group_by_id / pm_get_group_of_worker / pm_get_groups between pm_dist_tick_begin and pm_dist_tick_end (an API
    route while tick_dist holds only a shared lock): deaths in front of the tick leave tombstones in the group list; the
    reads must not compact the list under the carve, whose new groups are numbered behind the device's slots.  In front
    of the merge pass they answer with the list as it stood before the tick, and the tick's groups and tasks are the
    oracle's."""
    rng = np.random.default_rng(5)
    sw = make_swarm(17, 2000, 4000)
    late = rng.random(sw.W) < 0.2                              # rows that turn healthy in front of the second tick
    status0 = sw.status.copy()
    sw.status = np.where(late, orc.ST_DISCOVERED, sw.status).astype(np.uint8)
    nodes, cfgs, tasks, enabled = orc.from_swarm(sw)
    st = orc.State(nodes, cfgs, enabled=enabled, tasks=tasks, reference_shaped=False, group_id_seed=GROUP_ID_SEED)
    eng = E.Engine(group_id_seed=GROUP_ID_SEED)
    host.load_swarm(eng, sw)
    eng.dist_configure(0, 1, np.zeros(sw.W, dtype=np.uint8))
    flags = host.worker_flags(sw).astype(np.int64)
    phases = (eng.dist_tick_begin, eng.dist_carve_wait, eng.dist_match_begin, eng.dist_tick_end)
    for p in phases:
        p()
    st.try_form_new_groups()
    st.try_merge_solo_groups()
    assert [st.get_task_for_node(w) for w in range(sw.W)] == \
        [(-1 if eng.lookup(w).task == E.PM_NONE else eng.lookup(w).task) for w in range(sw.W)]
    for tick in range(3):
        # ---- deaths (tombstones in the list: the next push is a delta) and new healthy rows for the carve
        alive = np.nonzero(st.nodes["status"] == orc.ST_HEALTHY)[0]
        for w in rng.choice(alive, size=40, replace=False):
            st.set_node_status(int(w), orc.ST_DEAD)
            flags[w] &= ~E.W_HEALTHY
            eng.on_worker_status(int(w), int(flags[w]), True)
        for w in np.nonzero(late & (status0 == orc.ST_HEALTHY))[0][tick::3]:
            st.set_node_status(int(w), orc.ST_HEALTHY)
            flags[w] |= E.W_HEALTHY
            eng.on_worker_status(int(w), int(flags[w]), False)
        before = [g[1:] for g in oracle_groups(st)]
        assert len(before) > 100
        ids = [before[i][0] for i in rng.integers(0, len(before), 6)] + [(1 << 63) | 3]
        workers = [int(w) for w in rng.integers(0, sw.W, 24)] + [int(before[0][2][0])]
        reads = []
        for p in phases:
            p()
            if p is eng.dist_tick_begin:                       # the carve runs on a list that carries tombstones
                assert eng.debug_task_space()["n_dead_groups"] > 0, tick
            if p is not eng.dist_tick_end:
                reads.append(_read_all(eng, ids, workers))
        want_of = {w: g for g in before for w in g[2]}
        st.try_form_new_groups()
        st.try_merge_solo_groups()
        want_tasks = [st.get_task_for_node(w) for w in range(sw.W)]
        after = [g[1:] for g in oracle_groups(st)]
        # in front of the merge pass the list is the one before the tick; behind it (phase 3) the merge has taken the
        # carve's groups in, and the tasks come with the publish
        assert [g[:3] for g in reads[2][2]] in ([g[:3] for g in before], [g[:3] for g in after]), tick
        for by_id, of_worker, groups in reads[:2]:
            assert groups == before, tick
            for gid, got in zip(ids, by_id):
                g = next((g for g in before if g[0] == gid), None)
                assert (got is None) == (g is None) and (got is None or (got["id"], got["config"], got["members"]) == g[:3])
                if got is not None:
                    assert got["slot"] == before.index(g)
            for w, got in zip(workers, of_worker):
                g = want_of.get(w)
                assert (got is None) == (g is None) and (got is None or (got["id"], got["slot"]) == (g[0], before.index(g)))
        assert [(-1 if eng.lookup(w).task == E.PM_NONE else eng.lookup(w).task) for w in range(sw.W)] == want_tasks, tick
        assert engine_groups(eng) == after, tick
    eng.close()


def test_soak_on_two_in_process_ranks():
    """the schedule (no burst, no republish: a multi-GPU engine has none) on two ranks through ShardedEngine; every
    rank equals the oracle after every tick"""
    ticks, seed = env_int("PM_SOAK_DIST_TICKS", 200), env_int("PM_SOAK_SEED", 1) + 1
    s = Soak(seed, ticks, burst=False, republish=False)
    engines = [E.Engine(group_id_seed=GROUP_ID_SEED) for _ in range(2)]
    for e in engines:
        s.load(e)
    grp = _InProcGroup(2)
    for k in range(ticks):
        s.interval(k)
        out, errs = [None, None], []

        def rank_main(r):
            try:
                se = ShardedEngine(EngineLocal(engines[r], torch.device("cuda", 0)), s.sw.address[:s.W],
                                   exchanger=_InProcExchanger(grp, r))
                out[r] = se.tick()
            except Exception as ex:  # a dead rank must not leave the other at the barrier
                errs.append((r, repr(ex)))
                grp.barrier.abort()

        th = [threading.Thread(target=rank_main, args=(r,)) for r in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, (s.where(k, "rank failed"), errs)
        tasks, want, events = s.oracle_tick()
        for r, e in enumerate(engines):
            s.compare(e, k, tasks, want, events, out[r])
            s.check_bounds(e, k)
    for e in engines:
        e.close()
