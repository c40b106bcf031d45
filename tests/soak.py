"""The long mixed-operation schedule of tests/test_gpu_soak.py and tests/test_soak_schedule.py: one seeded generator
drives the CPU oracle (orc.State) and any number of engines side by side, tick by tick, through everything a
management loop that runs forever does to the engine's incremental state — worker appends, deaths, revivals, row
rewrites, task inserts in front and deletes anywhere, dissolutions by id, reads between ticks, full re-uploads of the
unchanged tables and a configuration switched off for a while.

The oracle's node table is fixed-size: rows that have not arrived yet carry status 0 there.  Its task table goes
through set_tasks + remap_tasks, the engines' through pm_tasks_delete / pm_tasks_insert_front."""
import ctypes as C
import os

import numpy as np

from oracle import oracle_ffi as orc
from protocol_amd import engine as E
from protocol_amd import host
from protocol_amd.swarm import make_swarm

NONE = 0xFFFFFFFF
GROUP_ID_SEED = 0x5EED
TASK_DEAD_SLACK = 4096           # pm_engine_tasks.inc PM_TASK_DEAD_SLACK
WORKER_FIELDS = ("address", "status", "has_p2p", "has_specs", "has_gpu", "gpu_count_some", "gpu_mem_some",
                 "gpu_model_some", "has_cpu", "cpu_cores_some", "ram_some", "storage_some", "gpu_count", "gpu_mem_mb",
                 "gpu_model_id", "cpu_cores", "ram_mb", "storage_gb", "price", "has_loc", "lat", "lon")


def env_int(name, default):
    v = os.environ.get(name)
    return int(v) if v else default


def task_capacity_for(n):
    """pm_engine_tasks.inc task_capacity_for"""
    return min((2 * n + 65536 + 63) & ~63, 0xFFFFFFC0)


def rows_of(packed, idx):
    return {k: np.ascontiguousarray(v[idx]) for k, v in packed.items()}


def engine_groups(eng):
    """[(id, config, members in BTreeSet order, task or -1)] in creation order"""
    _, groups, members = eng.get_groups()
    return [(int(g["id"]), int(g["config"]), members[int(g["member_begin"]):int(g["member_begin"]) + int(g["n_members"])].tolist(),
             -1 if int(g["task"]) == NONE else int(g["task"])) for g in groups]


def oracle_groups(st):
    """State.groups() of the live groups only: [(slot, id, config, members, task)] in slot (creation) order.  The
    oracle never reuses a slot, so a long run's slot count grows without bound; every live group has members, and
    node_to_group names the slots that are alive."""
    n2g = st.node_to_group
    L, h = orc.lib(), st._h
    buf = np.zeros(max(len(st.nodes), 1), dtype=np.uint32)
    pbuf = buf.ctypes.data
    out = []
    gid, cfg, n, task = C.c_uint64(0), C.c_uint32(0), C.c_uint32(0), C.c_int64(0)
    for sl in np.unique(n2g[n2g >= 0]):
        if L.orc_group_info(h, int(sl), C.byref(gid), C.byref(cfg), C.byref(n), pbuf, len(buf), C.byref(task)):
            out.append((int(sl), gid.value, cfg.value, buf[:n.value].tolist(), task.value))
    return out


class Soak:
    """seed: the schedule; ticks: its length (the burst and the periodic events are placed by it); burst: whether
    the schedule carries the burst phase that outgrows the task index space; republish: whether some inserts go through
    pm_tasks_insert_front_ex (one engine only: a multi-GPU engine has no republish)"""

    def __init__(self, seed, ticks, *, W0=5000, W_extra=5000, T0=2000, burst=True, republish=True):
        self.seed, self.ticks = seed, ticks
        self.rng = np.random.default_rng(seed)
        self.sample_rng = np.random.default_rng(seed + 1)         # (the comparison's samples: the schedule stays the same)
        r = self.rng
        Wmax = W0 + W_extra
        sw = make_swarm(1000 + seed % 1000, T0, Wmax)
        donor = make_swarm(2000 + seed % 1000, 10, Wmax)
        late = np.arange(W0, Wmax)
        # rows that arrive later: a tenth unhealthy on arrival, a tenth without a location
        sw.status[late[r.random(len(late)) < 0.1]] = orc.ST_UNHEALTHY
        sw.has_loc[late[r.random(len(late)) < 0.1]] = False
        self.sw, self.donor = sw, donor
        self.packed = host.pack_workers(sw)                    # the rows as the engines hold them (flags current)
        nodes, cfgs, tasks, enabled = orc.from_swarm(sw)
        self.arrival_status = nodes["status"].copy()
        nodes["status"][W0:] = 0                               # not there yet
        self.st = orc.State(nodes, cfgs, enabled=enabled, tasks=tasks, reference_shaped=False, group_id_seed=GROUP_ID_SEED)
        self.enabled0 = enabled.copy()
        self.enabled_mask = sw.enabled_mask()
        self.W, self.Wmax, self.T0 = W0, Wmax, T0
        # the task list (get_all_tasks order) and a pool of rows new tasks are drawn from
        self.tasks, self.masks = tasks.copy(), sw.task_masks()
        self.created, self.uid = sw.created_at.copy(), sw.task_uid.copy()
        self.pool_tasks, self.pool_masks = tasks.copy(), self.masks.copy()
        self.next_uid = 1 << 42
        self.engines = []
        # the schedule's own shape: where the burst and the disabled windows lie
        self.burst_ticks = set()
        if burst:
            b0 = ticks // 2
            self.burst_in = {b0: 24000, b0 + 1: 24000, b0 + 2: 24000}
            self.burst_out = {b0 + 3 + k: 15000 for k in range(5)}
            self.burst_ticks = set(range(b0, b0 + 8))
        else:
            self.burst_in, self.burst_out = {}, {}
        self.republish = republish
        self.mask_off = {}                                     # tick -> (config, until)
        for t0 in range(150, ticks, 200):
            self.mask_off[t0] = t0 + 20
        self.cov = dict(claimed_deletes=0, dissolve_hits=0, dissolve_misses=0, revivals=0, deaths=0, appends=0,
                        rewrites=0, reads=0, read_ticks=0, resyncs=0, mask_toggles=0, merges=0, min_groups=1 << 30,
                        max_T=len(self.tasks), max_insert=0, republishes=0, unknown_deletes=0, twice_deletes=0,
                        front_deletes=0, tail_deletes=0)
        self.disabled = None
        self.last_want = None

    # ------------------------------------------------------------------ engines
    def load(self, eng):
        host.load_swarm(eng, self.take_sw(self.W))
        eng.upload_workers(rows_of(self.packed, np.arange(self.W)))   # (ranks over the final address set: stable)
        eng.enable_group_events()
        self.engines.append(eng)

    def take_sw(self, n):
        import copy
        s = copy.copy(self.sw)
        for k in WORKER_FIELDS:
            setattr(s, k, getattr(self.sw, k)[:n].copy())
        return s

    def each(self, f):
        for e in self.engines:
            f(e)

    # ------------------------------------------------------------------ one interval between two ticks
    def claimed(self):
        """the claimed tasks as the last tick left them (the oracle's groups are read once a tick: see oracle_groups)"""
        if self.last_want is None:
            self.last_want = [g[1:] for g in oracle_groups(self.st)]
        return [g[3] for g in self.last_want if g[3] >= 0]

    def task_ops(self, k):
        r, st = self.rng, self.st
        T = len(self.tasks)
        n_new = self.burst_in.get(k, int(r.integers(50, 301)))
        if k in self.burst_out:
            n_del = self.burst_out[k]
        elif k in self.burst_in:
            n_del = int(r.integers(50, 301))
        else:                                                  # steady state: about as many go as come, back towards T0
            n_del = int(np.clip(n_new + (T - self.T0) // 2 + int(r.integers(-40, 41)), 50, 300))
        n_del = min(n_del, max(T - 500, 0))
        kill = set()
        claimed = sorted(set(self.claimed()))
        if claimed:
            pick = r.choice(claimed, size=min(len(claimed), int(r.integers(1, 6))), replace=False)
            kill |= set(int(x) for x in pick)
            self.cov["claimed_deletes"] += len(pick)
        if T and r.random() < 0.3:
            kill |= {0, 1}                                     # the front tasks
            self.cov["front_deletes"] += 1
        n_tail = min(n_del // 3, T)
        kill |= set(range(T - n_tail, T))                      # the oldest
        self.cov["tail_deletes"] += n_tail
        while len(kill) < n_del:
            kill.add(int(r.integers(0, T)))                    # anywhere in the middle
        keep = np.ones(T, dtype=bool)
        keep[list(kill)] = False
        dele = list(self.uid[~keep])
        if r.random() < 0.5:
            dele.append(np.uint64((1 << 62) + k))              # an id nobody has
            self.cov["unknown_deletes"] += 1
        if len(dele) > 1 and r.random() < 0.5:
            dele.append(dele[0])                               # an id named twice
            self.cov["twice_deletes"] += 1
        pick = r.integers(0, len(self.pool_tasks), n_new)
        new_rows = self.pool_tasks[pick].copy()
        new_created = int(self.created.max()) + 1 + np.arange(n_new)[::-1]
        new_rows["created_at"] = new_created
        new_masks = self.pool_masks[pick]
        new_uid = np.arange(self.next_uid, self.next_uid + n_new, dtype=np.uint64)
        self.next_uid += n_new
        old_to_new = np.where(keep, n_new + np.cumsum(keep) - 1, -1)
        self.tasks = np.concatenate([new_rows, self.tasks[keep]])
        self.masks = np.concatenate([new_masks, self.masks[keep]])
        self.created = np.concatenate([new_created, self.created[keep]])
        self.uid = np.concatenate([new_uid, self.uid[keep]])
        st.set_tasks(self.tasks)
        st.remap_tasks(old_to_new)
        republish = self.republish and k % 3 == 1 and k not in self.burst_ticks
        self.cov["republishes"] += republish
        n_gone = int((~keep).sum())
        dele = np.array(dele, dtype=np.uint64)

        def apply(e):
            before = self.hook(e)
            assert e.tasks_delete(dele) == n_gone, self.where(k, "tasks_delete")
            e.tasks_insert_front(new_masks, new_created, new_uid, republish=republish)
            assert e.T == len(self.masks), self.where(k, "T")
            self.note_rebuilds(e, before, claimed)
        self.each(apply)
        self.cov["max_T"] = max(self.cov["max_T"], len(self.tasks))
        self.cov["max_insert"] = max(self.cov["max_insert"], n_new)

    def worker_ops(self, k):
        r, st, P = self.rng, self.st, self.packed
        # ---- brand-new rows
        n_app = min(int(r.integers(0, 9)), self.Wmax - self.W)
        if n_app:
            idx = np.arange(self.W, self.W + n_app)
            for e in self.engines:
                assert e.append_workers(rows_of(P, idx)) == self.W
            for w in idx:
                st.set_node_status(int(w), int(self.arrival_status[w]))
            self.W += n_app
            self.cov["appends"] += n_app
        # ---- deaths (the whole group dissolves) and revivals
        status = st.nodes["status"][:self.W]
        alive = np.nonzero(status == orc.ST_HEALTHY)[0]
        down = np.nonzero((status == orc.ST_DEAD) | (status == orc.ST_UNHEALTHY))[0]
        dies = r.choice(alive, size=min(len(alive), int(r.integers(5, 26))), replace=False)
        back = r.choice(down, size=min(len(down), int(r.integers(0, 21))), replace=False)
        ws, fl, dd = [], [], []
        for w in dies:
            st.set_node_status(int(w), orc.ST_DEAD)
            P["flags"][w] &= ~np.uint32(E.W_HEALTHY)
            ws.append(int(w)), fl.append(int(P["flags"][w])), dd.append(1)
        for w in back:
            st.set_node_status(int(w), orc.ST_HEALTHY)
            P["flags"][w] |= np.uint32(E.W_HEALTHY)
            ws.append(int(w)), fl.append(int(P["flags"][w])), dd.append(0)
        self.cov["deaths"] += len(dies)
        self.cov["revivals"] += len(back)
        if k % 2:
            self.each(lambda e: e.on_worker_status_many(ws, fl, dd))
        else:
            for w, f, d in zip(ws, fl, dd):
                self.each(lambda e: e.on_worker_status(w, f, bool(d)))
        # ---- known rows rewritten by the discovery sync: specs, location
        if k % 10 == 3:
            idx = r.choice(self.W, size=12, replace=False)
            for f in WORKER_FIELDS:
                if f not in ("address", "status"):
                    getattr(self.sw, f)[idx] = getattr(self.donor, f)[idx]
            fresh = host.pack_workers(self.sw)
            for key in P:
                if key != "flags":
                    P[key][idx] = fresh[key][idx]
            healthy = st.nodes["status"][idx] == orc.ST_HEALTHY
            P["flags"][idx] = np.where(healthy, fresh["flags"][idx] | E.W_HEALTHY,
                                       fresh["flags"][idx] & ~np.uint32(E.W_HEALTHY)).astype(np.uint32)
            rows = rows_of(P, idx)
            self.each(lambda e: e.update_workers(idx, rows))
            fresh_nodes = orc.from_swarm(self.sw)[0]
            for w in idx:
                keep = int(st.nodes["status"][w])
                st.nodes[w] = fresh_nodes[w]
                st.nodes["status"][w] = keep
            self.cov["rewrites"] += 1

    def dissolve(self, k):
        if k % 7 != 5:
            return
        gs = oracle_groups(self.st)
        if self.rng.random() < 0.2 or not gs:
            gid = (1 << 63) | k                                # no such group: Ok(()), nothing happens
            for e in self.engines:
                assert e.dissolve_group_by_id(gid) is False, self.where(k, "dissolve of an unknown id")
            self.cov["dissolve_misses"] += 1
            return
        slot, gid = gs[int(self.rng.integers(0, len(gs)))][:2]
        self.st.dissolve_group(slot)
        for e in self.engines:
            assert e.dissolve_group_by_id(gid) is True, self.where(k, f"dissolve of group {gid:#x}")
        self.cov["dissolve_hits"] += 1

    def reads(self, k):
        """get_group_by_id / get_group_of_worker / get_groups against the oracle (they compact the engine's list)"""
        if k % 3 != 0:
            return
        want = [(gid, cfg, mem, task) for (_s, gid, cfg, mem, task) in oracle_groups(self.st)]
        of = {w: g for g in want for w in g[2]}
        probes = [want[int(i)] for i in self.rng.integers(0, len(want), 3)] if want else []
        workers = [int(w) for w in self.rng.integers(0, self.W, 4)]
        for e in self.engines:
            for g in probes:
                got = e.get_group_by_id(g[0])
                assert got is not None, self.where(k, f"read of group {g[0]:#x}: not found")
                assert (got["id"], got["config"], got["members"], -1 if got["task"] == NONE else got["task"]) == g, \
                    self.where(k, f"read of group {g[0]:#x}")
            assert e.get_group_by_id((1 << 63) | 7) is None
            for w in workers:
                got = e.get_group_of_worker(w)
                g = of.get(w)
                if g is None:
                    assert got is None, self.where(k, f"read of worker {w}: in a group")
                else:
                    assert got is not None and (got["id"], got["members"]) == (g[0], g[2]), self.where(k, f"read of worker {w}")
            self.same_groups(e, want, k, "read")
        self.cov["reads"] += len(probes) + len(workers) + 1
        self.cov["read_ticks"] += 1

    def resync(self, k):
        if k % 250 != 200:
            return
        rows = rows_of(self.packed, np.arange(self.W))
        for e in self.engines:
            e.upload_tasks(self.masks, self.created, self.uid)
            e.upload_workers(rows, keep_groups=True)
        self.cov["resyncs"] += 1

    def mask(self, k):
        if k in self.mask_off:
            on = [i for i in range(len(self.enabled0)) if self.enabled0[i] and self.st.enabled[i]]
            c = on[int(self.rng.integers(0, len(on)))]
            self.disabled = (c, self.mask_off[k])
            en = self.enabled0.copy()
            en[c] = 0
            self.st.set_enabled(en)
            self.each(lambda e: e.set_enabled_mask(self.enabled_mask & ~(1 << c)))
            self.cov["mask_toggles"] += 1
        elif self.disabled and k == self.disabled[1]:
            self.st.set_enabled(self.enabled0.copy())
            self.each(lambda e: e.set_enabled_mask(self.enabled_mask))
            self.disabled = None

    def interval(self, k):
        """everything between tick k-1 and tick k, on the oracle and every engine"""
        self.mask(k)
        self.task_ops(k)
        self.worker_ops(k)
        self.dissolve(k)
        self.reads(k)
        self.resync(k)

    # ------------------------------------------------------------------ the oracle's tick and the comparison
    def oracle_tick(self):
        st = self.st
        st.try_form_new_groups()
        self.cov["merges"] += st.try_merge_solo_groups()
        tasks = [st.get_task_for_node(w) for w in range(self.W)]   # (the oracle claims on this call)
        want = [(gid, cfg, mem, task) for (_s, gid, cfg, mem, task) in oracle_groups(st)]
        self.cov["min_groups"] = min(self.cov["min_groups"], len(want))
        self.last_want = want
        return tasks, want, st.drain_events()

    def compare(self, e, k, tasks, want, events, stats):
        W = self.W
        got = [(-1 if e.lookup(w).task == NONE else e.lookup(w).task) for w in range(W)]
        if got != tasks:
            w = next(i for i in range(W) if got[i] != tasks[i])
            raise AssertionError(self.where(k, f"worker {w}: task {got[w]}, the oracle {tasks[w]}"))
        self.same_groups(e, want, k, "tick")
        ev = e.drain_group_events()
        if ev != events:
            i = next((i for i in range(min(len(ev), len(events))) if ev[i] != events[i]), min(len(ev), len(events)))
            raise AssertionError(self.where(k, f"event {i} of {len(ev)} / {len(events)}: {ev[i:i + 1]} vs {events[i:i + 1]}"))
        for w in self.sample_rng.choice(W, size=64, replace=False):
            t, gi, gs, nxt = self.st.filter_tasks(int(w))
            a = e.lookup(int(w))
            if t >= 0:
                assert (a.group_index, a.group_size, a.next_worker) == (gi, gs, nxt), self.where(k, f"worker {w}: row")
        assert stats["host_resolved_steps"] == 0, self.where(k, "host-resolved steps")

    def same_groups(self, e, want, k, what):
        got = engine_groups(e)
        if got != want:
            i = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
            raise AssertionError(self.where(k, f"{what}: group {i} of {len(got)} / {len(want)}: "
                                               f"{got[i:i + 1]} vs the oracle's {want[i:i + 1]}"))

    # ------------------------------------------------------------------ the engines' index space
    @staticmethod
    def hook(e):
        return e.debug_task_space() if hasattr(e, "debug_task_space") else None

    def note_rebuilds(self, e, before, claimed):
        after = self.hook(e)
        if before is None or not claimed:
            return
        self.cov.setdefault("regrowths_claimed", 0)
        self.cov.setdefault("compactions_claimed", 0)
        self.cov["regrowths_claimed"] += after["regrowths"] - before["regrowths"]
        self.cov["compactions_claimed"] += after["compactions"] - before["compactions"]

    def check_bounds(self, e, k):
        s = e.debug_task_space()
        assert s["t_dead"] <= s["T"] + TASK_DEAD_SLACK, self.where(k, f"task tombstones {s}")
        assert s["t_cap"] - s["t_lo"] <= 2 * s["T"] + TASK_DEAD_SLACK, self.where(k, f"swept range {s}")
        assert s["t_cap"] <= task_capacity_for(2 * self.cov["max_T"] + TASK_DEAD_SLACK + self.cov["max_insert"]), \
            self.where(k, f"task capacity {s}")
        assert s["n_dead_groups"] * 4 <= s["n_groups"] + 256, self.where(k, f"group tombstones {s}")
        assert s["retired_buffers"] <= 32, self.where(k, f"retired snapshot buffers {s}")
        return s

    def where(self, k, what):
        return f"soak seed {self.seed}, tick {k}: {what}"
