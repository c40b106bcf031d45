"""Every ledger and directory together on one churning engine: the schedule and the models of tests/test_gpu_ledger_soak.py
and tests/test_ledger_soak_schedule.py.  A LedgerSoak owns a Soak (tests/soak.py, as it is) and, beside the oracle, carries the
models of the optional structures for the whole run: liveness_model.Ledger, metrics_model.Ledger, rollout_model.Ledger, the
address bytes of every row, and the expected change feed of every engine.  The models are the truth: they are never refilled
from an engine's reads, the reads are compared with them.

Between Soak.interval(k) and the tick every ledger is fed (ledger_steps); after the tick and the soak's own comparison every
read is compared (check): the ledgers on every tick, the rollout reads and a rotating pair of queries per directory on every
third, the spread report, the nearest-candidates query and the configuration report on every twelfth.  Without an engine the
same schedule runs on the oracle and the models alone, and counts what it exercises (cov).

Everything new draws from np.random.default_rng(seed + 2): the Soak's own streams are untouched.

The address book installs its ranks exactly as pm_set_addr_ranks would.  The book's addresses are not the swarm's (they are
rewritten, and tie on ten characters), so after the ranks and the reads that depend on them are compared, the swarm's ranks go
back with pm_set_addr_ranks: the tick runs under the order the oracle knows."""
import math

import numpy as np

from oracle import oracle_ffi as orc
from protocol_amd import engine as E
from protocol_amd import host
from protocol_amd.addresses import make_addresses
from soak import NONE, Soak, oracle_groups, rows_of

import addresses_model as AM
import changes_model as CM
import directory_model as DM
import discovery_model as DSM
import groupdir_model as GM
import liveness_model as LM
import metrics_model as MM
import near_model as NM
import report_model as RPM
import rollout_model as RM
import spread_model as SM
import taskdir_model as TM

SHAPES = {"small": dict(W0=900, W_extra=600, T0=1000, burst=False),
          "wide": dict(W0=1300, W_extra=800, T0=1000, burst=False)}
NOW0 = 1_760_000_000_000
STEP_MS = 30_000                 # an interval: a beat is present for three of them (LM.TTL_MS)
RO_CHUNK = 1024                  # PM_RO_CHUNK, PM_MX_CHUNK (pm_device.h): the tests that read the source assert it
ESTATE = -4
ALL_CLASSES = (1 << RM.RO_N) - 1
VALUES = [0.0, -0.0, 1.0, -1.0, 2.5, 1e300, -1e300, float("inf"), float("-inf"), float("nan"), 5e-324, 3.0]


# ---------------------------------------------------------------------------------------------------------------- queries
# the query lists and the readers are those of the three directory test files, of tests/test_gpu_rollout.py and of
# tests/test_gpu_discovery.py themselves (the modules import without a GPU; their tests are marked gpu)
import test_gpu_directory as TND
import test_gpu_discovery as TDS
import test_gpu_groupdir as TGD
import test_gpu_rollout as TRO
import test_gpu_taskdir as TTD


def node_queries():
    return TND._every_query() + TND.LIFE_QUERIES


def group_queries(n_cfgs):
    return TGD._every_query(True, True, n_cfgs) + TGD._life_queries(n_cfgs)


def task_queries(n_cfgs):
    return TTD._every_query(True, n_cfgs) + TTD._life_queries(n_cfgs)


node_read, group_read, task_read, rollout_reads, disc_dicts = TND._read, TGD._read, TTD._read, TRO._reads, TDS._as_dicts


def runs(rows):
    """sorted rows as [(first, n)] of consecutive runs"""
    out = []
    for w in sorted(int(x) for x in rows):
        if out and out[-1][0] + out[-1][1] == w:
            out[-1][1] += 1
        else:
            out.append([w, 1])
    return out


def code_of(call):
    try:
        call()
    except E.EngineError as err:
        return err.code
    return 0


class Spy:
    """An engine as the Soak drives it, with the calls that bear on the change feed watched: a publish by
    pm_tasks_insert_front_ex(republish = 1) is given to the feed's model with the rows as published at that moment, and
    pm_upload_tasks, pm_upload_workers(keep_groups = 0) and a rebuild of the task index space mark its resync."""

    def __init__(self, eng, owner):
        self.eng, self.owner, self.feed = eng, owner, CM.Feed()

    def __getattr__(self, name):
        return getattr(self.eng, name)

    def _rebuilt(self, call):
        a = self.eng.debug_task_space()
        out = call()
        b = self.eng.debug_task_space()
        if (a["regrowths"], a["compactions"]) != (b["regrowths"], b["compactions"]):
            self.feed.resync()
            self.owner.cov["feed_rebuild_resyncs"] += 1
        return out

    def tasks_delete(self, uids):
        return self._rebuilt(lambda: self.eng.tasks_delete(uids))

    def tasks_insert_front(self, topo_mask, created_at, uid=None, republish=False):
        self._rebuilt(lambda: self.eng.tasks_insert_front(topo_mask, created_at, uid, republish=republish))
        if republish:
            self.feed.publish(self.table())

    def upload_tasks(self, *a, **kw):
        self.feed.resync()
        return self.eng.upload_tasks(*a, **kw)

    def upload_workers(self, cols, keep_groups=False):
        if not keep_groups:
            self.feed.resync()
        return self.eng.upload_workers(cols, keep_groups=keep_groups)

    def table(self):
        uid, out = self.owner.s.uid, []
        for w in range(self.eng.W):
            a = self.eng.lookup(w)
            out.append(CM.row_of(a.group_slot, a.group_id, a.group_index, a.group_size, a.next_worker,
                                 None if a.task == NONE else int(uid[a.task])))
        return out


class LedgerSoak:
    def __init__(self, seed, ticks, shape="small"):
        self.seed, self.ticks, self.shape = seed, ticks, shape
        self.s = s = Soak(seed, ticks, **SHAPES[shape])
        self.r = r = np.random.default_rng(seed + 2)
        self.cfgs = orc.from_swarm(s.sw)[1]
        cfg_rows, alt_rows, req_models = host.pack_configs(s.sw.configs)
        self.cfg_pack = (cfg_rows, alt_rows, host.build_model_table(req_models, s.sw.model_names), len(s.sw.model_names))
        self.C = len(s.sw.configs)
        self.full = []                                                   # the engines with everything on, as Spies
        W = s.W
        flags = s.packed["flags"][:W]
        self.m = 3
        self.live = LM.Ledger(flags, self.m)
        self.mx, self.ro = MM.Ledger(), RM.Ledger()
        self.healthy = (flags & E.W_HEALTHY) != 0
        self.W_seen = W
        self.now = NOW0
        self.beats = np.zeros(W, dtype=np.uint64)
        self.in_pool = r.random(W) < 0.7
        self.mute_until = np.zeros(W, dtype=np.int64)
        self.ep_of = self._endpoints(W)
        self.listed = []                                                 # the last sweep's list
        # the address book: a supply of letter-led addresses; 90 % of the first rows hold one at load, the rest from interval 1
        self.supply = make_addresses(3000 + seed, 2 * s.Wmax + 800 + 2 * ticks, "letter_led")
        self.next_addr = 0
        self.addr, self.text = {}, {}
        held = r.random(W) < 0.9
        for w in np.flatnonzero(held):
            self._model_address(int(w), self._fresh_address())
        self.unheld = [int(w) for w in np.flatnonzero(~held)]
        self.ties = []                                                   # (row, the row it ties with)
        # rollout: what every row's group claims now, and what it claimed before that
        self.cur_uid, self.old_uid = {}, {}
        self.ro_phase, self.ro_keys = "grow", None
        self.nq, self.gq, self.tq = node_queries(), group_queries(self.C), task_queries(self.C)
        self.events = {}
        self.life = {"rollout_enable": ticks // 3, "metrics_enable": ticks // 2, "liveness_enable": (2 * ticks) // 3}
        self.cov = dict(emptied_by_sweep=0, sweep_dead=0, same_interval_reports=0, ties=0, key_crossings=0, max_keys=0, min_keys=1 << 30,
                        W_max=W, T_min=len(s.tasks), T_max=len(s.tasks), T_crossings=0, groups_min=1 << 30, groups_max=0,
                        group_crossings=0, members_plus_groups_max=0, configs_in_use=set(), node_orders={}, group_orders={},
                        task_orders={}, discoveries=0, disc_updates=0, feed_rebuild_resyncs=0, late_growth=0, report_reads=0,
                        rollout_reads=0, old_claim_reports=0, stranger_reports=0, twice_reports=0, clears=0)
        self._last = dict(T=len(s.tasks), groups=None, keys=None)
        self.first_W_above = {1024: None, 2048: None}                    # the tick at which W passes a chunk edge

    # ------------------------------------------------------------------------------------------------------------ helpers
    def where(self, k, structure, what):
        return self.s.where(k, f"{structure}: {what}")

    def same(self, k, structure, got, want, name="row"):
        """two lists: equal, or the first place where they are not"""
        if got == want:
            return
        n = min(len(got), len(want))
        i = next((i for i in range(n) if got[i] != want[i]), n)
        raise AssertionError(self.where(k, structure, f"{name} {i} of {len(got)} / {len(want)}: {got[i:i + 1]} vs the model's {want[i:i + 1]}"))

    def each(self, f):
        for e in self.full:
            f(e)

    def _endpoints(self, n):
        """a row's endpoint: its own, or (one row in ten) one of eight shared ones"""
        r = self.r
        return np.where(r.random(n) < 0.1, r.integers(0, 8, n), 1000 + r.integers(0, 1 << 20, n)).astype(np.int64)

    def _fresh_address(self):
        a = self.supply[self.next_addr].tobytes()
        self.next_addr += 1
        return a

    def _model_address(self, w, a):
        self.addr[w] = a
        self.text[w] = E.host_eip55(a)

    def _tying_address(self, other):
        """an address whose EIP-55 text shares its first ten characters with row `other`'s, and no more than that on purpose"""
        head, want = self.addr[other][:5], self.text[other][2:12]
        while True:
            a = head + self.r.integers(0, 256, 15, dtype=np.uint8).tobytes()
            if a != self.addr[other] and E.host_eip55(a)[2:12] == want:
                assert AM.eip55(a)[2:12] == AM.eip55(self.addr[other])[2:12]      # (the tie by the model's own sponge)
                return a

    def _set_addresses(self, rows):
        for first, n in runs(rows):
            block = np.frombuffer(b"".join(self.addr[w] for w in range(first, first + n)), dtype=np.uint8).reshape(n, 20)
            self.each(lambda e: e.set_addresses(first, block))

    def groups(self):
        """the oracle's groups as the last tick left them [(id, config, members, task position or -1)], and group_of [W]"""
        want = self.s.last_want or []
        group_of = np.full(self.s.W, -1, dtype=np.int64)
        for slot, g in enumerate(want):
            group_of[g[2]] = slot
        return want, group_of

    # ------------------------------------------------------------------------------------------------------------ engines
    def load(self, eng):
        """an engine with everything on -> the Spy the tests tick"""
        spy = Spy(eng, self)
        self.s.load(spy)
        eng.enable_assignment_changes(True)
        eng.liveness_enable(True, self.m)
        eng.metrics_enable(True)
        eng.rollout_enable(True)
        eng.enable_addresses(True)
        self.full.append(spy)
        for first, n in runs(self.addr):
            block = np.frombuffer(b"".join(self.addr[w] for w in range(first, first + n)), dtype=np.uint8).reshape(n, 20)
            eng.set_addresses(first, block)
        return spy

    # ------------------------------------------------------------------------------------------------------------ interval
    def interval(self, k):
        self.s.interval(k)
        self.life_events(k)
        self.ledger_steps(k)

    def life_events(self, k):
        s = self.s
        if k == self.life["rollout_enable"]:
            self.each(lambda e: e.rollout_enable(True))
            self.ro.clear()
            self.events["rollout_enable"] = k
        if k == self.life["metrics_enable"]:
            self.each(lambda e: (e.metrics_enable(False), e.metrics_enable(True)))
            self.mx = MM.Ledger()
            self.events["metrics_enable"] = k
        if k == self.life["liveness_enable"]:
            self.m = 1
            self.each(lambda e: e.liveness_enable(True, 1))
            self.live = LM.Ledger(s.packed["flags"][:s.W], 1)            # from the host's flags as they are now
            self.listed = []
            self.events["liveness_enable"] = k
        if s.cov["resyncs"] and "resync" not in self.events:
            self.events["resync"] = k
        if s.disabled and "masked" not in self.events:
            self.events["masked"] = k

    def ledger_steps(self, k):
        s, r = self.s, self.r
        W0, W = self.W_seen, s.W
        flags = s.packed["flags"][:W]
        new = list(range(W0, W))
        n_new = W - len(self.beats)
        if n_new:
            self.beats = np.concatenate([self.beats, np.zeros(n_new, dtype=np.uint64)])
            self.in_pool = np.concatenate([self.in_pool, r.random(n_new) < 0.7])
            self.mute_until = np.concatenate([self.mute_until, np.zeros(n_new, dtype=np.int64)])
            self.ep_of = np.concatenate([self.ep_of, self._endpoints(n_new)])
        self.cov["W_max"] = max(self.cov["W_max"], W)
        for edge in self.first_W_above:
            if W0 <= edge < W and self.first_W_above[edge] is None:
                self.first_W_above[edge] = k
        # ---- liveness: the ledger sees the new rows with the flags they have NOW; the rows the soak flipped are written
        self.live.append(flags[len(self.live.status):W])           # (a ledger enabled again in this interval has them)
        healthy = (flags & E.W_HEALTHY) != 0
        flipped = np.flatnonzero(healthy[:len(self.healthy)] != self.healthy)
        flipped = flipped[flipped < W0]
        st = np.where(healthy[flipped], LM.HEALTHY, LM.DEAD).astype(np.uint8)
        self.live.set(flipped, st)
        self.each(lambda e: e.liveness_set(flipped, st))
        self.healthy, self.W_seen = healthy.copy(), W
        self.now += STEP_MS
        for w in r.choice(W, size=6, replace=False):                     # six rows fall silent for ten intervals
            self.mute_until[w] = k + 10
        chatty = (r.random(W) < 0.8) & (self.mute_until <= k)
        self.beats = np.where(chatty, self.now - r.integers(0, STEP_MS // 2, size=W), self.beats).astype(np.uint64)
        if k % 50 == 49:
            self.in_pool = r.random(W) < 0.7
        pool = LM.pack_bits(self.in_pool) if k % 4 else None
        rows, census = self.live.sweep(self.now, self.beats, pool)
        self.listed = rows
        for e in self.full:
            n, got_census = e.liveness_sweep(self.now, self.beats, pool, apply=False)
            if n != len(rows) or got_census.tolist() != census:
                raise AssertionError(self.where(k, "liveness sweep", f"{n} rows, census {got_census.tolist()} vs the model's {len(rows)}, {census}"))
            self.check_transitions(e, k)
        dead = [w for w, _, new, _ in rows if new == LM.DEAD]
        self.cov["sweep_dead"] += len(dead)
        for w in dead:                                                   # the hook: a row the sweep turned Dead loses its metrics
            if self.mx.rows.get(w):
                self.cov["emptied_by_sweep"] += 1
            self.mx.clear_row(w)
        # ---- metrics: one batch over the rows appended now, rows the sweep just listed, and others
        self.metrics_step(k, new, rows)
        # ---- rollout
        self.rollout_step(k, new)
        # ---- address book
        self.address_step(k, new)
        # ---- discovery
        if k % 8 == 7:
            self.discovery_step(k)

    def check_transitions(self, e, k):
        t = e.liveness_transitions()
        assert np.all(t["_pad"] == 0)
        got = [(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(t["worker"], t["old_status"], t["new_status"], t["counter"])]
        self.same(k, "liveness transitions", got, self.listed)

    def metrics_step(self, k, new, listed):
        r, W = self.r, self.s.W
        S = int(r.integers(3, 41))
        ailing = [w for w, _, nw, _ in listed if nw == LM.UNHEALTHY]
        others = [w for w, _, nw, _ in listed if nw != LM.UNHEALTHY]
        rows = [int(w) for w in r.choice(W, size=16, replace=False)] + new
        for part in (ailing, others):
            if part:
                rows += [int(w) for w in r.choice(part, size=min(len(part), 8), replace=False)]
        if k % 5 == 0:
            rows.append(MM.MANUAL)
        per_row = []
        for row in rows:
            for _ in range(int(r.integers(1, 3))):
                n = int(r.integers(1 if row in ailing else 0, 7))
                ser = r.integers(0, S, size=n)
                vals = [float(VALUES[int(i)]) if r.random() < 0.3 else float(r.normal() * 10.0 ** int(r.integers(-3, 4)))
                        for i in r.integers(0, len(VALUES), size=n)]
                kind = MM.MERGE if row in ailing else int(r.choice([MM.REPLACE, MM.REPLACE, MM.MERGE, MM.MERGE, MM.DELETE]))
                per_row.append((row, kind, [(int(x), int(r.integers(0, 2)), v) for x, v in zip(ser, vals)]))
        beats, entries = [], []
        for i in (r.permutation(len(per_row)) if k % 2 else np.arange(len(per_row))):
            row, kind, ents = per_row[int(i)]
            beats.append((row, kind, len(entries), len(ents)))
            entries += ents
        self.mx.ingest(beats, entries, S)
        b = np.array(beats, dtype=E.mx_beat_dt)
        en = np.array(entries, dtype=E.mx_entry_dt) if entries else np.zeros(0, dtype=E.mx_entry_dt)
        self.each(lambda e: e.metrics_ingest(b, en, S))

    def rollout_step(self, k, new):
        s, r = self.s, self.r
        want = [g[1:] for g in oracle_groups(s.st)]                      # the groups as the interval left them
        uid = s.uid
        claimed = [g for g in want if g[3] >= 0]
        keys = len(self.ro.rows) + len(claimed)
        if keys > RO_CHUNK + 40:
            self.ro_phase = "shrink"
        elif keys < RO_CHUNK - 40:
            self.ro_phase = "grow"
        share = 0.35 if self.ro_phase == "grow" else 0.05
        reps = []
        for _gid, _cfg, mem, t in claimed:
            if r.random() < share:
                reps += [(w, RM.RUNNING if r.random() < 0.7 else int(r.integers(0, RM.TS_N)), int(uid[t])) for w in mem if w % 5]
        stale = [w for w in self.old_uid if w % 5]
        for w in (r.choice(stale, size=min(len(stale), 5), replace=False) if stale else []):
            reps.append((int(w), RM.RUNNING, self.old_uid[int(w)]))       # the task its group held before
            self.cov["old_claim_reports"] += 1
        for i, w in enumerate(r.choice(s.W, size=4, replace=False)):      # strangers: ids no task carries
            reps.append((int(w), int(r.integers(0, RM.TS_N)), (1 << 61) + 8 * k + i))
            self.cov["stranger_reports"] += 1
        for w in new:                                                     # rows appended in this very interval
            if r.random() < 0.6:
                reps.append((w, RM.PULLING, int(uid[int(r.integers(0, len(uid)))])))
                self.cov["same_interval_reports"] += 1
        reporters = sorted(self.ro.rows)
        n_clear = 150 if self.ro_phase == "shrink" else 3
        for w in (r.choice(reporters, size=min(len(reporters), n_clear), replace=False) if reporters else []):
            reps.append((int(w), RM.TS_NONE, 0))
            self.cov["clears"] += 1
        order = r.permutation(len(reps))
        reps = [reps[int(i)] for i in order]
        for i in r.integers(0, len(reps), size=min(3, len(reps))):        # rows named twice: the last report wins
            w = reps[int(i)][0]
            reps.append((w, RM.FAILED, int(uid[0])))
            self.cov["twice_reports"] += 1
        self.ro.ingest(reps)
        out = np.zeros(len(reps), dtype=E.ro_report_dt)
        for i, rep in enumerate(reps):
            out[i] = rep
        self.each(lambda e: e.rollout_ingest(out))

    def address_step(self, k, new):
        r = self.r
        rows = list(new)
        if k == 1:
            rows += self.unheld
            self.unheld = []
        for w in rows:
            self._model_address(w, self._fresh_address())
        if k % 10 == 9 and not self.unheld:
            known = [int(w) for w in r.choice(self.W_seen - len(new), size=12, replace=False)]
            for i, w in enumerate(known):
                if i < 2:
                    other = int(r.integers(0, self.W_seen - len(new)))
                    while other in known:
                        other = int(r.integers(0, self.W_seen - len(new)))
                    self._model_address(w, self._tying_address(other))
                    self.ties.append((w, other))
                    self.cov["ties"] += 1
                else:
                    self._model_address(w, self._fresh_address())
            rows += known
        self._set_addresses(rows)

    def discovery_step(self, k):
        r, W, now = self.r, self.s.W, self.now
        G = DSM.GRACE_MS
        stamps = [None, now - G - 1, now - G + 1, now - 1000, now - 10 * G]
        ip = lambda ep: "10.%d.%d.%d" % ((ep >> 16) & 255, (ep >> 8) & 255, ep & 255)
        nodes = [DSM.node("a%05d" % w, self.live.status[w], ip(int(self.ep_of[w])), 8080, stamps[int(r.integers(0, len(stamps)))],
                          None if r.random() < 0.5 else "loc", "specs-a" if r.random() < 0.5 else "specs-b") for w in range(W)]
        store = DSM.make_store(nodes)
        discovery = []
        for w in r.choice(W, size=40, replace=False):
            n = nodes[int(w)]
            addr = n["ip_address"] if r.random() < 0.7 else ip(int(r.integers(0, 8)))
            discovery.append(DSM.sighting(n["address"], addr, 8080, r.random() < 0.9, r.random() < 0.8, r.random() < 0.7,
                                          None if r.random() < 0.5 else "loc", "specs-a" if r.random() < 0.5 else "specs-b",
                                          [None, now - 500, now - 2 * G][int(r.integers(0, 3))], [None, None, None, 0, 7][int(r.integers(0, 5))]))
        for i in range(4):
            discovery.append(DSM.sighting("n%05d" % i, ip(int(r.integers(0, 8))), 8080, True, r.random() < 0.8, True))
        want, want_status, _, _, abi, _ = DSM.run_sequential(store, discovery, now, 2)
        rows = np.array(abi["rows"], dtype=E.disc_row_dt)
        for e in self.full:
            out, total = e.discovery_sync(now, abi["row_endpoint"], abi["n_endpoints"], 2, rows, apply=False)
            self.same(k, "discovery sync", disc_dicts(out), want, "result")
            if total != sum(len(x["updates"]) for x in want):
                raise AssertionError(self.where(k, "discovery sync", f"{total} updates"))
        self.live.status = list(want_status)                             # (the sync writes the ledger's statuses, not its counters)
        self.cov["discoveries"] += 1
        self.cov["disc_updates"] += sum(len(x["updates"]) for x in want)

    # ------------------------------------------------------------------------------------------------------------ the tick
    def tick(self, k, engines=None):
        """every engine ticks; the oracle ticks; the soak's comparison, then the ledgers' -> the engines' statistics"""
        s = self.s
        stats = [e.tick() for e in s.engines]
        for e in self.full:
            e.feed.publish(e.table())
        tasks, want, events = s.oracle_tick()
        for e, st in zip(s.engines, stats):
            s.compare(e, k, tasks, want, events, st)
            s.check_bounds(e, k)
        self.after_tick(k, want)
        for e in self.full:
            self.check(e, k)
        return stats

    def after_tick(self, k, want):
        """what the models and the coverage take from the tick's groups"""
        s, c = self.s, self.cov
        uid = s.uid
        n_claimed = members = 0
        for _gid, cfg, mem, t in want:
            c["configs_in_use"].add(cfg)
            members += len(mem)
            if t < 0:
                continue
            n_claimed += 1
            u = int(uid[t])
            for w in mem:
                if self.cur_uid.get(w) != u:
                    if w in self.cur_uid:
                        self.old_uid[w] = self.cur_uid[w]
                    self.cur_uid[w] = u
        keys, T, G = len(self.ro.rows) + n_claimed, len(s.tasks), len(want)
        L = self._last
        if L["keys"] is not None and (L["keys"] <= RO_CHUNK) != (keys <= RO_CHUNK):
            c["key_crossings"] += 1
        if (L["T"] <= 1024) != (T <= 1024):
            c["T_crossings"] += 1
        if L["groups"] is not None and (L["groups"] <= 256) != (G <= 256):
            c["group_crossings"] += 1
        L.update(keys=keys, T=T, groups=G)
        c["max_keys"], c["min_keys"] = max(c["max_keys"], keys), min(c["min_keys"], keys)
        c["T_min"], c["T_max"] = min(c["T_min"], T), max(c["T_max"], T)
        c["groups_min"], c["groups_max"] = min(c["groups_min"], G), max(c["groups_max"], G)
        c["members_plus_groups_max"] = max(c["members_plus_groups_max"], members + G)
        if k % 3 == 0:
            r = k // 3
            for qs, name, n in ((self.nq, "node_orders", 2), (self.gq, "group_orders", 2), (self.tq, "task_orders", 2)):
                for j in range(n):
                    o = qs[(n * r + j) % len(qs)]["order"]
                    c[name][o] = c[name].get(o, 0) + 1
            c["rollout_reads"] += 1
        if k % 12 == 0:                                                  # (drawn here: the schedule is the same without an engine)
            self.near_queries = [(E.NEAR_SEED if i % 4 == 0 else int(self.r.integers(0, s.W)), int(self.r.integers(0, self.C)))
                                 for i in range(8)]
            c["report_reads"] += 1

    def ledger_rows(self):
        return self.ro.get(range(self.s.W))

    def check(self, e, k):
        s = self.s
        W = s.W
        want, group_of = self.groups()
        # ---- the ledgers, on every tick
        st, cnt = e.liveness_get()
        self.same(k, "liveness statuses", st.tolist(), self.live.status)
        self.same(k, "liveness counters", cnt.tolist(), self.live.counter)
        self.check_transitions(e, k)
        uid, state = e.rollout_get()
        ledger = self.ledger_rows()
        self.same(k, "rollout ledger", list(zip(uid.tolist(), state.tolist())), ledger)
        self.check_metrics(e, k, want, group_of)
        self.check_feed(e, k, *e.drain_assignment_changes())
        ranks = self.check_addresses(e, k)
        # ---- the rollout reads and the directories, on every third tick
        if k % 3 == 0:
            by_rank = ranks if ranks is not None else s.packed["addr_rank"][:W].tolist()   # (no book ranks yet: the swarm's stand)
            task_uids = [int(u) for u in s.uid]
            reads, model = rollout_reads(e), RM.read(W, group_of, want, task_uids, self.ro)
            for name in ("summary", "tasks", "groups", "workers"):
                if name == "summary":
                    if reads[name] != model[name]:
                        raise AssertionError(self.where(k, "rollout summary", f"{reads[name]} vs the model's {model[name]}"))
                else:
                    self.same(k, f"rollout {name}", reads[name], model[name])
            self.check_directories(e, k, want, group_of, task_uids, ledger, by_rank)
        if ranks is not None:
            e.set_addr_ranks(s.packed["addr_rank"][:W])                  # the swarm's order again, for the tick
        if k % 12 == 0:
            self.check_reports(e, k, want, group_of)

    def check_metrics(self, e, k, want, group_of):
        got = e.metrics_rows()
        assert not got["_pad"].any()
        rows = [(int(a), int(b), MM.bits(float(c))) for a, b, c in zip(got["row"], got["series"], got["value"])]
        self.same(k, "metrics rows", rows, [(r, x, MM.bits(v)) for r, x, v in self.mx.listing()], "entry")
        for i, (row, gid, cfg) in enumerate(zip(got["row"].tolist(), got["group_id"].tolist(), got["config"].tolist())):
            g = want[group_of[row]] if row != MM.MANUAL and group_of[row] >= 0 else None
            if (gid, cfg) != ((MM.NONE, 0) if g is None else (g[0], g[1])):
                raise AssertionError(self.where(k, "metrics rows", f"entry {i}, row {row}: group {gid:#x}, config {cfg}"))
        sums, counts = e.metrics_totals()
        ws, wc = self.mx.totals()
        self.same(k, "metrics counts", counts.tolist(), wc, "series")
        for i, (x, y) in enumerate(zip(sums.tolist(), ws)):
            if not ((math.isnan(x) and math.isnan(y)) or MM.bits(x) == MM.bits(y)):
                raise AssertionError(self.where(k, "metrics totals", f"series {i}: {x!r} vs the model's {y!r}"))

    def check_feed(self, e, k, workers, what, resync):
        want, want_resync = e.feed.drain()
        if resync != want_resync:
            raise AssertionError(self.where(k, "change feed", f"resync {resync}, the model's {want_resync}"))
        self.same(k, "change feed", list(zip(workers.tolist(), what.tolist())), want)

    def check_addresses(self, e, k):
        """texts and ranks against the model -> the ranks the book installed (None while a row holds no address)"""
        W = self.s.W
        held = sorted(self.addr)
        if len(held) < W:
            if code_of(e.rank_addresses) != ESTATE:
                raise AssertionError(self.where(k, "address ranks", "ranked although a row holds no address"))
            self.same(k, "address texts", e.address_texts(held), [self.text[w] for w in held])
            return None
        texts = [self.text[w] for w in range(W)]
        self.same(k, "address texts", e.address_texts(), texts)
        ranks = AM.ranks_of_texts(texts)
        self.same(k, "address ranks", e.rank_addresses().tolist(), ranks)
        return ranks

    def check_directories(self, e, k, want, group_of, task_uids, ledger, ranks):
        s = self.s
        r = k // 3
        gof = group_of.tolist()
        for j in range(2):
            q = self.nq[(2 * r + j) % len(self.nq)]
            got = node_read(e, q)
            model = DM.directory(self.live.status, self.live.counter, gof, want, task_uids, ledger, ranks, q)
            if got[0] != model[0] or got[1] != model[1]:
                raise AssertionError(self.where(k, "node directory", f"{q}: total {got[0]}, counts {got[1]} vs the model's {model[0]}, {model[1]}"))
            self.same(k, f"node directory {q}", got[2], model[2])
        for j in range(2):
            q = self.gq[(2 * r + j) % len(self.gq)]
            got = group_read(e, q)
            model = GM.directory(want, self.live.status, ledger, ranks, task_uids, self.C, q)
            if got[0] != model[0] or got[1] != model[1]:
                raise AssertionError(self.where(k, "group directory", f"{q}: totals {got[0]}, {got[1]} vs the model's {model[0]}, {model[1]}"))
            self.same(k, f"group directory {q}", got[2], model[2])
            self.same(k, f"group directory {q} members", got[3], model[3], "member")
        tasks = list(zip(task_uids, [int(x) for x in s.created], [int(x) for x in s.masks]))
        full = None
        for j in range(-1, 3):                                           # (first the counters alone: ONE call, on whatever the last read left)
            q = TM.query(limit=0) if j < 0 else self.tq[(2 * r + j) % len(self.tq)] if j < 2 else TM.query()
            got = task_read(e, q)
            model = TM.directory(want, ledger, tasks, self.C, q)
            if got[0] != model[0] or got[1] != model[1]:
                raise AssertionError(self.where(k, "task directory", f"{q}: totals {got[0]}, {got[1]} vs the model's {model[0]}, {model[1]}"))
            self.same(k, f"task directory {q}", got[2], model[2])
            full = got
        self.cross(e, k, full)

    def cross(self, e, k, full):
        """_cross of tests/test_gpu_taskdir.py: the unfiltered list against pm_task_report, pm_rollout_tasks, pm_config_report"""
        totals, by_config, rows = full
        running, workers, allowed = e.task_report()
        self.same(k, "task directory vs pm_task_report: groups running", [x[5] for x in rows], running.tolist())
        self.same(k, "task directory vs pm_task_report: workers running", [x[6] for x in rows], workers.tolist())
        self.same(k, "task directory vs pm_task_report: groups allowed", [x[4] for x in rows], allowed.tolist())
        self.same(k, "task directory: positions", [x[3] for x in rows], list(range(len(rows))))
        self.same(k, "task directory vs pm_config_report: tasks allowing", by_config, e.config_report()["tasks_allowing"].tolist(), "config")
        rt = e.rollout_tasks()
        by_task = {int(x["task"]): x for x in rt if int(x["task"]) != NONE}
        got, model = [], []
        for x in rows:
            y = by_task.get(x[3])
            got.append(x[7:10])
            model.append((int(y["groups_converged"]), int(y["converged"]), tuple(y["reporters"].tolist())) if y is not None else (0, 0, (0,) * 8))
        self.same(k, "task directory vs pm_rollout_tasks", got, model)
        lost = [x for x in rt if int(x["task"]) == NONE]
        if totals[7:9] != (len(lost), sum(int(x["reporters"].sum()) for x in lost)):
            raise AssertionError(self.where(k, "task directory vs pm_rollout_tasks", f"orphans {totals[7:9]}"))

    def check_reports(self, e, k, want, group_of):
        """the spread report, the nearest-candidates query and the configuration report, each as its own test file compares it"""
        s = self.s
        W, P = s.W, s.packed
        flags, lat, lon = P["flags"][:W], P["lat"][:W], P["lon"][:W]
        rank = P["addr_rank"][:W]
        got = e.group_spread()
        model = [SM.group_spread(g[2], flags, lat, lon, rank) for g in want]
        try:
            SM.check_rows(got, model, lat, lon, None, "")
        except AssertionError as err:
            raise AssertionError(self.where(k, "spread report", str(err.args[0] if err.args else err)))
        if not np.array_equal(e.config_spread(), SM.config_spread(got, [g[1] for g in want], self.C)):
            raise AssertionError(self.where(k, "spread report", "the per-configuration rows are not the sum of the per-group rows"))
        compat = orc.compat_masks(s.st.nodes[:W], self.cfgs)
        pool = E.NEAR_IDLE if (k // 12) % 2 else E.NEAR_ELIGIBLE
        queries = self.near_queries
        rows, workers, km = e.nearest_workers(queries, pool, 16)
        for i, (o, c) in enumerate(queries):
            m = NM.nearest(o, c, pool, 16, compat, flags, group_of, lat, lon)
            tag = self.where(k, "nearest workers", f"query {i} ({o}, {c}) pool {pool}")
            row = tuple(int(rows[i][f]) for f in ("origin", "n", "candidates", "located"))
            if row != (m["origin"], m["n"], m["candidates"], m["located"]):
                raise AssertionError(f"{tag}: {row} vs the model's {(m['origin'], m['n'], m['candidates'], m['located'])}")
            far = [x for x in m["key"][:m["n"]] if x != NM.F64_MAX and x > SM.KM_AT_A_0_999]
            if far:                                                  # (spread_model.check_rows' rule: the kilometres' tolerance
                continue                                             # is derived up to a = 0.999; the counts above are not)
            try:
                NM.check_query(rows[i], workers[i], km[i], m, False, tag)
            except AssertionError as err:
                raise AssertionError(f"{tag}: {err.args}")
        why = RPM.why_codes(rows_of(P, np.arange(W)), *self.cfg_pack)
        enabled = s.enabled_mask & ~(1 << s.disabled[0]) if s.disabled else s.enabled_mask
        model = RPM.config_report(why, flags, group_of, enabled, [(g[1], len(g[2]), g[3]) for g in want], s.masks)
        rep = e.config_report()
        for c in range(self.C):
            if rep[c] != model[c]:
                raise AssertionError(self.where(k, "configuration report", f"configuration {c}: {rep[c]} vs the model's {model[c]}"))

    # ------------------------------------------------------------------------------------------------------------ epilogue
    def epilogue(self):
        """no oracle: a shorter table without keep_groups, 300 rows appended, and a table of the same length without keep_groups;
        after each upload every ledger reads as freshly initialised, after the append as the models say"""
        s, r = self.s, self.r
        k = self.ticks
        P = s.packed
        W = s.W - 100
        cols = rows_of(P, np.arange(W))
        self.each(lambda e: e.upload_workers(cols))
        self._fresh(W, cols["flags"])
        for e in self.full:
            self.check_fresh(e, k, W, cols, "a shorter table")
        # ---- 300 rows behind it (copies of the first 300: only the ledgers are looked at), something in every ledger
        more = rows_of(P, np.arange(300))
        self.each(lambda e: e.append_workers(more))
        cols = {key: np.concatenate([cols[key], more[key]]) for key in cols}
        W += 300
        self.live.append(more["flags"])
        some = r.choice(W, size=40, replace=False)
        st = r.integers(0, LM.N_STATUS, size=40).astype(np.uint8)
        self.live.set(some, st)
        self.each(lambda e: e.liveness_set(some, st))
        self.now += STEP_MS
        beats = np.where(r.random(W) < 0.5, self.now - 5, 0).astype(np.uint64)
        self.listed, census = self.live.sweep(self.now, beats, None)
        for w, _, new, _ in self.listed:
            if new == LM.DEAD:
                self.mx.clear_row(w)
        for e in self.full:
            n, got = e.liveness_sweep(self.now, beats, None)
            if n != len(self.listed) or got.tolist() != census:
                raise AssertionError(self.where(k, "epilogue: liveness sweep", f"{n} rows, census {got.tolist()}"))
        mb = [(int(w), MM.MERGE, 2 * i, 2) for i, w in enumerate(r.choice(W, size=50, replace=False))]
        me = [(int(x), 0, float(x)) for x in r.integers(0, 20, size=100)]
        self.mx.ingest(mb, me, 20)
        self.each(lambda e: e.metrics_ingest(np.array(mb, dtype=E.mx_beat_dt), np.array(me, dtype=E.mx_entry_dt), 20))
        reps = [(int(w), int(r.integers(0, RM.TS_N)), int(s.uid[int(r.integers(0, len(s.uid)))])) for w in r.choice(W, size=200, replace=False)]
        self.ro.ingest(reps)
        out = np.zeros(len(reps), dtype=E.ro_report_dt)
        for i, rep in enumerate(reps):
            out[i] = rep
        self.each(lambda e: e.rollout_ingest(out))
        for w in range(W):
            self._model_address(w, self._fresh_address())
        self._set_addresses(range(W))
        self.s.W = W                                                     # (the checks below read the models over this table)
        for e in self.full:
            self.check_table(e, k, W, cols, "300 rows appended")
        # ---- the same length, the groups dropped: only the flag of the upload can tell the ledgers
        self.each(lambda e: e.upload_workers(cols))
        self._fresh(W, cols["flags"])
        for e in self.full:
            self.check_fresh(e, k, W, cols, "a table of the same length")
        self.events["epilogue"] = k

    def _fresh(self, W, flags):
        self.live = LM.Ledger(flags, self.m)
        self.listed = []
        self.mx.clear_workers()
        self.ro.clear()
        self.addr, self.text = {}, {}
        self.s.W = W
        self.s.last_want = []

    def check_fresh(self, e, k, W, cols, tag):
        tag = f"epilogue, {tag}"
        for call in (e.rank_addresses, lambda: e.address_texts([0])):
            if code_of(call) != ESTATE:
                raise AssertionError(self.where(k, tag, "the address book still holds an address"))
        if any(self.ro.rows) or any(r != MM.MANUAL for r in self.mx.rows):
            raise AssertionError(self.where(k, tag, "the models are not fresh"))
        self.check_table(e, k, W, cols, tag, book=False)
        total, _, _ = e.group_directory(limit=0)[0]["total"], None, None
        if total or len(e.liveness_transitions()):
            raise AssertionError(self.where(k, tag, f"{total} groups listed, {len(e.liveness_transitions())} transitions"))

    def check_table(self, e, k, W, cols, tag, book=True):
        """every ledger and every directory against the models, over a table that holds no group"""
        st, cnt = e.liveness_get()
        self.same(k, f"{tag}: liveness statuses", st.tolist(), self.live.status)
        self.same(k, f"{tag}: liveness counters", cnt.tolist(), self.live.counter)
        self.check_transitions(e, k)
        uid, state = e.rollout_get()
        ledger = self.ro.get(range(W))
        self.same(k, f"{tag}: rollout ledger", list(zip(uid.tolist(), state.tolist())), ledger)
        group_of = np.full(W, -1, dtype=np.int64)
        self.check_metrics(e, k, [], group_of)
        ranks = [int(x) for x in cols["addr_rank"]]
        if book:
            ranks = self.check_addresses(e, k)
        task_uids = [int(u) for u in self.s.uid]
        reads, model = rollout_reads(e), RM.read(W, group_of, [], task_uids, self.ro)
        for name in ("tasks", "groups", "workers"):
            self.same(k, f"{tag}: rollout {name}", reads[name], model[name])
        if reads["summary"] != model["summary"]:
            raise AssertionError(self.where(k, f"{tag}: rollout summary", f"{reads['summary']} vs the model's {model['summary']}"))
        tasks = list(zip(task_uids, [int(x) for x in self.s.created], [int(x) for x in self.s.masks]))
        for q in self.nq[::5]:
            got, m = node_read(e, q), DM.directory(self.live.status, self.live.counter, group_of.tolist(), [], task_uids, ledger, ranks, q)
            self.same(k, f"{tag}: node directory {q}", [got[0], got[1]] + got[2], [m[0], m[1]] + m[2])
        for q in self.gq[::7]:
            got, m = group_read(e, q), GM.directory([], self.live.status, ledger, ranks, task_uids, self.C, q)
            self.same(k, f"{tag}: group directory {q}", list(got), list(m), "part")
        for q in self.tq[::4]:
            got, m = task_read(e, q), TM.directory([], ledger, tasks, self.C, q)
            self.same(k, f"{tag}: task directory {q}", [got[0], got[1]] + got[2], [m[0], m[1]] + m[2])
