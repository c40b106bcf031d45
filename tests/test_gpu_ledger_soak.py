"""Every ledger and directory together on one churning engine, against the oracle and the models for 240 ticks
(PM_LEDGER_SOAK_TICKS) of the schedule in tests/ledger_soak.py (PM_SOAK_SEED): the change feed, liveness, the discovery sync,
metrics, rollout, the address book, the three directories, the spread report, the nearest-candidates query and the configuration
report are all on and all fed between the ticks of the soak of tests/soak.py, while rows are appended, die and revive, tasks come
and go in front and anywhere, groups dissolve, the tables are uploaded again and the ledgers are switched off and on.  The
ledgers' own test files keep each of them alone for a few steps; here they catch up from different sizes in the same interval,
read each other while they grow, and share one sort and one pager for hundreds of rounds, at sizes that walk across a radix
chunk of rows, of tasks and of rollout keys and across a block of groups.

Also the same schedule on a bare engine and on one with everything on, side by side: the ledgers leave the tick alone."""
import time

import pytest

from protocol_amd import engine as E
from ledger_soak import LedgerSoak
from soak import GROUP_ID_SEED, engine_groups, env_int
from test_ledger_soak_schedule import SEED, TICKS, covered

pytestmark = pytest.mark.gpu
# pm_stats' counters that are a function of the engine's state.  The others (proposals, fast steps, launches, candidates scanned)
# count how the streaming carve's row makers and its validator met in time and differ between two runs of ONE engine
# (tests/test_gpu_metrics.py test_the_ledger_leaves_the_tick_alone): no statement about the ledgers can be read from them
STATE_COUNTERS = ("n_groups", "n_formed", "n_merged", "carve_steps", "host_resolved_steps", "pair_evals")


@pytest.mark.parametrize("shape", ["small", "wide"])
def test_ledger_soak(shape):
    ticks, seed = env_int("PM_LEDGER_SOAK_TICKS", TICKS), env_int("PM_SOAK_SEED", SEED)
    ls = LedgerSoak(seed, ticks, shape)
    eng = E.Engine(group_id_seed=GROUP_ID_SEED)
    ls.load(eng)
    t0 = time.perf_counter()
    for k in range(ticks):
        ls.interval(k)
        ls.tick(k)
    ls.epilogue()
    print(f"\nledger soak {shape}: {ticks} ticks, seed {seed}, {time.perf_counter() - t0:.1f} s; address sorts {eng.debug_address_sorts()}; "
          f"task space {eng.debug_task_space()}; coverage {ls.cov}; events {ls.events}")
    if (ticks, seed) == (TICKS, SEED):                                      # (what the default schedule is built to reach)
        covered(ls, shape)
        sorts = eng.debug_address_sorts()
        assert sorts["deep"] >= ticks // 2 and sorts["shallow"] >= 5, sorts  # ranks before and behind the first ten-character tie
        assert ls.cov["feed_rebuild_resyncs"] >= 1, ls.cov                  # the task index space was rebuilt under the feed
    eng.close()


def test_ledgers_leave_the_soak_alone():
    """the small shape for 80 ticks on a bare engine and on one with everything on, in one Soak: after every tick the groups,
    every row's lookup and the group events are equal (each equals the oracle's, and the rows are compared with each other),
    and so are the tick's counters that are a function of the engine's state"""
    ticks, seed = 80, env_int("PM_SOAK_SEED", SEED)
    ls = LedgerSoak(seed, ticks, "small")
    bare, full = E.Engine(group_id_seed=GROUP_ID_SEED), E.Engine(group_id_seed=GROUP_ID_SEED)
    ls.s.load(bare)
    ls.load(full)
    other = {"bare": 0, "differ": 0}
    for k in range(ticks):
        ls.interval(k)
        sb, sf = ls.tick(k)                                                 # (Soak.compare: groups, tasks and events are the oracle's)
        a, b = engine_groups(bare), engine_groups(full)
        assert a == b, ls.where(k, "bare and full", f"groups {len(a)} / {len(b)}")
        for w in range(ls.s.W):
            x, y = bare.lookup(w), full.lookup(w)
            assert (x.task, x.group_slot, x.group_index, x.group_size, x.next_worker, x.group_id) == \
                   (y.task, y.group_slot, y.group_index, y.group_size, y.next_worker, y.group_id), ls.where(k, "bare and full", f"row {w}")
        assert {c: sb[c] for c in STATE_COUNTERS} == {c: sf[c] for c in STATE_COUNTERS}, ls.where(k, "bare and full", f"statistics {sb} / {sf}")
        rest = [c for c in sb if not c.startswith("ms_") and c not in STATE_COUNTERS]
        other["differ"] += any(sb[c] != sf[c] for c in rest)
    print(f"\nticks whose timing-dependent counters differ between the two engines: {other['differ']} of {ticks}")
    bare.close(), full.close()
