"""The schedule of tests/test_gpu_ledger_soak.py run against the CPU oracle and the ledgers' models alone, in both shapes: what
it exercises does not depend on the GPU, so its coverage is asserted here — the sizes an engine's life walks across (a radix
chunk of rows, of tasks and of rollout keys, a block of groups), the couplings (metrics rows a sweep empties, reports of rows
appended in the same interval, ten-character ties in the address book), every life event, every directory order.  An edit of
tests/soak.py or tests/ledger_soak.py that empties the GPU test fails here.

The bounds are those of a run at seed 1 and 240 ticks; they hold only there, as the GPU test's do."""
import time

import pytest

import directory_model as DM
import groupdir_model as GM
import taskdir_model as TM
from ledger_soak import RO_CHUNK, LedgerSoak
from soak import env_int

TICKS, SEED = 240, 1


def covered(ls, shape):
    """the coverage assertions of a run of the default length at the default seed (the GPU test asserts them too)"""
    c, sc, ticks = ls.cov, ls.s.cov, ls.ticks
    msg = (shape, {k: v for k, v in c.items()}, sc)
    if shape == "small":
        assert c["W_max"] == 1500 and ls.first_W_above[1024] is not None and 20 <= ls.first_W_above[1024] <= 40, msg
        assert c["T_crossings"] > 40 and c["T_min"] < 1024 - 40 and c["T_max"] > 1024 + 20, msg
        assert c["members_plus_groups_max"] > RO_CHUNK, msg
        assert c["key_crossings"] >= 4 and c["min_keys"] < RO_CHUNK < c["max_keys"], msg
        assert sc["resyncs"] == 1 and sc["mask_toggles"] == 1, msg
        assert len(c["configs_in_use"]) >= 13, msg
    else:
        assert c["W_max"] == 2100 and ls.first_W_above[2048] is not None, msg
        assert c["group_crossings"] >= 4 and c["groups_min"] < 256 - 40 and c["groups_max"] > 256, msg
    assert c["emptied_by_sweep"] >= ticks, msg
    assert c["same_interval_reports"] >= 20, msg
    assert c["ties"] >= 5, msg
    assert c["old_claim_reports"] >= ticks and c["stranger_reports"] >= ticks and c["twice_reports"] >= ticks and c["clears"] >= ticks, msg
    assert c["discoveries"] == ticks // 8 and c["disc_updates"] >= ticks // 8, msg
    assert ls.events["rollout_enable"] == ticks // 3 and ls.events["metrics_enable"] == ticks // 2, msg
    assert ls.events["liveness_enable"] == (2 * ticks) // 3 and ls.events["resync"] == 200 and ls.events["masked"] == 150, msg
    assert "epilogue" in ls.events, msg
    for name, orders in (("node_orders", (DM.BY_ROW, DM.BY_ADDRESS)), ("group_orders", (GM.BY_SLOT, GM.BY_ID_TEXT, GM.BY_SIZE_DESC)),
                         ("task_orders", (TM.BY_LIST, TM.BY_OLDEST, TM.BY_WORKERS_DESC, TM.BY_REPORTERS_DESC))):
        assert all(c[name].get(o, 0) >= 5 for o in orders), msg
    assert c["rollout_reads"] == (ticks + 2) // 3 and c["report_reads"] == (ticks + 11) // 12, msg


@pytest.mark.parametrize("shape", ["small", "wide"])
def test_the_ledger_soak_schedule_covers_what_it_is_for(shape):
    ticks, seed = env_int("PM_LEDGER_SOAK_TICKS", TICKS), env_int("PM_SOAK_SEED", SEED)
    ls = LedgerSoak(seed, ticks, shape)
    t0 = time.perf_counter()
    for k in range(ticks):
        ls.interval(k)
        ls.tick(k)
    ls.epilogue()
    took = time.perf_counter() - t0
    print(f"{shape}: {ticks} oracle ticks in {took:.1f} s: {ls.cov}; first W above {ls.first_W_above}; events {ls.events}; soak {ls.s.cov}")
    if (ticks, seed) == (TICKS, SEED):
        covered(ls, shape)
