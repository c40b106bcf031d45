"""What an engine holds from the HIP runtime is its members' to give back (protocol_amd/csrc/pm_owned.h): an engine that has
used every ledger and every report returns the process to the allocation counts it found, two engines do not share anything,
and a ledger switched off and on again costs nothing that stays and reads as a fresh one.  The counts are
pm_debug_live_allocations: device bytes, pinned host bytes, events + streams.

192 workers are three bitmap words: the ledgers' lists have more than one word."""
import gc

import numpy as np
import pytest

from protocol_amd import engine as E
from protocol_amd import host

pytestmark = pytest.mark.gpu
W, NOW = 192, 10_000_000
ON = E.W_HEALTHY | E.W_HAS_P2P | E.W_HAS_LOC
CONFIGS = [("pairs", 1, 2, None), ("quads", 2, 4, None)]
ALL = np.arange(W, dtype=np.uint32)


def live():
    gc.collect()  # (an engine some earlier test dropped without closing goes now, not between two readings)
    return E.Engine.debug_live_allocations()


def make_engine():
    """192 located workers, 2 requirement-free configurations, 3 tasks"""
    eng = E.Engine(group_id_seed=5)
    cfg_rows, alt_rows, _ = host.pack_configs(CONFIGS)
    eng.set_configs(cfg_rows, alt_rows)
    z = np.zeros(W, dtype=np.uint32)
    eng.upload_workers(dict(flags=np.full(W, ON, dtype=np.uint32), gpu_count=z, gpu_mem_mb=z, gpu_model_class=z, cpu_cores=z,
                            ram_mb=z, storage_gb=z, price=z, lat=30.0 + 0.1 * (ALL % 16), lon=-100.0 + 0.1 * (ALL // 16)))
    eng.upload_tasks(np.array([1, 2, 3], dtype=np.uint64), np.array([30, 20, 10], dtype=np.int64),
                     np.array([101, 102, 103], dtype=np.uint64))
    return eng


def table(eng):
    out = []
    for w in range(W):
        a = eng.lookup(w)
        out.append((a.task, a.group_slot, a.group_index, a.group_size, a.next_worker, a.group_id))
    return out


def all_healthy(eng):
    """(host only) every row as it was uploaded: what an applying sweep or sync took away comes back"""
    eng.on_worker_status_many(ALL, np.full(W, ON, dtype=np.uint32), np.zeros(W, dtype=np.uint32))


# ---- one use of each ledger; each returns something that shows the call did its work

def use_changes(eng):
    eng.tick()
    workers, what, resync = eng.drain_assignment_changes()
    return len(workers), resync


def use_liveness(eng):
    n, census = eng.liveness_sweep(NOW, np.zeros(W, dtype=np.uint64), apply=True)  # (nobody has ever beaten)
    assert n == len(eng.liveness_transitions()) and int(census.sum()) == W
    return n


def use_discovery(eng):
    ep = (ALL % 5).astype(np.uint32)
    rows = [(w, ep[w], ep[w], 7, 0, 0) for w in (0, 64, 191)] + [(E.DISC_NEW, 4, 0, 7, 0, 0)]
    out, total = eng.discovery_sync(NOW, ep, 5, 1, np.array(rows, dtype=E.disc_row_dt), apply=True)
    return len(out)


def use_metrics(eng):
    beats = np.array([(E.MX_MANUAL, E.MXB_MERGE, 4, 1), (0, E.MXB_MERGE, 0, 2), (64, E.MXB_REPLACE, 2, 1), (191, E.MXB_MERGE, 3, 1)],
                     dtype=E.mx_beat_dt)
    entries = np.array([(0, 0, 1.5), (7, 0, 2.5), (3, 0, -1.0), (7, 1, 4.0), (2, 0, 8.0)], dtype=E.mx_entry_dt)
    eng.metrics_ingest(beats, entries, 8)
    s, c = eng.metrics_totals()
    assert c.tolist() == [1, 0, 1, 1, 0, 0, 0, 2] and s[7] == 6.5
    assert len(eng.metrics_rows()) == 5 and len(eng.metrics_rows([64, E.MX_MANUAL])) == 2
    return 5


def use_reports(eng):
    assert len(eng.group_spread()) > 0 and len(eng.config_spread()) == len(CONFIGS)
    rows, workers, km = eng.nearest_workers([(0, 0), (E.NEAR_SEED, 1), (191, 1)], pool=E.NEAR_ELIGIBLE, k=4)
    assert len(rows) == 3
    cfg_rows, alt_rows, bits, n_rows, n_cls = host.pack_probes([("probe", 1, 3, None)], [])
    prows, overlap, mask = eng.probe_configs(cfg_rows, alt_rows, bits, n_rows, n_cls)
    assert len(prows) == 1 and eng.config_overlap().shape == (2, 2)
    why, state = eng.explain_workers()
    assert why.shape == (W, 2) and len(eng.config_report()) == 2 and len(eng.task_report()[0]) == 3


def test_an_engine_gives_back_everything_it_took():
    base = live()
    for k in range(5):
        eng = make_engine()
        eng.enable_assignment_changes()
        eng.liveness_enable(True, 1)
        eng.metrics_enable(True)
        st = eng.tick()
        assert st["n_groups"] > 0
        assert use_liveness(eng) == W  # (Healthy and never beaten: every row is listed)
        assert use_discovery(eng) == 4
        all_healthy(eng)
        use_metrics(eng)
        n, resync = use_changes(eng)
        assert n == W and resync
        use_reports(eng)
        used = E.Engine.debug_live_allocations()
        print(f"round {k}: base {base}, in use {used}")
        assert all(u > b for u, b in zip(used, base)), (used, base)
        eng.close()
        assert live() == base, k


def test_two_engines_share_nothing():
    base = live()
    alone = make_engine()  # what an engine left alone publishes after one tick, and after two
    alone.tick()
    want1 = table(alone)
    alone.tick()
    want2 = table(alone)
    alone.close()
    assert live() == base
    a, b = make_engine(), make_engine()
    for eng in (a, b):
        eng.enable_assignment_changes()
        eng.liveness_enable(True, 1)
        eng.metrics_enable(True)
        eng.tick()
    assert table(a) == want1 and table(b) == want1 and any(r[0] != E.PM_NONE for r in want1)
    both = live()
    a.close()
    one = live()
    assert all(base[k] < one[k] < both[k] for k in range(3)), (base, one, both)
    assert table(b) == want1  # (the published rows are pinned memory of b's own)
    b.tick()
    assert table(b) == want2
    assert use_liveness(b) > 0
    use_metrics(b)
    b.close()
    assert live() == base


def _cycle(eng, which):
    """enable, use, disable"""
    all_healthy(eng)
    if which == "changes":
        eng.enable_assignment_changes(True)
        assert use_changes(eng) == (W, True)
        eng.enable_assignment_changes(False)
    elif which == "liveness":
        eng.liveness_enable(True, 1)
        assert use_liveness(eng) > 0
        eng.liveness_enable(False)
    elif which == "discovery":  # (its scratch lives and goes with the liveness ledger)
        eng.liveness_enable(True, 1)
        assert use_discovery(eng) == 4
        eng.liveness_enable(False)
    else:
        eng.metrics_enable(True)
        use_metrics(eng)
        eng.metrics_enable(False)


@pytest.mark.parametrize("which", ["changes", "liveness", "discovery", "metrics"])
def test_a_ledger_switched_off_leaves_nothing(which):
    base = live()
    eng = make_engine()
    for _ in range(3):
        eng.tick()
    _cycle(eng, which)  # (a warm-up: an applying path may grow the engine's ordinary staging the first time)
    before = live()
    _cycle(eng, which)
    after = live()
    print(f"{which}: base {base}, off {before}, off again {after}")
    assert after == before
    # on again it reads as a fresh one
    all_healthy(eng)
    if which == "changes":
        eng.enable_assignment_changes(True)
        workers, what, resync = eng.drain_assignment_changes()
        assert len(workers) == 0 and not resync  # (nothing until the next publish)
        assert use_changes(eng) == (W, True)
    elif which in ("liveness", "discovery"):
        eng.liveness_enable(True, 1)
        s, c = eng.liveness_get()
        assert (s == E.NS_HEALTHY).all() and not c.any() and len(eng.liveness_transitions()) == 0
    else:
        eng.metrics_enable(True)
        s, c = eng.metrics_totals()
        assert len(s) == 0 and len(c) == 0 and len(eng.metrics_rows()) == 0
    eng.close()
    assert live() == base
