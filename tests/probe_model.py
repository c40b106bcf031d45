"""numpy restatement of the probe calls (include/pm_engine.h, pm_probe_configs / pm_config_overlap), on the engine's own packed
columns.  The clause code and the worker states are report_model's (imported, not copied).

  probe         (rows: probe_row_dt [P], overlap: uint32 [P, C], mask: uint64 [W]) of a probe table against an installed one
  config_overlap  uint32 [C, C]: the installed table on both sides
"""
import numpy as np

from protocol_amd import engine as E

from report_model import why_codes, worker_state


def meets_bits(why) -> np.ndarray:
    """uint64 [W]: bit c = the pair's code is PM_WHY_OK (the orientation of pm_compat_masks)"""
    W, C = why.shape
    out = np.zeros(W, dtype=np.uint64)
    for c in range(C):
        out |= (why[:, c] == 0).astype(np.uint64) << np.uint64(c)
    return out


def probe_from_codes(why_p, why_c, flags, group_of, enabled: int, min_sizes):
    """why_p [W, P] / why_c [W, C]: the codes against the probes / the installed configurations"""
    W, P = why_p.shape
    C = why_c.shape[1]
    f = np.asarray(flags).astype(np.uint32)
    idle = worker_state(f, group_of) == E.WS_IDLE
    elig = ((f & E.W_HEALTHY) != 0) & ((f & E.W_HAS_P2P) != 0)  # grouped or not
    located = (f & E.W_HAS_LOC) != 0
    meets_p = why_p == 0
    meets_c = why_c == 0
    en = np.array([(int(enabled) >> c) & 1 for c in range(C)], dtype=bool)
    meets_enabled = (meets_c & en[None, :]).any(axis=1) if C else np.zeros(W, dtype=bool)
    rows = np.zeros(P, dtype=E.probe_row_dt)
    for p in range(P):
        r = rows[p]
        counts = np.bincount(why_p[elig, p], minlength=10)[:10]
        r["why"] = counts
        r["eligible_meets"] = counts[0]
        mine = idle & meets_p[:, p]
        r["idle_meets"] = int(mine.sum())
        r["idle_located"] = int((mine & located).sum())
        r["idle_exclusive"] = int((mine & ~meets_enabled).sum())
        r["groups_max"] = int(r["idle_meets"]) // int(min_sizes[p])
        r["groups_exclusive"] = int(r["idle_exclusive"]) // int(min_sizes[p])
    overlap = (meets_p[idle].astype(np.int64).T @ meets_c[idle].astype(np.int64)).astype(np.uint32).reshape(P, C)
    return rows, overlap, meets_bits(why_p)


def probe(workers: dict, group_of, enabled: int, installed, probes, n_classes: int):
    """installed / probes: (cfg_rows, alt_rows, model bits) each, over the same n_classes spec models"""
    why_c = why_codes(workers, installed[0], installed[1], installed[2], n_classes)
    why_p = why_codes(workers, probes[0], probes[1], probes[2], n_classes)
    return probe_from_codes(why_p, why_c, workers["flags"], group_of, enabled, [int(r["min_group_size"]) for r in probes[0]])


def config_overlap(workers: dict, group_of, installed, n_classes: int) -> np.ndarray:
    why_c = why_codes(workers, installed[0], installed[1], installed[2], n_classes)
    idle = worker_state(workers["flags"], group_of) == E.WS_IDLE
    m = (why_c == 0)[idle].astype(np.int64)
    return (m.T @ m).astype(np.uint32)
