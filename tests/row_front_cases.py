"""Swarms for tests/test_gpu_row_front.py: every worker eligible (Healthy, p2p id known), locations and configurations
laid out so that the rows of late seeds are — without the rule "no located candidate in front of the seed" — mostly
made of candidates that are in a group by the seed's turn."""
import numpy as np

from oracle import oracle_ffi as orc
from protocol_amd.swarm import ST_HEALTHY, make_swarm


def _base(seed, W, configs):
    sw = make_swarm(seed, 0, W)
    sw.status[:] = ST_HEALTHY
    sw.has_p2p[:] = True
    sw.configs = list(configs)
    rng = np.random.default_rng(seed)
    # scattered, no two at one site: distinct latitudes on the 0.0001-degree grid
    lat = 25.0 + rng.permutation(350000)[:W] * 1e-4
    sw.lat[:] = np.round(lat, 4)
    sw.lon[:] = np.round(rng.uniform(-125.0, 40.0, W), 4)
    sw.has_loc[:] = True
    return sw, rng


def all_at_once(seed=11):
    """(a) 1,500 located workers, one configuration (2, 8): every seed gets its ticket at once, a late seed's row is made
    while nearly everything in front of it is still free"""
    return _base(seed, 1500, [("c0", 2, 8, None)])[0]


def windowed(seed=12):
    """(b) 2,400 located workers, the same configuration: two look-ahead windows"""
    return _base(seed, 2400, [("c0", 2, 8, None)])[0]


def unlocated_in_front(seed=13):
    """(c) 600 workers, every second one without a location; the first configuration (2, 8) takes the workers with eight
    GPUs, whose located count is no multiple of 8 — its last located group is filled with location-less workers from
    positions in front of its seed; a second configuration (2, 5) takes what is left"""
    sw, _rng = _base(seed, 600, [("c0", 2, 8, "gpu:count=8"), ("c1", 2, 5, None)])
    nodes, cfgs, _t, _e = orc.from_swarm(sw)
    comp0 = (orc.compat_masks(nodes, cfgs) & np.uint64(1)) != 0
    for part in (np.nonzero(comp0)[0], np.nonzero(~comp0)[0]):
        sw.has_loc[part[1::2]] = False
    n_loc = int((comp0 & sw.has_loc).sum())
    if n_loc % 8 == 0:  # one located worker fewer
        sw.has_loc[np.nonzero(comp0 & sw.has_loc)[0][-1]] = False
    return sw


def cities(seed=14):
    """(d) 5 shared sites of 60 workers each among 900 scattered ones, one configuration (2, 9)"""
    sw, rng = _base(seed, 1200, [("c0", 2, 9, None)])
    at = rng.permutation(1200)[:300]
    s_lat, s_lon = np.round(rng.uniform(25.0, 60.0, 5), 4) + 0.00005, np.round(rng.uniform(-125.0, 40.0, 5), 4)
    sw.lat[at] = s_lat[np.arange(300) % 5]  # (off the scattered workers' grid: a site holds its 60 and nobody else)
    sw.lon[at] = s_lon[np.arange(300) % 5]
    return sw


def walk(n):
    """(e) n located workers (the smallest eligible count with a spatial index), one configuration (2, 8)"""
    return _base(15, n, [("c0", 2, 8, None)])[0]


def enabled_all(sw):
    return (1 << len(sw.configs)) - 1
