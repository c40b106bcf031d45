"""The schedule of tests/test_gpu_soak.py run against the CPU oracle alone, for ~300 ticks: what it exercises does not
depend on the GPU, so its coverage is checked here — claimed tasks deleted, dissolutions by id that hit, revivals,
reads between ticks, full re-uploads, a configuration switched off, the floor of standing groups, merges."""
import time

from soak import Soak, env_int


def test_the_soak_schedule_covers_what_it_is_for():
    ticks = env_int("PM_SOAK_SCHEDULE_TICKS", 300)
    s = Soak(env_int("PM_SOAK_SEED", 1), ticks, burst=False)
    t0 = time.perf_counter()
    for k in range(ticks):
        s.interval(k)
        s.oracle_tick()
    c = s.cov
    print(f"{ticks} oracle ticks in {time.perf_counter() - t0:.1f} s: {c}")
    assert c["min_groups"] >= 400, c
    assert c["claimed_deletes"] >= ticks, c
    assert c["dissolve_hits"] >= ticks // 10 and c["dissolve_misses"] >= 1, c
    assert c["revivals"] >= 5 * ticks and c["deaths"] >= 10 * ticks, c
    assert c["appends"] >= 2 * ticks, c
    assert c["read_ticks"] >= ticks // 4 and c["rewrites"] >= ticks // 12, c
    assert c["resyncs"] >= 1 and c["mask_toggles"] >= 1, c
    assert c["merges"] >= 20, c
    assert c["unknown_deletes"] >= 10 and c["twice_deletes"] >= 10 and c["front_deletes"] >= 10, c
    assert c["republishes"] >= ticks // 4, c


def test_the_burst_outgrows_the_task_index_space():
    """the burst phase of the default schedule: the live count passes the room task_capacity_for leaves in front of the
    table (65,536 rows), and comes back down"""
    s = Soak(1, 40, burst=True)
    peak = 0
    for k in range(40):
        s.interval(k)
        peak = max(peak, len(s.tasks))
        s.oracle_tick()
    assert peak > 2000 + 65536, peak
    assert len(s.tasks) < 6000, len(s.tasks)
