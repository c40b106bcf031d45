"""The C++ plugin over the real engine: GpuMatchPlugin's group directory methods through pm_plugin_c.h (pmx_list_groups,
pmx_group_counts, pmx_degraded_groups) on a 300-node swarm behind a tick.  list_groups in id-text order is get_all_groups, page
by page; group_counts is a count over get_all_groups; degraded_groups follows a sweep that makes one member Unhealthy and leaves
the list when the member recovers."""
import ctypes as C

import pytest

from protocol_amd.swarm import make_swarm

from plugin_cxx import PluginCxx, _check, _text, plugin_lib, uuid_of

pytestmark = pytest.mark.gpu
NOW = 1_760_000_000_000
STEP = 15_000
ALL64, TO_END = 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF
HEALTH, ROLLOUT = ("lost", "degraded", "sound"), ("no_task", "converged", "rolling")


def bind(L):
    vp, sz, s, u32, u64 = C.c_void_p, C.c_size_t, C.c_char_p, C.c_uint32, C.c_uint64
    L.pmx_enable_liveness.argtypes = [vp, u32]
    L.pmx_enable_rollout.argtypes = [vp]
    L.pmx_report_task.argtypes = [vp, s, s, s]
    L.pmx_flush_rollout.argtypes = [vp]
    L.pmx_beat.argtypes = [vp, s, u64]
    L.pmx_sweep_statuses.argtypes = [vp, u64, C.POINTER(s), u32, s, sz, C.POINTER(sz)]
    L.pmx_list_groups.argtypes = [vp, u64, u32, u32, u32, u32, u32, u32, u32, u32, s, sz, C.POINTER(sz)]
    L.pmx_group_counts.argtypes = [vp, s, sz, C.POINTER(sz)]
    L.pmx_degraded_groups.argtypes = [vp, s, sz, C.POINTER(sz)]
    return L


def _groups(text):
    """group lines -> [{id, config, size, health, rollout, task, created_at, nodes}]"""
    out = []
    for line in text.splitlines():
        f = line.split("\t")
        out.append(dict(id=f[0], config=f[1], size=int(f[2]), health=f[3], rollout=f[4], task=f[5], created_at=int(f[6]),
                        nodes=f[7].split(",")))
    return out


def list_groups(p, order=1, offset=0, limit=TO_END, config_mask=ALL64, holds=0, size_min=0, size_max=TO_END, health=7, rollout=7):
    text = _text(lambda o, c, n: p.L.pmx_list_groups(p._p, config_mask, holds, size_min, size_max, health, rollout, order, offset,
                                                     limit, o, c, n))
    head, _, rest = text.partition("\n")
    tag, total, members = head.split("\t")
    assert tag == "total"
    return int(total), int(members), _groups(rest)


def degraded(p):
    return _groups(_text(lambda o, c, n: p.L.pmx_degraded_groups(p._p, o, c, n)))


def sweep(p, now):
    arr = (C.c_char_p * 1)()
    return _text(lambda o, c, n: p.L.pmx_sweep_statuses(p._p, now, arr, 0, o, c, n))


def test_the_group_directory_over_a_ticked_swarm():
    sw = make_swarm(43, 120, 300)
    W = sw.W
    bind(plugin_lib())
    p = PluginCxx(sw)
    p.set_clock(NOW)
    p.sync_nodes(range(W), set(range(W)))
    p.sync_tasks(sw.task_masks(), sw.created_at, sw.task_uid)
    p.eng.W = W
    # both ledgers off: the listing works, the rows name no class, the degraded list needs liveness
    p.tick()
    want = p.get_all_groups()                                   # sorted by id text (mod.rs:1040)
    assert len(want) > 20 and [g["id"] for g in want] == sorted(g["id"] for g in want)
    total, members, got = list_groups(p)
    assert total == len(want) and members == sum(len(g["nodes"]) for g in want)
    assert [(g["id"], g["config"], g["created_at"], g["nodes"]) for g in got] == \
           [(g["id"], g["config"], g["created_at"], g["nodes"]) for g in want]
    assert {(g["health"], g["rollout"]) for g in got} == {("-", "-")}
    with pytest.raises(RuntimeError):
        degraded(p)
    _check(p.L.pmx_enable_liveness(p._p, 3))
    _check(p.L.pmx_enable_rollout(p._p))
    # page by page, in id-text order
    for page in (1, 7, 50):
        joined = []
        for off in range(0, total + page, page):
            t, m, part = list_groups(p, offset=off, limit=page)
            assert (t, m) == (total, members) and len(part) == max(0, min(page, total - off))
            joined += part
        assert [(g["id"], g["config"], g["nodes"]) for g in joined] == [(g["id"], g["config"], g["nodes"]) for g in want], page
        assert all(g["size"] == len(g["nodes"]) for g in joined)
    # the gauge: a count over get_all_groups, present names only
    counts = {}
    for g in want:
        counts[g["config"]] = counts.get(g["config"], 0) + 1
    gauge = _text(lambda o, c, n: p.L.pmx_group_counts(p._p, o, c, n))
    assert gauge == "".join("%s\t%d\n" % kv for kv in sorted(counts.items()))
    # the claimed task's id; by size, largest first; one configuration alone
    served = [g for g in got if g["task"] != "-"]
    assert served and all(g["task"] in {uuid_of(u) for u in p.tasks} for g in served)
    _, _, by_size = list_groups(p, order=2)
    assert [g["size"] for g in by_size] == sorted((g["size"] for g in by_size), reverse=True) and len(by_size) == total
    first = p.config_names.index(want[0]["config"])
    t, _, only = list_groups(p, config_mask=1 << first)
    assert t == counts[want[0]["config"]] and {g["config"] for g in only} == {want[0]["config"]}
    # every node Healthy, every report missing: sound and (where a task is held) rolling; nobody is degraded
    _, _, got = list_groups(p)
    assert {g["health"] for g in got} == {"sound"} and {g["rollout"] for g in got} <= {"no_task", "rolling"}
    assert degraded(p) == []
    victim_group = next(g for g in want if len(g["nodes"]) > 1)
    victim = p.node_of_addr[victim_group["nodes"][0]]
    task = next(g["task"] for g in got if g["id"] == victim_group["id"])
    if task != "-":                                             # its members report the claimed task RUNNING: converged
        for a in victim_group["nodes"]:
            _check(p.L.pmx_report_task(p._p, a.encode(), task.encode(), b"RUNNING"))
        _check(p.L.pmx_flush_rollout(p._p))
        _, _, conv = list_groups(p, rollout=1 << 1)
        assert [g["id"] for g in conv] == [victim_group["id"]] and conv[0]["rollout"] == "converged"
    # one silent interval for one member: Unhealthy, the group stands (handle_status_change dissolves on Dead and LowBalance only)
    now = NOW
    for k, quiet in enumerate(({victim}, set())):
        now += STEP
        for node in range(W):
            if node not in quiet:
                _check(p.L.pmx_beat(p._p, p.addr[node], now - 100))
        sweep(p, now)
        d = degraded(p)
        if k == 0:
            assert [(g["id"], g["health"], g["nodes"]) for g in d] == [(victim_group["id"], "degraded", victim_group["nodes"])]
            t, _, rows = list_groups(p, health=1 << 1)
            assert t == 1 and rows == d
            assert victim_group["id"] in [g["id"] for g in p.get_all_groups()]
        else:
            assert d == []                                      # it beat again: Healthy, the list is empty
    p.close()
