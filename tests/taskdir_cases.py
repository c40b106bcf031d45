"""Named cases of the task directory, worked out by hand from the header's definitions (include/pm_engine.h, "task directory").
tests/test_taskdir_model.py holds the model to them; tests/test_gpu_taskdir.py runs them through the C ABI.

A case: name, W, n_cfgs, tasks [(uid, created_at, topo_mask)] in list order, groups [(id, config, members, task position or -1)],
ledger [(uid, state)] per worker row or None (rollout off), queries [(query, listed positions in order, totals or None)]."""
import taskdir_model as M

RUN, PULLING, FAILED, SILENT = M.TS_RUNNING, 1, 4, M.TS_NONE
ALL = M.ALL_ONES

# Three configurations; seven tasks, newest first:
#   0  id 50   unrestricted       held by g0 (converged) and g1 (one member pulling, one silent): running, rolling
#   1  id 40   c0                 no group holds it, three c0 groups stand: waiting, unheld; the FIRST row of id 40
#   2  id 30   c2                 no c2 group stands: starved
#   3  id 20   mask 0             names only unknown topologies: starved, listed under "no filter" alone
#   4  id 40   c0 | c1            a DUPLICATE id; held by g2, whose one member reports 40 running: running, converged —
#                                 the reported columns of id 40 are credited to row 1, this row shows zeros there
#   5  id ~0   c1                 held by g3; an id of all ones never matches: rolling, and its reports are orphans
#   6  id 10   bit 3 alone        a bit above the installed configurations: allows nothing installed, starved
# twelve rows: g0 = {0, 1}, g1 = {2, 3, 4}, g2 = {5}, g3 = {6, 7}, g4 = {8} holds nothing; 9, 10, 11 are in no group.
# Rows 8 and 10 report id 77, which no task carries; row 9 reports id 40 failed from outside any group.
TASKS = [(50, 90, ALL), (40, 80, 0b001), (30, 70, 0b100), (20, 60, 0), (40, 50, 0b011), (ALL, 40, 0b010), (10, 30, 0b1000)]
GROUPS = [(0x10, 0, [0, 1], 0), (0x11, 0, [2, 3, 4], 0), (0x12, 1, [5], 4), (0x13, 1, [6, 7], 5), (0x14, 0, [8], -1)]
LEDGER = [(50, RUN), (50, RUN), (50, RUN), (50, PULLING), (0, SILENT), (40, RUN), (ALL, RUN), (ALL, RUN), (77, RUN), (40, FAILED),
          (77, RUN), (0, SILENT)]
Q = M.query
EVERYTHING = (7, 7, (3, 1, 3), (4, 1, 2), 1, 8, 6, 2, 4, 3)
EVERYTHING_RO_OFF = (7, 7, (3, 1, 3), (0, 0, 0), 1, 8, 0, 0, 0, 3)


def _case(name, queries, ledger=LEDGER, tasks=TASKS, groups=GROUPS, W=12, n_cfgs=3):
    return dict(name=name, W=W, n_cfgs=n_cfgs, tasks=tasks, groups=groups, ledger=ledger, queries=queries)


CASES = [
    _case("every_task_in_list_order", [(Q(), [0, 1, 2, 3, 4, 5, 6], EVERYTHING)]),
    _case("serving_classes", [
        (Q(serve_mask=1 << M.TKS_RUNNING), [0, 4, 5], (7, 3, (3, 0, 0), (0, 1, 2), 1, 8, 4, 2, 4, 3)),
        (Q(serve_mask=1 << M.TKS_WAITING), [1], (7, 1, (0, 1, 0), (1, 0, 0), 0, 0, 2, 2, 4, 3)),
        (Q(serve_mask=1 << M.TKS_STARVED), [2, 3, 6], (7, 3, (0, 0, 3), (3, 0, 0), 0, 0, 0, 2, 4, 3))]),
    _case("rollout_classes", [
        (Q(rollout_mask=1 << M.TKR_UNHELD), [1, 2, 3, 6], None),
        (Q(rollout_mask=1 << M.TKR_CONVERGED), [4], (7, 1, (1, 0, 0), (0, 1, 0), 0, 1, 0, 2, 4, 3)),
        (Q(rollout_mask=1 << M.TKR_ROLLING), [0, 5], None)]),
    _case("mask_0_task_only_without_a_filter", [
        (Q(), [0, 1, 2, 3, 4, 5, 6], None),
        (Q(config_mask=0b111), [0, 1, 2, 4, 5], None),
        (Q(config_mask=ALL >> 1), [0, 1, 2, 4, 5], None)]),
    _case("configuration_filters", [
        (Q(config_mask=0b100), [0, 2], None),
        (Q(config_mask=0b1000), [], (7, 0, (0, 0, 0), (0, 0, 0), 0, 0, 0, 2, 4, 3)),
        (Q(config_mask=(1 << 63) | 0b010), [0, 4, 5], None)]),
    _case("unrestricted_task", [(Q(config_mask=0b100, serve_mask=1 << M.TKS_RUNNING), [0], (7, 1, (1, 0, 0), (0, 0, 1), 1, 5, 4, 2, 4, 3))]),
    _case("two_holders_one_converged", [(Q(workers_min=5, workers_max=5), [0], None)]),
    _case("orphans_whatever_the_filter", [(Q(serve_mask=1 << M.TKS_WAITING, config_mask=0b100), [], (7, 0, (0, 0, 0), (0, 0, 0), 0, 0, 0, 2, 4, 3))]),
    _case("duplicate_id_with_reporters", [(Q(order=M.BY_REPORTERS_DESC, limit=2), [0, 1], None),
                                          (Q(rollout_mask=1 << M.TKR_CONVERGED), [4], None)]),
    _case("id_of_all_ones", [(Q(config_mask=0b010, workers_min=2), [0, 5], None)]),
    _case("workers_filter", [(Q(workers_min=1, workers_max=2), [4, 5], None), (Q(workers_max=0), [1, 2, 3, 6], None)]),
    _case("filters_combined", [(Q(config_mask=0b010, serve_mask=1 << M.TKS_RUNNING, rollout_mask=1 << M.TKR_ROLLING, workers_min=2,
                                  order=M.BY_WORKERS_DESC), [0, 5], None)]),
    _case("orders_with_ties", [
        (Q(order=M.BY_OLDEST), [6, 5, 4, 3, 2, 1, 0], EVERYTHING),
        (Q(order=M.BY_WORKERS_DESC), [0, 5, 4, 1, 2, 3, 6], EVERYTHING),
        (Q(order=M.BY_REPORTERS_DESC), [0, 1, 2, 3, 4, 5, 6], EVERYTHING)]),
    _case("windows", [
        (Q(order=M.BY_OLDEST, offset=2, limit=3), [4, 3, 2], EVERYTHING),
        (Q(offset=6, limit=5), [6], None), (Q(offset=7), [], EVERYTHING), (Q(offset=M.TO_END, limit=M.TO_END), [], None),
        (Q(limit=0), [], EVERYTHING), (Q(order=M.BY_WORKERS_DESC, offset=1, limit=2), [5, 4], None)]),
    _case("rollout_off", [(Q(), [0, 1, 2, 3, 4, 5, 6], EVERYTHING_RO_OFF), (Q(order=M.BY_WORKERS_DESC), [0, 5, 4, 1, 2, 3, 6], None)],
          ledger=None),
    _case("no_group_stands", [(Q(), [0, 1], (2, 2, (0, 0, 2), (2, 0, 0), 1, 0, 1, 1, 1, 1))],
          tasks=[(7, 2, ALL), (8, 1, 1)], groups=[], ledger=[(7, RUN), (9, RUN)], W=2, n_cfgs=1),
]
