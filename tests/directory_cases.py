"""Named cases of the node directory, as data: statuses, adopted groups, a task list, reports, ranks, queries, and what must come
out — written down by hand from the rules of include/pm_engine.h, so that the model (tests/directory_model.py) is held to them on
the CPU and the engine to the model on the GPU.

A case: `statuses` one PM_NS_* per row; `counters` (default: the row index); `tasks` the ids of the list in its order; `groups`
[(members, position of the claimed task or -1)] in creation order; `delete` ids that pm_tasks_delete takes out afterwards (the
groups that held them dissolve); `reports` None (the rollout ledger stays off) or [(worker, state, uid)]; `ranks` the addr_rank
column (default: the row index); `queries` [(query, total, the window's workers in order)]."""
import directory_model as M

D, W_, H, U, X, E, B, L = M.DISCOVERED, M.WAITING, M.HEALTHY, M.UNHEALTHY, M.DEAD, M.EJECTED, M.BANNED, M.LOWBALANCE
Q = M.query
ROW, ADDR = M.BY_ROW, M.BY_ADDRESS
MIXED = [X, D, H, U, W_, H, E, D, B, X, L, H]      # classes: H {2, 5, 11}, D {1, 7}, other {3, 4, 6, 8, 10}, dead {0, 9}
MIXED_ORDER = [2, 5, 11, 1, 7, 3, 4, 6, 8, 10, 0, 9]

CASES = [
    dict(name=f"status_{M.STATUS_NAMES[s]}_alone", statuses=[s] * 3, tasks=[], groups=[], reports=None,
         queries=[(Q(), 3, [0, 1, 2]), (Q(status_mask=1 << s, order=ADDR), 3, [0, 1, 2]),
                  (Q(status_mask=M.ALL & ~(1 << s)), 0, [])])
    for s in range(M.NS_N)
] + [
    dict(name="mixed_statuses_in_listing_order", statuses=MIXED, tasks=[], groups=[], reports=None,
         queries=[(Q(), 12, MIXED_ORDER), (Q(status_mask=M.NOT_DEAD), 10, MIXED_ORDER[:10]),
                  (Q(status_mask=1 << D), 2, [1, 7]), (Q(status_mask=1 << X), 2, [0, 9]),
                  (Q(limit=0), 12, []), (Q(offset=12), 12, []), (Q(offset=13, limit=5), 12, []),
                  (Q(offset=11), 12, [9]), (Q(offset=4, limit=M.TO_END), 12, MIXED_ORDER[4:])]),
    dict(name="all_rows_in_the_middle_class", statuses=[U, W_, E, B, L, U], tasks=[], groups=[], reports=None,
         ranks=[5, 4, 3, 2, 1, 0],
         queries=[(Q(), 6, [0, 1, 2, 3, 4, 5]), (Q(order=ADDR), 6, [5, 4, 3, 2, 1, 0])]),
    dict(name="an_empty_class_between_two_full_ones", statuses=[X, H, X, H, U, H], tasks=[], groups=[], reports=None,
         queries=[(Q(), 6, [1, 3, 5, 4, 0, 2]), (Q(status_mask=(1 << H) | (1 << X)), 5, [1, 3, 5, 0, 2]),
                  (Q(status_mask=(1 << H) | (1 << X), offset=2, limit=2), 5, [5, 0])]),
    dict(name="every_row_grouped", statuses=[H, H, D, H], tasks=[70], groups=[([0, 1], 0), ([2, 3], -1)], reports=None,
         queries=[(Q(), 4, [0, 1, 3, 2]), (Q(membership=M.GROUPED), 4, [0, 1, 3, 2]), (Q(membership=M.UNGROUPED), 0, [])]),
    dict(name="no_row_grouped", statuses=[H, D, X], tasks=[70], groups=[], reports=None,
         queries=[(Q(membership=M.GROUPED), 0, []), (Q(membership=M.UNGROUPED), 3, [0, 1, 2])]),
    dict(name="a_group_without_a_task", statuses=[H, H, H, D], tasks=[5, 6], groups=[([0, 2], -1), ([1], 1)], reports=None,
         queries=[(Q(), 4, [0, 1, 2, 3]), (Q(membership=M.GROUPED), 3, [0, 1, 2]), (Q(membership=M.UNGROUPED), 1, [3])]),
    dict(name="a_task_deleted_under_its_group", statuses=[H, H, H, H, U], tasks=[11, 12], groups=[([0, 1], 0), ([2, 3], 1)],
         delete=[11], reports=[(0, 2, 11), (1, 2, 11), (2, 2, 12)],
         queries=[(Q(), 5, [0, 1, 2, 3, 4]), (Q(membership=M.GROUPED), 2, [2, 3]), (Q(membership=M.UNGROUPED), 3, [0, 1, 4])]),
    dict(name="rollout_on_without_reports", statuses=[H, D], tasks=[1], groups=[([0], 0)], reports=[],
         queries=[(Q(), 2, [0, 1])]),
    dict(name="rollout_on_reports_and_a_cleared_row", statuses=[H, H, D, X], tasks=[1, 2], groups=[([0, 1], 1)],
         reports=[(0, 2, 2), (1, 0, 1), (3, 4, 0xFFFFFFFFFFFFFFFF), (2, 2, 9), (2, 255, 0)],
         queries=[(Q(), 4, [0, 1, 2, 3]), (Q(order=ADDR, offset=1, limit=2), 4, [1, 2])]),
    dict(name="tied_ranks_fall_back_to_the_row", statuses=[H, H, H, D, D, H], tasks=[], groups=[], reports=None,
         ranks=[7, 3, 7, 3, 3, 3],
         queries=[(Q(order=ADDR), 6, [1, 5, 0, 2, 3, 4]), (Q(order=ROW), 6, [0, 1, 2, 5, 3, 4])]),
    dict(name="ranks_at_the_edges_of_u32", statuses=[H, H, H, H, D, D, D], tasks=[], groups=[], reports=None,
         ranks=[0xFFFFFFFF, 1 << 31, 0, (1 << 31) - 1, 0xFFFFFFFF, 0, 1 << 31],
         queries=[(Q(order=ADDR), 7, [2, 3, 1, 0, 5, 6, 4]), (Q(order=ADDR, offset=3, limit=2), 7, [0, 5])]),
    dict(name="a_window_across_each_class_boundary", statuses=MIXED, tasks=[], groups=[], reports=None,
         ranks=[11 - w for w in range(12)],
         queries=[(Q(offset=2, limit=2), 12, [11, 1]), (Q(offset=4, limit=2), 12, [7, 3]), (Q(offset=9, limit=2), 12, [10, 0]),
                  (Q(order=ADDR, offset=2, limit=2), 12, [2, 7]), (Q(order=ADDR, offset=4, limit=2), 12, [1, 10]),
                  (Q(order=ADDR, offset=9, limit=2), 12, [3, 9]), (Q(order=ADDR), 12, [11, 5, 2, 7, 1, 10, 8, 6, 4, 3, 9, 0])]),
]


class Run:
    """a case's host state as the model takes it"""

    def __init__(self, case):
        self.W = len(case["statuses"])
        self.statuses = list(case["statuses"])
        self.counters = list(case.get("counters", range(self.W)))
        self.ranks = list(case.get("ranks", range(self.W)))
        uids = list(case["tasks"])
        live = list(range(len(uids)))
        groups = [(0x6000 + k, 0, sorted(m), t) for k, (m, t) in enumerate(case["groups"])]
        for u in case.get("delete", []):                              # an id names the first live row that carries it
            hit = [k for k in live if uids[k] == u][0]
            live.remove(hit)
            groups = [g for g in groups if g[3] != hit]
        self.task_uids = [uids[k] for k in live]
        self.groups = [(gid, cfg, mem, -1 if t < 0 else live.index(t)) for gid, cfg, mem, t in groups]
        self.group_of = [-1] * self.W
        for s, (_gid, _cfg, mem, _t) in enumerate(self.groups):
            for w in mem:
                self.group_of[w] = s
        self.ledger = None
        if case["reports"] is not None:
            self.ledger = [(0, M.TS_NONE)] * self.W
            for w, st, uid in case["reports"]:
                self.ledger[w] = (0, M.TS_NONE) if st == M.TS_NONE else (uid, st)

    def read(self, q):
        return M.directory(self.statuses, self.counters, self.group_of, self.groups, self.task_uids, self.ledger, self.ranks, q)
