"""Named cases of the rollout ledger, as data: a task list, adopted groups, steps, and what must come out — written down by
hand from the rules of include/pm_engine.h, so that the model (tests/rollout_model.py) is held to them on the CPU and the engine
to the model on the GPU.

A case: W workers; `tasks` the ids of the list in its order; `groups` [(members, position of the claimed task or -1)] in
creation order; `steps`:
  ("report", [(worker, id or None, state text or None), ...])   the heartbeat's fields: update_node_task's match decides
  ("delete", [ids])                                             pm_tasks_delete: the groups that held them dissolve
  ("dead", worker)                                              the node dies: its group dissolves, its row stays
`classes`: the class of every worker at the end; `per_task`: {id: reporting rows} (nodes_per_task); `converged`: the number of
groups whose every member is converged."""
import rollout_model as M

I, S, Q, O, B, C = M.IDLE, M.STRAY, M.SILENT, M.OTHER, M.BEHIND, M.CONVERGED
ONES = M.ALL_ONES

CASES = [
    dict(name="every_class", W=8, tasks=[10, 20],
         groups=[([0, 1, 2, 3], 0), ([4, 5], -1)],
         steps=[("report", [(0, 10, "RUNNING"), (1, 10, "PULLING"), (2, 20, "RUNNING"), (4, 10, "RUNNING"), (6, 20, "FAILED")])],
         classes=[C, B, O, Q, S, I, S, I], per_task={10: 3, 20: 2}, converged=0),
    dict(name="last_member_lags", W=4, tasks=[7],
         groups=[([0, 1, 2, 3], 0)],
         steps=[("report", [(0, 7, "RUNNING"), (1, 7, "RUNNING"), (2, 7, "RUNNING"), (3, 7, "PENDING")])],
         classes=[C, C, C, B], per_task={7: 4}, converged=0),
    dict(name="last_member_arrives", W=4, tasks=[7],
         groups=[([0, 1, 2, 3], 0)],
         steps=[("report", [(0, 7, "RUNNING"), (1, 7, "RUNNING"), (2, 7, "RUNNING"), (3, 7, "PENDING")]),
                ("report", [(3, 7, "RUNNING")])],
         classes=[C, C, C, C], per_task={7: 4}, converged=1),
    dict(name="two_groups_one_task_one_converged", W=5, tasks=[5, 6],
         groups=[([0, 1], 1), ([2, 3, 4], 1)],
         steps=[("report", [(0, 6, "RUNNING"), (1, 6, "RUNNING"), (2, 6, "RUNNING"), (3, 6, "RUNNING"), (4, 6, "COMPLETED")])],
         classes=[C, C, C, C, B], per_task={6: 5}, converged=1),
    dict(name="reported_id_no_task_carries", W=3, tasks=[1],
         groups=[([0, 1], 0)],
         steps=[("report", [(0, 999, "RUNNING"), (2, 999, "RUNNING"), (1, 1, "RUNNING")])],
         classes=[O, C, S], per_task={1: 1, 999: 2}, converged=0),
    dict(name="task_deleted_under_its_reporters", W=4, tasks=[11, 12],
         groups=[([0, 1], 0), ([2, 3], 1)],
         steps=[("report", [(0, 11, "RUNNING"), (1, 11, "RUNNING"), (2, 12, "RUNNING"), (3, 12, "RUNNING")]),
                ("delete", [11])],
         classes=[S, S, C, C], per_task={11: 2, 12: 2}, converged=1),
    dict(name="duplicate_ids", W=4, tasks=[3, 3, 4],
         groups=[([0, 1], 1), ([2], 0)],
         steps=[("report", [(0, 3, "RUNNING"), (1, 3, "RUNNING"), (2, 3, "RUNNING"), (3, 3, "UNKNOWN")])],
         classes=[C, C, C, S], per_task={3: 4}, converged=2),
    dict(name="all_ones_id", W=4, tasks=[ONES, 8],
         groups=[([0, 1], 0), ([2], 1)],
         steps=[("report", [(0, ONES, "RUNNING"), (2, ONES, "RUNNING"), (3, ONES, "RUNNING")])],
         classes=[O, Q, O, S], per_task={ONES: 3}, converged=0),
    dict(name="report_for_a_dead_row", W=3, tasks=[2],
         groups=[([0, 1], 0)],
         steps=[("report", [(0, 2, "RUNNING"), (1, 2, "RUNNING")]), ("dead", 1), ("report", [(1, 2, "FAILED")])],
         classes=[S, S, I], per_task={2: 2}, converged=0),
    dict(name="cleared_row", W=3, tasks=[2],
         groups=[([0, 1, 2], 0)],
         steps=[("report", [(0, 2, "RUNNING"), (1, 2, "RUNNING"), (2, 2, "RUNNING")]),
                ("report", [(1, None, None), (2, 2, None), (0, None, "RUNNING")])],
         classes=[Q, Q, Q], per_task={}, converged=0),
    dict(name="state_strings_in_wrong_case", W=3, tasks=[2],
         groups=[([0, 1, 2], 0)],
         steps=[("report", [(0, 2, "running"), (1, 2, "Running"), (2, 2, " RUNNING")])],
         classes=[B, B, B], per_task={2: 3}, converged=0),
    dict(name="id_zero_is_an_id", W=3, tasks=[0],
         groups=[([0, 1], 0)],
         steps=[("report", [(0, 0, "RUNNING"), (2, 0, "PAUSED")])],
         classes=[C, Q, S], per_task={0: 2}, converged=0),
]


def reports_of(rows, task_state=M.task_state_from):
    """the heartbeat's fields -> ledger reports [(worker, state, uid)] by update_node_task's match (node_store.rs:356-373)"""
    out = []
    for w, uid, state in rows:
        if uid is not None and state is not None:
            out.append((w, task_state(state), uid))
        else:
            out.append((w, M.TS_NONE, 0))
    return out


class Run:
    """a case's host state, step by step: the task list, the groups (each holding a row of the ORIGINAL list), the ledger"""

    def __init__(self, case):
        self.case = case
        self.W = case["W"]
        self.uids = list(case["tasks"])
        self.live = list(range(len(self.uids)))                      # original rows still in the list, in its order
        self.groups = [(0x5000 + k, 0, sorted(m), t) for k, (m, t) in enumerate(case["groups"])]
        self.led = M.Ledger()

    def apply(self, step, task_state=M.task_state_from):
        kind, arg = step
        if kind == "report":
            self.led.ingest(reports_of(arg, task_state))
        elif kind == "delete":
            gone = set()
            for u in arg:                                             # an id names the first live row that carries it
                hit = [k for k in self.live if self.uids[k] == u]
                if hit:
                    gone.add(hit[0])
                    self.live.remove(hit[0])
            self.groups = [g for g in self.groups if g[3] not in gone]
        elif kind == "dead":
            self.groups = [g for g in self.groups if arg not in g[2]]
        else:
            raise ValueError(kind)

    def task_uids(self):
        return [self.uids[k] for k in self.live]

    def group_list(self):
        """[(id, config, members, task position or -1)] as pm_get_groups would give it"""
        return [(gid, cfg, mem, -1 if t < 0 else self.live.index(t)) for gid, cfg, mem, t in self.groups]

    def group_of(self):
        of = [-1] * self.W
        for s, (_gid, _cfg, mem, _t) in enumerate(self.groups):
            for w in mem:
                of[w] = s
        return of

    def read(self):
        return M.read(self.W, self.group_of(), self.group_list(), self.task_uids(), self.led)
