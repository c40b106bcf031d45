"""A plain restatement of the solo-group merge, written from the reference's Rust — NOT from oracle/pm_oracle.c — so that
the test suite has a second, independent reading of it beside the oracle:

    try_merge_solo_groups            crates/orchestrator/src/plugins/node_groups/mod.rs:631-673
    try_merge_groups_for_config      :676-709
    find_compatible_solo_groups      :712-749
    attempt_group_merge              :752-860
    is_merge_beneficial              :863-873
    should_switch_tasks              :257-296
    get_all_groups' order            :1040 (by the id STRING, ids are format!("{:x}", u64): :1489-1493)

It picks no task and makes no group ids (a merged group has two members or more and never enters a later list, so its
id does not matter here); those stay the oracle's.  The only thing it borrows is the distance function
(oracle_ffi.distance_column: the same libm as the oracle and the engine's host path); the sort is Python's stable sort
on the distance alone.

Every attempt gets one label:

    prox_full   a located seed and its nearest located neighbours fill the batch to max_group_size
    prox_short  ... fewer than max but at least min: kept short, no refill (:823-826 is false)
    cleared     ... fewer than min: the partial batch is thrown away (:828-832) and the batch is refilled first-come from
                the top of the list (:835-847); `partial` is the size of what was thrown away
    no_seed     no located group in the list (or proximity off): first-come
    refused     the batch has fewer than two groups, or switching is off (:868-870, :263-265): ends the configuration
    blocked     prefer_larger_groups = false and a group of the batch holds a task (:277-287): ends the configuration
"""
from oracle import oracle_ffi as orc

LABELS = ("prox_full", "prox_short", "cleared", "no_seed", "refused", "blocked")


class Attempt:
    __slots__ = ("cfg", "label", "select", "partial", "n_rem", "n_loc", "batch")

    def __init__(self, cfg, label, select, partial, n_rem, n_loc, batch):
        self.cfg = cfg          # configuration index
        self.label = label      # one of LABELS
        self.select = select    # how the batch was selected (prox_full / prox_short / cleared / no_seed), also when refused
        self.partial = partial  # size of the proximity batch that was cleared (0 otherwise)
        self.n_rem = n_rem      # length of the remaining list the attempt saw
        self.n_loc = n_loc      # located groups in it (0 with proximity off: nobody looked)
        self.batch = batch      # nodes of the batch in batch order

    def __repr__(self):
        return f"Attempt(cfg={self.cfg}, {self.label}, select={self.select}, partial={self.partial}, n_rem={self.n_rem}, n={len(self.batch)})"


class Result:
    def __init__(self):
        self.merged = []     # [(configuration, [nodes in batch order])] in creation order
        self.attempts = []   # [Attempt] in order
        self.lists = []      # [(configuration, len(find_compatible_solo_groups))] per available configuration, in order

    def count(self, label):
        return sum(a.label == label for a in self.attempts)


def id_string(gid: int) -> str:
    return "%x" % gid


def available_order(configs, enabled):
    """get_available_configurations (:399-418) over the constructor's template order (:150-164): both sorts are stable.
    configs: [(name, min, max, requirement or None)] in the order they were given; enabled: per configuration."""
    template = sorted(range(len(configs)), key=lambda i: (-configs[i][1], configs[i][3] is None))
    avail = [i for i in template if enabled[i]]
    return sorted(avail, key=lambda i: -configs[i][1])


def _attempt(rem, cfg, mn, mx, has_loc, lat, lon, task_of, proximity, switching, prefer_larger):
    """attempt_group_merge over `rem` = [(id string, node)] in get_all_groups order -> Attempt: the batch as it was
    selected; the label says whether it is applied"""
    batch = []
    select, partial, n_loc = "no_seed", 0, 0
    if proximity:                                                     # :763
        located = [node for _gid, node in rem if has_loc[node]]
        n_loc = len(located)
        if located:                                                   # :772-780: the first located group is the seed
            seed, others = located[0], located[1:]                    # :791-802 (filter_map: located groups only)
            batch.append(seed)                                        # :786-788
            if others:
                d = orc.distance_column(float(lat[seed]), float(lon[seed]), lat[others], lon[others]).tolist()
                for k in sorted(range(len(others)), key=d.__getitem__):    # :804-805 (stable), :808-818
                    if len(batch) + 1 <= mx:
                        batch.append(others[k])
                        if len(batch) >= mx:
                            break
            select = "prox_full" if len(batch) >= mx else "prox_short"
    if not batch or (len(batch) < mx and len(batch) < mn):           # :823-826
        if len(batch) < mn:                                           # :828-832
            if batch:
                select, partial = "cleared", len(batch)
            batch = []
        taken = set(batch)
        for _gid, node in rem:                                        # :835-847
            if node not in taken and len(batch) + 1 <= mx:
                batch.append(node)
                taken.add(node)
                if len(batch) >= mx:
                    break
    label = select
    if len(batch) < 2:                                                # :868-870 (solo groups: new_size == groups.len())
        label = "refused"
    elif not switching:                                               # :263-265
        label = "refused"
    elif not prefer_larger and any(task_of[n] >= 0 for n in batch):  # :277-287
        label = "blocked"
    return Attempt(cfg, label, select, partial, len(rem), n_loc, batch)


def merge_solo_groups(groups, has_loc, lat, lon, compat, avail, min_max, *, proximity=True, switching=True,
                      prefer_larger=True) -> Result:
    """groups: the live groups [(id, configuration, members, task or -1)]; has_loc / lat / lon: per node (numpy);
    compat(cfg, node) -> bool; avail: the available configurations in order (available_order); min_max[cfg] = (min, max)."""
    res = Result()
    solos = sorted((id_string(gid), mem[0]) for gid, _cfg, mem, _task in groups if len(mem) == 1)    # :1040
    if len(solos) < 2:                                                # :640-644
        return res
    task_of = {mem[0]: task for _gid, _cfg, mem, task in groups if len(mem) == 1}
    gone = set()                                                      # nodes of dissolved solo groups (:903-921)
    for cfg in avail:                                                 # :654 (:656: the list is read again)
        mn, mx = min_max[cfg]
        rem = [g for g in solos if g[1] not in gone and compat(cfg, g[1])]     # :685, :712-734
        res.lists.append((cfg, len(rem)))
        while len(rem) >= mn:                                         # :687-690, :694
            a = _attempt(rem, cfg, mn, mx, has_loc, lat, lon, task_of, proximity, switching, prefer_larger)
            res.attempts.append(a)
            if a.label in ("refused", "blocked"):                     # :704
                break
            res.merged.append((cfg, list(a.batch)))
            gone.update(a.batch)
            rem = [g for g in rem if g[1] not in gone]                # :702
    return res
