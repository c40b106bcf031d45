"""A plain restatement of group formation, written from the reference's Rust — NOT from oracle/pm_oracle.c — so that the
test suite has a second, independent reading of it beside the oracle:

    try_form_new_groups              crates/orchestrator/src/plugins/node_groups/mod.rs:478-628
    is_node_compatible_with_config   :206-215 (taken as the compat matrix: compat has its own tests)
    calculate_distance               :218-231 (borrowed: oracle_ffi.distance_column, the oracle's and the host path's libm)
    sort_nodes_by_proximity          :234-255
    get_available_configurations     :399-418 (merge_model.available_order)

It makes no group ids and picks no tasks; those stay the oracle's.  Python lists, and Python's stable sort on the
distance alone.  What it keeps between two iterations of the `while` of :507 — the configuration's compatible nodes in
input order — is what :511-515 would filter out of healthy_nodes again: only the nodes of the group just made leave
either list (:585).

Every iteration of the `while` gets one record and one label:

    prox_full        located seed, the group reaches max_group_size with located candidates only (:545-551)
    prox_fill        located seed, the group reaches max only with location-less candidates: they sort behind every
                     located one, in input order (unwrap_or(f64::MAX), :239-253, a stable sort); `fill_in_front` says
                     whether one of them stands in front of the seed in the input
    prox_short       located seed, everything compatible is taken and it is fewer than max (at least min: :564 is false):
                     the configuration's last group
    seed_unlocated   no located compatible node: the seed is compatible_nodes.first(), sort_nodes_by_proximity does
                     nothing (:238), the group is first-come (:526-530)
    first_come       proximity off (:553-560)
    stop_compatible  fewer compatible nodes than min: the configuration ends, its leftovers stay free (:517)
    stop_total       the `while` condition fails: total_available — ALL eligible nodes, compatible or not — is below min

A step's `tie` says whether the selection's boundary (the last candidate taken, the first one left) falls inside a run of
exactly equal distances: "site" when the whole run is at one site (input order decides, and everybody can see that),
"cross" when it spans different sites (the engine's certificate cannot settle it: the step is the host's), else None.
"""
from oracle import oracle_ffi as orc
from merge_model import available_order  # noqa: F401  (re-exported: the cases call it through this module)

LABELS = ("prox_full", "prox_fill", "prox_short", "seed_unlocated", "first_come", "stop_compatible", "stop_total")
GROUP_LABELS = LABELS[:5]
ST_HEALTHY = 2              # NodeStatus::Healthy (models/node.rs:75-85)
F64_MAX = 1.7976931348623157e308


class Step:
    __slots__ = ("cfg", "label", "n_total", "n_compatible", "n_located", "seed", "group", "fill_in_front", "tie")

    def __init__(self, cfg, label, n_total, n_compatible, n_located, seed=None, group=None, fill_in_front=False, tie=None):
        self.cfg = cfg                      # configuration index
        self.label = label                  # one of LABELS
        self.n_total = n_total              # total_available at the top of the iteration
        self.n_compatible = n_compatible    # compatible_nodes.len()
        self.n_located = n_located          # located ones among them
        self.seed = seed                    # the seed node (None for a stop, and with proximity off)
        self.group = group                  # members in BTreeSet (address) order, None for a stop
        self.fill_in_front = fill_in_front  # prox_fill: a location-less member stands in front of the seed
        self.tie = tie                      # None / "site" / "cross"

    def __repr__(self):
        return (f"Step(cfg={self.cfg}, {self.label}, total={self.n_total}, compatible={self.n_compatible}, "
                f"located={self.n_located}, seed={self.seed}, n={len(self.group) if self.group else 0}, tie={self.tie})")


class Result:
    def __init__(self):
        self.groups = []    # [(configuration, [members in BTreeSet order])] in creation order
        self.steps = []     # [Step] in order
        self.entries = []   # [(configuration, n_total, n_compatible, n_located)] at each available configuration's entry

    def count(self, label):
        return sum(s.label == label for s in self.steps)

    def entry(self, cfg):
        return next(e for e in self.entries if e[0] == cfg)


def _tie(order, d, taken, lat, lon):
    """order: the candidates behind the seed as sorted; d: their sort keys in that order; taken: how many the group took"""
    if taken == 0 or taken >= len(order) or d[taken - 1] != d[taken] or d[taken] == F64_MAX:
        return None
    lo = taken - 1
    while lo > 0 and d[lo - 1] == d[taken]:
        lo -= 1
    hi = taken
    while hi + 1 < len(order) and d[hi + 1] == d[taken]:
        hi += 1
    sites = {(float(lat[w]), float(lon[w])) for w in order[lo:hi + 1]}
    return "site" if len(sites) == 1 else "cross"


def form_new_groups(status, has_p2p, has_loc, lat, lon, in_group, addr_key, configs, enabled, compat, proximity=True) -> Result:
    """status / has_p2p / has_loc / lat / lon / in_group / addr_key: per node, in NodeStore::get_nodes order (in_group:
    the node is in NODE_GROUP_MAP_KEY; addr_key: something that orders like the address string);
    configs: [(name, min, max, requirement or None)] as given to the constructor; enabled: per configuration;
    compat(cfg, node) -> bool."""
    res = Result()
    W = len(status)
    has_loc = [bool(v) for v in has_loc]
    healthy = [w for w in range(W) if status[w] == ST_HEALTHY and has_p2p[w] and not in_group[w]]    # :492-497
    total = len(healthy)                                                                               # :503
    for cfg in available_order(configs, enabled):                                                      # :483, :505
        _name, mn, mx, _req = configs[cfg]
        compatible = [w for w in healthy if compat(cfg, w)]                                            # :511-515
        located = [w for w in compatible if has_loc[w]]
        res.entries.append((cfg, total, len(compatible), len(located)))
        while True:
            if not total >= mn:                                                                        # :507
                res.steps.append(Step(cfg, "stop_total", total, len(compatible), len(located)))
                break
            if len(compatible) < mn:                                                                   # :517
                res.steps.append(Step(cfg, "stop_compatible", total, len(compatible), len(located)))
                break
            seed, tie, in_front = None, None, False
            if proximity:                                                                              # :524
                seed = located[0] if located else compatible[0]                                        # :526-530
                picked = [seed]                                                                        # :534-535
                # (max = 1 takes nobody from the list, :546: neither the list nor the sort is made)
                rest = [w for w in compatible if w != seed] if mx > 1 else []                          # :538-541
                if has_loc[seed] and mx > 1:                                                           # :238
                    d = orc.distance_column(float(lat[seed]), float(lon[seed]), lat[rest], lon[rest]).tolist()
                    key = [d[i] if has_loc[w] else F64_MAX for i, w in enumerate(rest)]                # :240-249
                    idx = sorted(range(len(rest)), key=key.__getitem__)                               # :239, :250-252 (stable)
                    rest = [rest[i] for i in idx]
                    key = [key[i] for i in idx]
                else:
                    key = None
                for w in rest:                                                                         # :545-551
                    if len(picked) >= mx:
                        break
                    picked.append(w)
                if key is not None:
                    tie = _tie(rest, key, len(picked) - 1, lat, lon)
                if not has_loc[seed]:
                    label = "seed_unlocated"
                elif len(picked) < mx:
                    label = "prox_short"
                elif all(has_loc[w] for w in picked):
                    label = "prox_full"
                else:
                    label = "prox_fill"
                    in_front = any(not has_loc[w] and w < seed for w in picked)
            else:
                picked = compatible[:mx]                                                               # :554-560
                label = "first_come"
            assert len(picked) >= mn                                                                   # (:564 cannot hold)
            group = sorted(picked, key=addr_key.__getitem__)                                           # :521 (BTreeSet)
            res.steps.append(Step(cfg, label, total, len(compatible), len(located), seed, group, in_front, tie))
            res.groups.append((cfg, group))
            gone = set(picked)                                                                         # :585
            healthy = [w for w in healthy if w not in gone] if len(gone) > 8 else _without(healthy, picked)
            compatible = [w for w in compatible if w not in gone] if len(gone) > 8 else _without(compatible, picked)
            located = [w for w in located if w not in gone] if len(gone) > 8 else _without(located, picked)
            total = len(healthy)                                                                       # :586
    return res


def _without(nodes, picked):
    """`nodes` without the picked ones, order kept (retain, :585) — small groups leave a long list one by one"""
    for w in picked:
        try:
            nodes.remove(w)
        except ValueError:
            pass
    return nodes
