"""The discovery monitor's sync as a model, twice.

sequential_pass is the reference read literally: DiscoveryMonitor::get_nodes -> sync_single_node_with_discovery
(orchestrator/src/discovery/monitor.rs:218-435) over a dict store, one discovery row after the other, every row counting the
Healthy nodes on its endpoint in the store as the rows before it left it.  add_node writes the whole snapshot
(store/domains/node_store.rs:27-60, 211-226); update stamps now (:284-305).  Every arm a row takes leaves its label.

parallel_pass is the formulation pm_discovery_sync computes (include/pm_engine.h): integers only, a count from three sets, the
row rule as a function of (status, count, row).  to_abi turns a store and a discovery list into its inputs; as_results turns
the sequential pass's outcomes into its outputs, so the two can be compared field by field."""

DISCOVERED, WAITING, HEALTHY, UNHEALTHY, DEAD, EJECTED, BANNED, LOWBALANCE = range(8)
N_STATUS = 8
STATUS_NAMES = ["Discovered", "WaitingForHeartbeat", "Healthy", "Unhealthy", "Dead", "Ejected", "Banned", "LowBalance"]
GRACE_MS = 300_000                                                       # monitor.rs:304
DISC_NEW = EP_NONE = 0xFFFFFFFF
DF_VALIDATED, DF_WHITELISTED, DF_ACTIVE, DF_LOCATION_NEW, DF_SPECS_DIFFER, DF_BALANCE_ZERO = 1, 2, 4, 8, 16, 32
DO_ADMIT, DO_SKIP, DO_IP_REWRITE, DO_LOCATION, DO_SPECS_REWRITE, DO_STAMP_NOW = 1, 2, 4, 8, 16, 32

ARMS = ["known.shared_endpoint_dead", "known.not_whitelisted_ejected", "known.whitelisted_ejected_to_dead",
        "known.inactive_ejected", "known.inactive_dead", "known.inactive_in_grace", "known.ip_rewrite", "known.location",
        "known.dead_rediscovered", "known.specs_rewrite", "known.low_balance", "known.nothing", "new.skip", "new.admit"]


def node(address, status, ip="10.0.0.1", port=8080, stamp=None, location=None, specs="specs-a"):
    """an OrchestratorNode: ip None stands for a row the host has retired (it matches no endpoint)"""
    return dict(address=address, status=status, ip_address=ip, port=port, last_status_change=stamp, location=location,
                compute_specs=specs)


def sighting(address, ip="10.0.0.1", port=8080, validated=True, whitelisted=True, active=True, location=None,
             specs="specs-a", last_updated=None, balance=None):
    """a DiscoveryNode"""
    return dict(id=address, ip_address=ip, port=port, is_validated=validated, is_provider_whitelisted=whitelisted,
                is_active=active, location=location, compute_specs=specs, last_updated=last_updated, latest_balance=balance)


def make_store(nodes):
    return {n["address"]: dict(n) for n in nodes}


# ---------------------------------------------------------------------------------------------------------------- sequential

def _add_node(store, n):                                                 # node_store.rs:211-226: every field of the clone
    store[n["address"]] = dict(n)


def _update_node_status(store, address, new, now_ms, out):               # monitor.rs:65-88
    old = store[address]["status"]                                       # :71-74
    store[address]["status"] = new                                       # node_store.rs:284-305
    store[address]["last_status_change"] = now_ms
    out["updates"].append((old, new))                                    # :83-85: the handlers see (updated node, old)


def count_healthy_nodes_with_same_endpoint(store, address, ip, port):    # :218-234
    return sum(1 for o in store.values()
               if o["address"] != address and o["ip_address"] == ip and o["port"] == port and o["status"] == HEALTHY)


def sync_single_node(store, d, now_ms, max_same):
    """monitor.rs:236-420 -> dict(cnt, arms, updates, known, old_status)"""
    address = d["id"]
    cnt = count_healthy_nodes_with_same_endpoint(store, address, d["ip_address"], d["port"])  # :243-249
    out = dict(cnt=cnt, arms=[], updates=[], known=address in store, old_status=None)
    ex = store.get(address)                                              # :251
    if ex is None:                                                       # :397-413
        if cnt >= max_same:
            out["arms"].append("new.skip")
            return out
        out["arms"].append("new.admit")
        _add_node(store, node(address, DISCOVERED, d["ip_address"], d["port"], None, d["location"], d["compute_specs"]))
        return out
    ex = dict(ex)                                                        # the snapshot
    out["old_status"] = ex["status"]
    assert ex["last_status_change"] != now_ms, "the model tells an update's stamp from the snapshot's by its value"
    if cnt > 0 and ex["status"] != HEALTHY:                              # :254-268
        out["arms"].append("known.shared_endpoint_dead")
        _update_node_status(store, address, DEAD, now_ms, out)
        return out
    if d["is_validated"] and not d["is_provider_whitelisted"]:           # :270-280
        out["arms"].append("known.not_whitelisted_ejected")
        _update_node_status(store, address, EJECTED, now_ms, out)
    if d["is_validated"] and d["is_provider_whitelisted"] and ex["status"] == EJECTED:  # :284-297
        out["arms"].append("known.whitelisted_ejected_to_dead")
        _update_node_status(store, address, DEAD, now_ms, out)
    if not d["is_active"] and ex["status"] == HEALTHY:                   # :298-334
        if ex["last_status_change"] is not None:
            should_mark_inactive = now_ms - ex["last_status_change"] > GRACE_MS  # :306 signed, strict
        else:
            should_mark_inactive = True                                  # :309
        if should_mark_inactive:
            if not d["is_provider_whitelisted"]:
                out["arms"].append("known.inactive_ejected")
                _update_node_status(store, address, EJECTED, now_ms, out)
            else:
                out["arms"].append("known.inactive_dead")
                _update_node_status(store, address, DEAD, now_ms, out)
        else:
            out["arms"].append("known.inactive_in_grace")
    if ex["ip_address"] != d["ip_address"]:                              # :336-344
        out["arms"].append("known.ip_rewrite")
        n = dict(ex)
        n["ip_address"] = d["ip_address"]
        _add_node(store, n)
    if ex["location"] is None and d["location"] is not None:            # :345-357
        out["arms"].append("known.location")
        store[address]["location"] = d["location"]                       # update_node_location: the location only
    if ex["status"] == DEAD:                                             # :359-383
        if ex["last_status_change"] is not None and d["last_updated"] is not None:
            if ex["last_status_change"] < d["last_updated"]:
                out["arms"].append("known.dead_rediscovered")
                if ex["compute_specs"] != d["compute_specs"]:
                    out["arms"].append("known.specs_rewrite")
                    n = dict(ex)
                    n["compute_specs"] = d["compute_specs"]
                    _add_node(store, n)
                _update_node_status(store, address, DISCOVERED, now_ms, out)
    if d["latest_balance"] is not None and d["latest_balance"] == 0:    # :385-395
        out["arms"].append("known.low_balance")
        _update_node_status(store, address, LOWBALANCE, now_ms, out)
    if not out["arms"]:
        out["arms"].append("known.nothing")
    return out


def sequential_pass(store, discovery, now_ms, max_same):
    """monitor.rs:422-430; the store is changed in place"""
    return [sync_single_node(store, d, now_ms, max_same) for d in discovery]


# ------------------------------------------------------------------------------------------------------- the ABI's inputs

class Interner:
    def __init__(self):
        self.ids = {}

    def __call__(self, ip, port):
        if ip is None:
            return EP_NONE
        return self.ids.setdefault("%s:%d" % (ip, port), len(self.ids))

    def __len__(self):
        return len(self.ids)


def to_abi(store, discovery, intern=None):
    """-> dict(addresses, status [W], row_endpoint [W], n_endpoints, rows [D] of (row, endpoint, endpoint_after, flags,
    last_change_ms, last_updated_ms)); table row w is the store's w-th node"""
    intern = intern if intern is not None else Interner()
    addresses = list(store)
    index = {a: w for w, a in enumerate(addresses)}
    row_endpoint = [intern(store[a]["ip_address"], store[a]["port"]) for a in addresses]
    rows = []
    for d in discovery:
        ex = store.get(d["id"])
        flags = (DF_VALIDATED if d["is_validated"] else 0) | (DF_WHITELISTED if d["is_provider_whitelisted"] else 0) \
            | (DF_ACTIVE if d["is_active"] else 0) | (DF_BALANCE_ZERO if d["latest_balance"] == 0 else 0)
        endpoint = intern(d["ip_address"], d["port"])
        if ex is None:
            rows.append((DISC_NEW, endpoint, 0, flags, 0, d["last_updated"] or 0))
            continue
        if ex["location"] is None and d["location"] is not None:
            flags |= DF_LOCATION_NEW
        if ex["compute_specs"] != d["compute_specs"]:
            flags |= DF_SPECS_DIFFER
        rows.append((index[d["id"]], endpoint, intern(d["ip_address"], ex["port"]), flags, ex["last_status_change"] or 0,
                     d["last_updated"] or 0))
    return dict(addresses=addresses, status=[store[a]["status"] for a in addresses], row_endpoint=row_endpoint,
                n_endpoints=len(intern), rows=rows, intern=intern)


def as_results(outs, store_before, store_after, now_ms):
    """the sequential pass's outcomes in pm_disc_result's terms: dict(cnt, old_status, final_status, updates, ops) per row"""
    res = []
    for o, d in zip(outs["outs"], outs["discovery"]):
        a = o["arms"]
        if not o["known"]:
            admit = "new.admit" in a
            res.append(dict(cnt=o["cnt"], old_status=N_STATUS, final_status=DISCOVERED if admit else N_STATUS, updates=[],
                            ops=DO_ADMIT if admit else DO_SKIP))
            continue
        after = store_after[d["id"]]
        ops = (DO_IP_REWRITE if "known.ip_rewrite" in a else 0) | (DO_LOCATION if "known.location" in a else 0) \
            | (DO_SPECS_REWRITE if "known.specs_rewrite" in a else 0) | (DO_STAMP_NOW if after["last_status_change"] == now_ms else 0)
        res.append(dict(cnt=o["cnt"], old_status=o["old_status"], final_status=after["status"], updates=list(o["updates"]), ops=ops))
    return res


def run_sequential(store, discovery, now_ms, max_same, intern=None):
    """one pass over a copy of the store -> (results as as_results gives them, the table's final status [W], its final endpoint
    column [W] under the interning of to_abi, the store after the pass)"""
    abi = to_abi(store, discovery, intern)
    after = {a: dict(n) for a, n in store.items()}
    outs = sequential_pass(after, discovery, now_ms, max_same)
    res = as_results(dict(outs=outs, discovery=discovery), store, after, now_ms)
    final_status = [after[a]["status"] for a in abi["addresses"]]
    final_endpoint = [abi["intern"](after[a]["ip_address"], after[a]["port"]) for a in abi["addresses"]]
    return res, final_status, final_endpoint, after, abi, outs


# ------------------------------------------------------------------------------------------------------------------ parallel

def row_rule(s, cnt, flags, last_change_ms, last_updated_ms, ip_differs, now_ms):
    """the steps 1-8 of include/pm_engine.h -> (final status, updates, ops)"""
    st = {"status": s, "updates": [], "ops": 0}

    def update(new):
        st["updates"].append((st["status"], new))
        st["status"] = new
        st["ops"] |= DO_STAMP_NOW

    def put_back(op):
        st["status"] = s
        st["ops"] = (st["ops"] & ~DO_STAMP_NOW) | op

    validated, white, active = bool(flags & DF_VALIDATED), bool(flags & DF_WHITELISTED), bool(flags & DF_ACTIVE)
    if cnt > 0 and s != HEALTHY:
        update(DEAD)
        return st["status"], st["updates"], st["ops"]
    if validated and not white:
        update(EJECTED)
    if validated and white and s == EJECTED:
        update(DEAD)
    if not active and s == HEALTHY:
        if last_change_ms == 0 or now_ms - last_change_ms > GRACE_MS:
            update(DEAD if white else EJECTED)
    if ip_differs:
        put_back(DO_IP_REWRITE)
    if flags & DF_LOCATION_NEW:
        st["ops"] |= DO_LOCATION
    if s == DEAD and last_change_ms != 0 and last_updated_ms != 0 and last_change_ms < last_updated_ms:
        if flags & DF_SPECS_DIFFER:
            put_back(DO_SPECS_REWRITE)
        update(DISCOVERED)
    if flags & DF_BALANCE_ZERO:
        update(LOWBALANCE)
    return st["status"], st["updates"], st["ops"]


def _endpoint_after(ops, endpoint_after, table_ep):
    return endpoint_after if (ops & DO_IP_REWRITE) and not (ops & DO_SPECS_REWRITE) else table_ep


def parallel_pass(status, row_endpoint, rows, now_ms, max_same):
    """cnt(j, k) = unlisted Healthy on k + listed Healthy on k still to come + listed, still Healthy, on k after their step
    -> (results, final status [W], final endpoint [W], events per endpoint: the segment lengths a test wants to know)"""
    W = len(status)
    pos = [None] * W
    for j, r in enumerate(rows):
        if r[0] != DISC_NEW:
            assert pos[r[0]] is None
            pos[r[0]] = j
    base, before, after = {}, {}, {}
    for w in range(W):
        if status[w] != HEALTHY:
            continue
        ep = row_endpoint[w]
        if pos[w] is None:
            if ep != EP_NONE:
                base[ep] = base.get(ep, 0) + 1
            continue
        _, _, ea, flags, lc, lu = rows[pos[w]]
        fin, _, ops = row_rule(HEALTHY, 0, flags, lc, lu, ea != ep, now_ms)
        if ep != EP_NONE:
            before.setdefault(ep, []).append(pos[w])
        if fin == HEALTHY:
            ep2 = _endpoint_after(ops, ea, ep)
            if ep2 != EP_NONE:
                after.setdefault(ep2, []).append(pos[w])
    res, final_status, final_endpoint = [], list(status), list(row_endpoint)
    for j, (row, k, ea, flags, lc, lu) in enumerate(rows):
        cnt = base.get(k, 0) + sum(1 for p in before.get(k, ()) if p > j) + sum(1 for p in after.get(k, ()) if p < j)
        if row == DISC_NEW:
            admit = cnt < max_same
            res.append(dict(cnt=cnt, old_status=N_STATUS, final_status=DISCOVERED if admit else N_STATUS, updates=[],
                            ops=DO_ADMIT if admit else DO_SKIP))
            continue
        fin, updates, ops = row_rule(status[row], cnt, flags, lc, lu, ea != row_endpoint[row], now_ms)
        res.append(dict(cnt=cnt, old_status=status[row], final_status=fin, updates=updates, ops=ops))
        final_status[row] = fin
        final_endpoint[row] = _endpoint_after(ops, ea, row_endpoint[row])
    seg = {k: len(before.get(k, ())) + len(after.get(k, ())) for k in set(before) | set(after)}
    return res, final_status, final_endpoint, seg


def count_once_differs(status, row_endpoint, rows, results, max_same):
    """the rows whose DECISION a count taken once at the start of the pass would change (the order-dependent rows)"""
    n = 0
    for (row, k, _, _, _, _), r in zip(rows, results):
        once = sum(1 for w in range(len(status)) if w != row and status[w] == HEALTHY and row_endpoint[w] == k)
        if row == DISC_NEW:
            n += (once >= max_same) != (r["cnt"] >= max_same)
        elif status[row] != HEALTHY:
            n += (once > 0) != (r["cnt"] > 0)
    return n


# ------------------------------------------------------------------------------------------------------------- seeded cases

def seeded_case(seed, W=None, D=None, n_ep=None):
    """a store and a discovery list: W and D at lane edges, endpoints from 1, 2, 4 or 16 ids, 70 % of the listed rows keep
    their endpoint, 3 % of the table rows are retired, stamps on both sides of the grace edge"""
    import random
    rng = random.Random(seed)
    now = 1_700_000_000_000
    W = W or rng.choice([1, 5, 63, 64, 65, 130, 257])
    D = D or rng.choice([1, 3, 63, 64, 65, 100])
    n_ep = n_ep or rng.choice([1, 2, 4, 16])
    eps = [("10.0.%d.%d" % (k // 4, k % 4), 8080 + (k % 2)) for k in range(n_ep)]
    max_same = rng.choice([0, 1, 2, 3])
    stamps = [None, now - GRACE_MS - 1, now - GRACE_MS, now - GRACE_MS + 1, now - 1000, now + 5000, now - 10 * GRACE_MS]
    nodes = []
    for w in range(W):
        ip, port = rng.choice(eps)
        if rng.random() < 0.03:
            ip = None
        st = HEALTHY if rng.random() < 0.55 else rng.choice([DISCOVERED, WAITING, UNHEALTHY, DEAD, DEAD, EJECTED, BANNED, LOWBALANCE])
        nodes.append(node("a%05d" % w, st, ip, port, rng.choice(stamps), rng.choice([None, "loc"]), rng.choice(["specs-a", "specs-b"])))
    store = make_store(nodes)
    listed = rng.sample(range(W), min(W, D, rng.randint(0, D)))
    discovery = []
    for w in listed:
        n = nodes[w]
        if n["ip_address"] is not None and rng.random() < 0.7:
            ip, port = n["ip_address"], n["port"]
        else:
            ip, port = rng.choice(eps)
        discovery.append(sighting(n["address"], ip, port, rng.random() < 0.9, rng.random() < 0.8, rng.random() < 0.7,
                                  rng.choice([None, "loc"]), rng.choice(["specs-a", "specs-b"]),
                                  rng.choice([None, now - 500, now - 2 * GRACE_MS]), rng.choice([None, None, None, 0, 7])))
    for k in range(D - len(listed)):
        ip, port = rng.choice(eps)
        discovery.append(sighting("n%05d" % k, ip, port, True, rng.random() < 0.8, True))
    rng.shuffle(discovery)
    return store, discovery, now, max_same


N_SEEDED = 400
