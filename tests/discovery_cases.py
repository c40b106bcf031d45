"""Named cases for the discovery sync: every arm and every put-back of sync_single_node_with_discovery
(discovery/monitor.rs:236-420), each with its hand-written outcome.  A case is a store, a discovery list, the constructor's
max and, per discovery row, want = (final status | "admit" | "skip", [(old, new) of every update], the row's ip after the pass).
The model test holds both formulations of tests/discovery_model.py to them, the GPU test the engine."""
from discovery_model import (node, sighting, GRACE_MS, DISCOVERED, WAITING, HEALTHY, UNHEALTHY, DEAD, EJECTED, BANNED, LOWBALANCE)

NOW_MS = 1_700_000_000_000
A, B, C, N1, N2 = "addr-a", "addr-b", "addr-c", "new-1", "new-2"
X, Y = "10.0.0.1", "10.0.0.2"
OLD = NOW_MS - 10 * GRACE_MS


def case(name, store, discovery, want, max_same=1):
    assert len(discovery) == len(want)
    return dict(name=name, store=store, discovery=discovery, want=want, max=max_same, now=NOW_MS)


def _grace(name, stamp, want):
    return case(name, [node(A, HEALTHY, X, stamp=stamp)], [sighting(A, X, active=False)], [want])


CASES = [
    # ---- the issue's list
    case("healthy not whitelisted, ip changed: one Ejected update, put back, ends Healthy on the new ip",
         [node(A, HEALTHY, X, stamp=OLD)], [sighting(A, Y, whitelisted=False)], [(HEALTHY, [(HEALTHY, EJECTED)], Y)]),
    case("dead, ip and specs changed: the specs put-back restores the OLD ip, then Discovered",
         [node(A, DEAD, X, stamp=NOW_MS - 1000, specs="specs-a")], [sighting(A, Y, specs="specs-b", last_updated=NOW_MS - 500)],
         [(DISCOVERED, [(DEAD, DISCOVERED)], X)]),
    _grace("grace: 299,999 ms is inside", NOW_MS - 299_999, (HEALTHY, [], X)),
    _grace("grace: 300,000 ms is inside (strict)", NOW_MS - 300_000, (HEALTHY, [], X)),
    _grace("grace: 300,001 ms is over", NOW_MS - 300_001, (DEAD, [(HEALTHY, DEAD)], X)),
    _grace("grace: a stamp in the future never marks", NOW_MS + 60_000, (HEALTHY, [], X)),
    _grace("grace: no stamp marks", None, (DEAD, [(HEALTHY, DEAD)], X)),
    case("three updates: not whitelisted, inactive, zero balance",
         [node(A, HEALTHY, X)], [sighting(A, X, whitelisted=False, active=False, balance=0)],
         [(LOWBALANCE, [(HEALTHY, EJECTED), (EJECTED, EJECTED), (EJECTED, LOWBALANCE)], X)]),
    case("max = 0 admits nobody", [], [sighting(N1, X)], [("skip", [], None)], max_same=0),
    case("a port-only difference is no rewrite",
         [node(A, HEALTHY, X, 8080, stamp=OLD)], [sighting(A, X, 9090)], [(HEALTHY, [], X)]),
    # ---- the remaining arms
    case("a healthy node on the endpoint: the other one dies, and nothing else of its row happens",
         [node(A, HEALTHY, X), node(B, DISCOVERED, X)], [sighting(B, X, whitelisted=False, balance=0)],
         [(DEAD, [(DISCOVERED, DEAD)], X)]),
    case("ejected and whitelisted again: Dead, so that it can recover",
         [node(A, EJECTED, X)], [sighting(A, X, active=False)], [(DEAD, [(EJECTED, DEAD)], X)]),
    case("inactive and not whitelisted (not validated): Ejected",
         [node(A, HEALTHY, X)], [sighting(A, X, validated=False, whitelisted=False, active=False)],
         [(EJECTED, [(HEALTHY, EJECTED)], X)]),
    case("a location where there was none: reported, no update",
         [node(A, HEALTHY, X, stamp=OLD)], [sighting(A, X, location="loc")], [(HEALTHY, [], X)]),
    case("dead and updated on discovery since: Discovered",
         [node(A, DEAD, X, stamp=NOW_MS - 1000)], [sighting(A, X, last_updated=NOW_MS - 500)],
         [(DISCOVERED, [(DEAD, DISCOVERED)], X)]),
    case("dead and not updated since: stays",
         [node(A, DEAD, X, stamp=NOW_MS - 500)], [sighting(A, X, last_updated=NOW_MS - 500)], [(DEAD, [], X)]),
    case("dead without either stamp: stays",
         [node(A, DEAD, X, stamp=None), node(B, DEAD, Y, stamp=NOW_MS - 500)],
         [sighting(A, X, last_updated=NOW_MS - 100), sighting(B, Y, last_updated=None)], [(DEAD, [], X), (DEAD, [], Y)]),
    case("zero balance: LowBalance", [node(A, HEALTHY, X, stamp=OLD)], [sighting(A, X, balance=0)],
         [(LOWBALANCE, [(HEALTHY, LOWBALANCE)], X)]),
    case("a balance that is not zero", [node(A, UNHEALTHY, X)], [sighting(A, X, balance=7)], [(UNHEALTHY, [], X)]),
    case("dead, not whitelisted, ip changed, updated since: Ejected is put back, then Discovered on the new ip",
         [node(A, DEAD, X, stamp=NOW_MS - 1000)], [sighting(A, Y, whitelisted=False, last_updated=NOW_MS - 500)],
         [(DISCOVERED, [(DEAD, EJECTED), (DEAD, DISCOVERED)], Y)]),
    case("waiting and banned rows pass through", [node(A, WAITING, X), node(B, BANNED, Y)],
         [sighting(A, X), sighting(B, Y)], [(WAITING, [], X), (BANNED, [], Y)]),
    # ---- admissions and the threshold
    case("new and alone: admitted", [], [sighting(N1, X)], [("admit", [], X)]),
    case("the reference's same-endpoint test: same port skipped, other port admitted",
         [node(A, HEALTHY, "127.0.0.1", 8080)], [sighting(N1, "127.0.0.1", 8080), sighting(N2, "127.0.0.1", 8081)],
         [("skip", [], None), ("admit", [], "127.0.0.1")]),
    case("max = 2: one healthy is below, two are on it",
         [node(A, HEALTHY, X), node(B, HEALTHY, Y), node(C, HEALTHY, Y)], [sighting(N1, X), sighting(N2, Y)],
         [("admit", [], X), ("skip", [], None)], max_same=2),
    case("an admitted node is Discovered: the next new one on the endpoint is admitted too",
         [], [sighting(N1, X), sighting(N2, X)], [("admit", [], X), ("admit", [], X)]),
    # ---- order
    case("a demotion at position 1: the query before it sees the node, the one behind it does not",
         [node(A, HEALTHY, X)], [sighting(N1, X), sighting(A, X, active=False), sighting(N2, X)],
         [("skip", [], None), (DEAD, [(HEALTHY, DEAD)], X), ("admit", [], X)]),
    case("an ip move X -> Y at position 2: X is taken before and free behind, Y the other way round",
         [node(A, HEALTHY, X, stamp=OLD), node(B, UNHEALTHY, X), node(C, UNHEALTHY, Y)],
         [sighting(N1, X), sighting(N2, Y), sighting(A, Y), sighting(B, X), sighting(C, Y)],
         [("skip", [], None), ("admit", [], Y), (HEALTHY, [], Y), (UNHEALTHY, [], X), (DEAD, [(UNHEALTHY, DEAD)], Y)]),
    case("a retired row gains an endpoint by the rewrite and counts there from then on",
         [node(A, HEALTHY, None, stamp=OLD)], [sighting(N1, X), sighting(A, X), sighting(N2, X)],
         [("admit", [], X), (HEALTHY, [], X), ("skip", [], None)]),
    case("a node never counts itself", [node(A, UNHEALTHY, X), node(B, HEALTHY, Y)], [sighting(A, X), sighting(B, Y)],
         [(UNHEALTHY, [], X), (HEALTHY, [], Y)]),
]
