"""Named cases of the metrics ledger: a few calls of the reference's store and what its hashes hold afterwards, written down
by hand.  An op is ("beat", address, metrics) — the heartbeat route, ("store", address, metrics) — store_metrics alone,
("manual", label, value), ("delete", task_id, label, address), ("clear", address) — the status updater's clean-up, or
("flush",) — where a host that queues would send its batch (a case without one is ONE batch).  metrics: [(task_id, label,
value)].  `want` is {address: {field: value}}, compared bit for bit.  tests/test_metrics_model.py holds both models to the
`want`s; tests/test_gpu_metrics.py runs every case through the engine."""
from metrics_model import ZERO

A, B = "0x00000000000000000000000000000000000000aa", "0x00000000000000000000000000000000000000bb"
ADDRESSES = [A, B]
NAN = float("nan")
P = "dashboard-progress/step"       # a keep-the-maximum label
T = "task-1"


def case(name, ops, want):
    return dict(name=name, ops=ops, want=want)


CASES = [
    # ---- MAX against a lower, an equal and a higher stored value
    case("max lower keeps", [("beat", A, [(T, P, 5.0)]), ("beat", A, [(T, P, 4.0)])], {A: {f"{T}:{P}": 5.0}}),
    case("max equal keeps", [("beat", A, [(T, P, 5.0)]), ("beat", A, [(T, P, 5.0)])], {A: {f"{T}:{P}": 5.0}}),
    case("max higher sets", [("beat", A, [(T, P, 5.0)]), ("beat", A, [(T, P, 6.0)])], {A: {f"{T}:{P}": 6.0}}),
    # ---- NaN and the zeroes
    case("max against a stored NaN keeps the NaN", [("store", A, [(T, P, NAN)]), ("store", A, [(T, P, 7.0)])], {A: {f"{T}:{P}": NAN}}),
    case("max with a NaN keeps the number", [("store", A, [(T, P, 7.0)]), ("store", A, [(T, P, NAN)])], {A: {f"{T}:{P}": 7.0}}),
    case("max NaN into an absent series is stored", [("store", A, [(T, P, NAN)])], {A: {f"{T}:{P}": NAN}}),
    case("max 0.0 does not replace -0.0", [("store", A, [(T, P, -0.0)]), ("store", A, [(T, P, 0.0)])], {A: {f"{T}:{P}": -0.0}}),
    case("max -0.0 does not replace 0.0", [("store", A, [(T, P, 0.0)]), ("store", A, [(T, P, -0.0)])], {A: {f"{T}:{P}": 0.0}}),
    case("set replaces a NaN", [("store", A, [(T, "loss", NAN)]), ("store", A, [(T, "loss", 1.5)])], {A: {f"{T}:loss": 1.5}}),
    # ---- one series three times in one beat: MAX, then SET (the label with a colon: no "dashboard-progress" in it), then MAX
    case("max set max in one beat",
         [("beat", A, [(T, "dashboard-progress", 9.0), (T, "dashboard:-progress", 2.0), (T, "dashboard-progress", 3.0)])],
         {A: {f"{T}:dashboard-progress": 3.0}}),
    case("max set max in one beat, the last lower",
         [("beat", A, [(T, "dashboard-progress", 9.0), (T, "dashboard:-progress", 2.0), (T, "dashboard-progress", 1.0)])],
         {A: {f"{T}:dashboard-progress": 2.0}}),
    # ---- REPLACE drops a MAX series, a later beat brings it back lower
    case("replace drops a max series, re-added lower",
         [("beat", A, [(T, P, 8.0)]), ("beat", A, [(T, "loss", 1.0)]), ("beat", A, [(T, P, 2.0)])],
         {A: {f"{T}:{P}": 2.0}}),
    case("three beats of one row, the middle one lacks the series",
         [("beat", A, [(T, P, 8.0), (T, "loss", 3.0)]), ("beat", A, [(T, "loss", 2.0)]), ("beat", A, [(T, P, 1.0), (T, "loss", 1.0)])],
         {A: {f"{T}:{P}": 1.0, f"{T}:loss": 1.0}}),
    case("three beats of one row across two batches",
         [("beat", A, [(T, P, 8.0), (T, "loss", 3.0)]), ("flush",), ("beat", A, [(T, "loss", 2.0)]), ("beat", A, [(T, P, 1.0)])],
         {A: {f"{T}:{P}": 1.0}}),
    # ---- MERGE onto a REPLACE
    case("merge onto a replace",
         [("beat", A, [(T, "loss", 1.0), (T, P, 4.0)]), ("store", A, [(T, "lr", 0.5), (T, P, 3.0), (T, "loss", 0.25)])],
         {A: {f"{T}:loss": 0.25, f"{T}:{P}": 4.0, f"{T}:lr": 0.5}}),
    case("replace after a merge drops what the merge added",
         [("store", A, [(T, "lr", 0.5)]), ("beat", A, [(T, "loss", 1.0)])], {A: {f"{T}:loss": 1.0}}),
    # ---- DELETE
    case("delete of an absent series", [("beat", A, [(T, "loss", 1.0)]), ("beat", B, [(T, "lr", 2.0)]), ("delete", T, "lr", A)],
         {A: {f"{T}:loss": 1.0}, B: {f"{T}:lr": 2.0}}),
    case("delete of a series nobody ever stored", [("beat", A, [(T, "loss", 1.0)]), ("delete", T, "never", A)], {A: {f"{T}:loss": 1.0}}),
    case("delete then a max entry starts over", [("beat", A, [(T, P, 8.0)]), ("delete", T, P, A), ("store", A, [(T, P, 1.0)])],
         {A: {f"{T}:{P}": 1.0}}),
    case("delete cleans its label too", [("beat", A, [(T, "a:b", 1.0), (T, "c", 2.0)]), ("delete", T, "a:b", A)], {A: {f"{T}:c": 2.0}}),
    # ---- the empty REPLACE, the absent metrics
    case("empty replace empties the row", [("beat", A, [(T, "loss", 1.0), (T, P, 2.0)]), ("beat", B, [(T, "loss", 5.0)]), ("beat", A, [])],
         {B: {f"{T}:loss": 5.0}}),
    case("a beat without metrics changes nothing", [("beat", A, [(T, "loss", 1.0)]), ("beat", A, None)], {A: {f"{T}:loss": 1.0}}),
    case("an empty store changes nothing", [("beat", A, [(T, "loss", 1.0)]), ("store", A, [])], {A: {f"{T}:loss": 1.0}}),
    case("the clean-up of a dead node", [("beat", A, [(T, "loss", 1.0)]), ("beat", B, [(T, "loss", 2.0)]), ("clear", A)],
         {B: {f"{T}:loss": 2.0}}),
    # ---- the manual row
    case("manual entries", [("manual", "uptime", 3.0), ("manual", "uptime", 2.0), ("manual", "dashboard-progress", 5.0),
                            ("manual", "dashboard-progress", 4.0), ("beat", A, [("", "uptime", 7.0)])],
         {ZERO: {"manual:uptime": 2.0, "manual:dashboard-progress": 5.0}, A: {"manual:uptime": 7.0}}),
    case("a manual entry survives the workers' beats", [("manual", "uptime", 3.0), ("beat", A, [(T, "loss", 1.0)]), ("beat", A, [])],
         {ZERO: {"manual:uptime": 3.0}}),
    # ---- one series, two labels, two rules
    case("dashboard:-progress sets where dashboard-progress keeps",
         [("store", A, [(T, "dashboard-progress", 9.0)]), ("store", B, [(T, "dashboard-progress", 9.0)]),
          ("store", A, [(T, "dashboard:-progress", 1.0)]), ("store", B, [(T, "dashboard-progress", 1.0)])],
         {A: {f"{T}:dashboard-progress": 1.0}, B: {f"{T}:dashboard-progress": 9.0}}),
]
