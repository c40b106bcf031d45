"""A literal, sequential model of the reference's metrics store and of the engine's metrics ledger.  No GPU, no numpy.

`Store` is the reference line by line, with its strings: MetricsStore (orchestrator/src/store/domains/metrics_store.rs:25-240),
the heartbeat route's stale-key deletion in front of the store (api/routes/heartbeat.rs:94-151), the status updater's clean-up
(status_update/mod.rs:314-343) and the sync service's list (metrics/sync_service.rs:127-200).  One dict per address stands for
the node's Redis hash: field "{task_id or "manual"}:{label without ':'}" -> value.

`Interner` is what a host does in front of the C ABI: the field becomes a dense series number, and the keep-the-maximum rule a
flag of the incoming entry (from the ORIGINAL label, metrics_store.rs:52).

`Ledger` is include/pm_engine.h "metrics ledger" beat by beat, entry by entry: what pm_metrics_ingest / _totals / _rows must
give, the row bound and the order of the sums included."""
import struct

ZERO = "0x0000000000000000000000000000000000000000"   # Address::ZERO: store_manual_metrics' node, the ledger's manual row
MANUAL, ROW_MAX = 0xFFFFFFFF, 1024
REPLACE, MERGE, DELETE = 0, 1, 2
F_MAX = 1
NONE = 0xFFFFFFFF


def bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def clean_label(label: str) -> str:                       # metrics_store.rs:21-23
    return label.replace(":", "")


def field_of(task_id: str, label: str) -> str:            # :43-49
    return f"{task_id if task_id else 'manual'}:{clean_label(label)}"


class Store:
    def __init__(self):
        self.nodes = {}                                   # address -> {field: value}

    # metrics_store.rs:25-75.  metrics: [(task_id, label, value)] or None
    def store_metrics(self, metrics, address):
        if metrics is None:                               # :30-32
            return
        if not metrics:                                   # :34-36
            return
        node = self.nodes.setdefault(address, {})
        for task_id, label, value in metrics:             # :42
            key = field_of(task_id, label)                # :43-49
            if "dashboard-progress" in label:             # :52 (the original label)
                if key in node:                           # :53-58 (a stored value always parses: it was written as an f64)
                    should_update = value > node[key]
                else:
                    should_update = True                  # :59
            else:
                should_update = True                      # :62
            if should_update:                             # :65-72
                node[key] = value

    def store_manual_metrics(self, label, value):         # :77-89
        self.store_metrics([("", label, value)], ZERO)

    def delete_metric(self, task_id, label, address):     # :91-109
        key = f"{task_id}:{clean_label(label)}"
        return self.nodes.get(address, {}).pop(key, None) is not None

    def get_metric_keys_for_node(self, address):          # :133-140
        return list(self.nodes.get(address, {}))

    # api/routes/heartbeat.rs:94-151.  metrics None = the beat carried none: nothing happens
    def heartbeat(self, address, metrics):
        if metrics is None:                               # :94
            return
        previous = self.get_metric_keys_for_node(address)                 # :96-107
        new_set = {field_of(t, lab) for t, lab, _ in metrics}             # :110-120
        stale = [k for k in previous if k not in new_set]                 # :123-126
        for key in stale:                                                 # :129-140
            task_id, _, label = key.partition(":")
            self.delete_metric(task_id, label, address)
        self.store_metrics(list(metrics), address)                        # :143-150

    # status_update/mod.rs:314-343: a node that became Dead, Ejected or Banned loses every metric
    def clear_node(self, address):
        for key in self.get_metric_keys_for_node(address):
            task_id, _, label = key.partition(":")
            self.delete_metric(task_id, label, address)

    def get_metrics_for_node(self, address):              # :111-131 -> {task: {name: value}}
        out = {}
        for key, value in self.nodes.get(address, {}).items():
            task_id, sep, name = key.partition(":")
            if sep:
                out.setdefault(task_id, {})[name] = value
        return out

    def get_aggregate_metrics_for_task(self, task_id, order=None):   # :143-174
        out = {}
        for address in (order if order is not None else self.nodes):
            for key, value in self.nodes.get(address, {}).items():
                t, sep, name = key.partition(":")
                if sep and t == task_id:
                    out[name] = out.get(name, 0.0) + value
        return out

    def get_aggregate_metrics_for_all_tasks(self, order=None):       # :176-202
        out = {}
        for address in (order if order is not None else self.nodes):
            for key, value in self.nodes.get(address, {}).items():
                _, sep, name = key.partition(":")
                if sep:
                    out[name] = out.get(name, 0.0) + value
        return out

    def get_all_metrics(self):                            # :204-240 -> {task: {name: {address: value}}}
        out = {}
        for address, node in self.nodes.items():
            for key, value in node.items():
                task_id, sep, name = key.partition(":")
                if sep:
                    out.setdefault(task_id, {}).setdefault(name, {})[address] = value
        return out

    # sync_service.rs:127-200: (address, task_id, task name or "unknown", label, value, group id or None, config name or None)
    def synced_metrics(self, task_names, group_of_address):
        out = []
        for task_id, by_name in self.get_all_metrics().items():
            for name, by_node in by_name.items():
                for address, value in by_node.items():
                    gid, cfg = group_of_address.get(address, (None, None))
                    out.append((address, task_id, task_names.get(task_id, "unknown"), name, value, gid, cfg))
        return out

    def fields(self):
        """{address: {field: value}} without the empty hashes (Redis holds none)"""
        return {a: dict(n) for a, n in self.nodes.items() if n}


class Interner:
    def __init__(self):
        self.ids, self.keys = {}, []                      # field -> series; series -> (task_id or "manual", cleaned label)

    def series(self, task_id, label):
        key = field_of(task_id, label)
        if key not in self.ids:
            self.ids[key] = len(self.keys)
            self.keys.append((task_id if task_id else "manual", clean_label(label)))
        return self.ids[key]

    def entry(self, task_id, label, value):
        """(series, flags, value): the flag from the ORIGINAL label"""
        return (self.series(task_id, label), F_MAX if "dashboard-progress" in label else 0, value)

    def lookup(self, task_id, label):
        """delete_metric's key (no "manual" substitution, :100): the series, or None if no such field was ever stored"""
        return self.ids.get(f"{task_id}:{clean_label(label)}")

    def field(self, series):
        t, lab = self.keys[series]
        return f"{t}:{lab}"

    @property
    def n_series(self):
        return len(self.keys)


class Refused(Exception):
    pass


class Ledger:
    """rows: {row: {series: value}}, row = a worker index or MANUAL"""

    def __init__(self):
        self.rows = {}
        self.n_series = 0

    def ingest(self, beats, entries, n_series):
        """beats: [(row, kind, first, n)], entries: [(series, flags, value)].  Raises Refused, the ledger as it was, if a
        row would hold more than ROW_MAX series at any moment."""
        new = {r: dict(v) for r, v in self.rows.items()}
        for row, kind, first, n in beats:
            ents = entries[first:first + n]
            assert all(s < n_series for s, _, _ in ents)
            node = new.setdefault(row, {})
            if kind == DELETE:
                for s, _, _ in ents:
                    node.pop(s, None)
                continue
            if kind == REPLACE:
                named = {s for s, _, _ in ents}
                for s in [s for s in node if s not in named]:
                    del node[s]
            for s, flags, value in ents:
                if s not in node:
                    if len(node) >= ROW_MAX:
                        raise Refused()
                    node[s] = value
                elif not (flags & F_MAX) or value > node[s]:
                    node[s] = value
        self.rows = new
        self.n_series = max(self.n_series, n_series)

    def order(self):
        return ([MANUAL] if MANUAL in self.rows else []) + sorted(r for r in self.rows if r != MANUAL)

    def totals(self):
        """(sums, counts) per series: from +0.0, one value after the other in ascending row order, the manual row first"""
        sums, counts = [0.0] * self.n_series, [0] * self.n_series
        for r in self.order():
            for s, v in self.rows[r].items():
                sums[s] += v
                counts[s] += 1
        return sums, counts

    def listing(self, rows=None):
        """[(row, series, value)]: every entry, the manual row first, then ascending (worker, series) — or the named rows"""
        out = []
        for r in (self.order() if rows is None else rows):
            out += [(r, s, self.rows[r][s]) for s in sorted(self.rows.get(r, {}))]
        return out

    def clear_workers(self):
        self.rows = {r: v for r, v in self.rows.items() if r == MANUAL}

    def clear_row(self, row):
        self.rows.pop(row, None)


class Host:
    """A Store's calls turned into ledger batches, as a host in front of the C ABI would: an address book (ZERO is the manual
    row), the interner, a queue."""

    def __init__(self, addresses):
        self.row_of = {a: w for w, a in enumerate(addresses)}
        self.row_of[ZERO] = MANUAL
        self.intern = Interner()
        self.beats, self.entries = [], []

    def _queue(self, address, kind, ents):
        self.beats.append((self.row_of[address], kind, len(self.entries), len(ents)))
        self.entries += ents

    def heartbeat(self, address, metrics):
        if metrics is not None:
            self._queue(address, REPLACE, [self.intern.entry(*m) for m in metrics])

    def store_metrics(self, metrics, address):
        if metrics:
            self._queue(address, MERGE, [self.intern.entry(*m) for m in metrics])

    def store_manual_metrics(self, label, value):
        self.store_metrics([("", label, value)], ZERO)

    def delete_metric(self, task_id, label, address):
        s = self.intern.lookup(task_id, label)
        if s is not None and address in self.row_of:
            self._queue(address, DELETE, [(s, 0, 0.0)])

    def clear_node(self, address):
        self._queue(address, REPLACE, [])

    def take(self):
        out = (self.beats, self.entries, max(self.intern.n_series, 1))
        self.beats, self.entries = [], []
        return out

    def fields(self, listing):
        """a ledger listing [(row, series, value)] as Store.fields() gives it"""
        addr = {w: a for a, w in self.row_of.items()}
        out = {}
        for r, s, v in listing:
            out.setdefault(addr[r], {})[self.intern.field(s)] = v
        return out


def same_fields(a, b) -> bool:
    """two {address: {field: value}} with the values compared bit for bit"""
    return {k: {f: bits(v) for f, v in n.items()} for k, n in a.items()} == \
           {k: {f: bits(v) for f, v in n.items()} for k, n in b.items()}
