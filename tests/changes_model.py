"""The contract of the assignment change feed (include/pm_engine.h "assignment change feed"), in plain Python: what the GPU
tests judge the engine by.

A TABLE is a list with one entry per worker: (group_id, group_index, group_size, next_worker, task) — task the task's own
identity (its uid) or None — or NO_GROUP for a worker in no group.  group_slot and the task's position are not in it."""
from __future__ import annotations

NONE = 0xFFFFFFFF
GROUP, RING, TASK = 1, 2, 4
ALL = GROUP | RING | TASK
NO_GROUP = (0, 0, 0, NONE, None)


def what(prev, cur) -> int:
    """the bits of one row at one publish"""
    bits = 0
    if prev[0] != cur[0]:
        bits |= GROUP
    if prev[1:4] != cur[1:4]:
        bits |= RING
    if prev[4] != cur[4]:
        bits |= TASK
    return bits


def diff(prev: list, cur: list) -> list:
    """per-row bits of the publish `cur` against the publish `prev`; rows `prev` does not have compare against NO_GROUP"""
    assert len(prev) <= len(cur), "rows are only appended between two publishes without a resync"
    return [what(prev[w] if w < len(prev) else NO_GROUP, cur[w]) for w in range(len(cur))]


def row_of(group_slot, group_id, group_index, group_size, next_worker, task_identity):
    """a published row (pm_assignment, the task's position already turned into the task's identity) as a table entry"""
    if group_slot == NONE:
        return NO_GROUP
    return (int(group_id), int(group_index), int(group_size), int(next_worker), task_identity)


class Feed:
    """the feed's state: the table remembered from the last publish, the pending bits, the two resync flags"""

    def __init__(self):
        self.prev = None          # None: the remembered table is invalid (enable, or one of the resync events)
        self.pending = []         # what(w), accumulated since the last drain
        self.resync_flag = False  # the next drain reports RESYNC

    def resync(self):
        self.prev = None

    def publish(self, table: list):
        table = list(table)
        if self.prev is None:     # every row [0, W) with all three bits; marks of an older, longer table are gone
            self.pending = [ALL] * len(table)
            self.resync_flag = True
        else:
            bits = diff(self.prev, table)
            self.pending += [0] * (len(table) - len(self.pending))
            self.pending = [p | b for p, b in zip(self.pending, bits)]
        self.prev = table

    def drain(self):
        """-> ([(worker, what)] ascending, resync)"""
        rows = [(w, b) for w, b in enumerate(self.pending) if b]
        flag = self.resync_flag
        self.pending = [0] * len(self.pending)
        self.resync_flag = False
        return rows, flag


# ---- the drain's list as the device makes it: a per-word prefix over popcounts, then the expansion

def bitmap_of(what_bytes: list) -> list:
    """the pending bitmap of a `what` column: bit w of word w // 64 <=> what[w] != 0"""
    words = [0] * ((len(what_bytes) + 63) // 64)
    for w, b in enumerate(what_bytes):
        if b:
            words[w >> 6] |= 1 << (w & 63)
    return words


def word_prefix(words: list, words_per_thread: int = 4, threads: int = 256) -> tuple:
    """(exclusive prefix of the words' popcounts, total) the way one workgroup scans them: passes of threads * words_per_thread
    words, a thread's words in a row, the threads' sums scanned, the running total carried from pass to pass"""
    prefix, acc = [0] * len(words), 0
    tile = words_per_thread * threads
    for base in range(0, len(words), tile):
        sums = []
        for t in range(threads):
            j0 = base + t * words_per_thread
            sums.append(sum(bin(words[j]).count("1") for j in range(j0, min(j0 + words_per_thread, len(words)))))
        before = 0
        for t in range(threads):
            at = acc + before
            j0 = base + t * words_per_thread
            for j in range(j0, min(j0 + words_per_thread, len(words))):
                prefix[j] = at
                at += bin(words[j]).count("1")
            before += sums[t]
        acc += before
    return prefix, acc


def expand(words: list, prefix: list, what_bytes: list, total: int) -> list:
    """[(worker, what)]: bit b of word j lands at prefix[j] + (set bits of word j below b)"""
    out = [None] * total
    for j, word in enumerate(words):
        for b in range(64):
            if (word >> b) & 1:
                at = prefix[j] + bin(word & ((1 << b) - 1)).count("1")
                assert out[at] is None, "two rows in one place"
                out[at] = (j * 64 + b, what_bytes[j * 64 + b])
    assert all(r is not None for r in out), "a place of the list was not written"
    return out


def drain_list(what_bytes: list) -> list:
    words = bitmap_of(what_bytes)
    prefix, total = word_prefix(words)
    return expand(words, prefix, what_bytes, total)
