// pm_engine_types.inc — part of pm_engine.cpp (one translation unit; included in place): SiteMap, Group, PubTable, KeySort, and
// ListPage with the two steps the directories share (inside namespace pm; DevBuf and the other owning types: pm_owned.h).
// coordinates -> site id: an open-addressing table (linear probing, load <= 1/2) of the (lat, lon) bit patterns.  A node table
// of 100k rows interns a thousand new rows per churn tick: a node-per-entry std::unordered_map spent 80 ns an insertion on
// its allocations.
struct SiteMap {
  std::vector<uint64_t> ka, kb;
  std::vector<uint32_t> val;  // id + 1; 0 = empty slot
  size_t count = 0;
  size_t size() const { return count; }
  void clear() {
    std::fill(val.begin(), val.end(), 0u);
    count = 0;
  }
  void reserve(size_t n) {
    size_t cap = 64;
    while (cap < 2 * n) cap <<= 1;
    if (cap > val.size()) rehash(cap);
  }
  // (a look-up is up to three dependent misses of the host's caches — 65 ns a row of a thousand-row delta, two thirds of an
  // append: whoever interns a batch asks for the slots of the rows a few places ahead first)
  void prefetch(uint64_t a, uint64_t b) const {
    if (val.empty()) return;
    const size_t i = size_t(splitmix64_mix(a ^ splitmix64_mix(b))) & (val.size() - 1);
    __builtin_prefetch(&val[i]);
    __builtin_prefetch(&ka[i]);
    __builtin_prefetch(&kb[i]);
  }
  // the id of (a, b); a pair seen for the first time gets id size()
  uint32_t find_or_insert(uint64_t a, uint64_t b) {
    if (2 * (count + 1) > val.size()) rehash(val.empty() ? 64 : val.size() * 2);
    const size_t mask = val.size() - 1;
    size_t i = size_t(splitmix64_mix(a ^ splitmix64_mix(b))) & mask;
    for (;; i = (i + 1) & mask) {
      if (!val[i]) {
        ka[i] = a, kb[i] = b;
        val[i] = uint32_t(++count);
        return uint32_t(count - 1);
      }
      if (ka[i] == a && kb[i] == b) return val[i] - 1u;
    }
  }

 private:
  void rehash(size_t cap) {
    std::vector<uint64_t> oa, ob;
    std::vector<uint32_t> ov;
    oa.swap(ka), ob.swap(kb), ov.swap(val);
    ka.assign(cap, 0), kb.assign(cap, 0), val.assign(cap, 0u);
    const size_t mask = cap - 1;
    for (size_t j = 0; j < ov.size(); ++j) {
      if (!ov[j]) continue;
      size_t i = size_t(splitmix64_mix(oa[j] ^ splitmix64_mix(ob[j]))) & mask;
      while (val[i]) i = (i + 1) & mask;
      ka[i] = oa[j], kb[i] = ob[j], val[i] = ov[j];
    }
  }
};

struct Group {
  uint64_t id;
  uint32_t cfg;
  uint32_t task;      // index into the current task table or PM_NONE
  uint64_t task_uid;  // identity of the claimed task across uploads
  MemberList members;  // carve order; BTreeSet order is derived from addr_rank (pm_members.h: small lists need no heap)
  bool dead = false;              // dissolved, not yet removed from the list (compact_groups)
};

// Published assignment table: two buffers, each guarded by a sequence counter (seqlock).  pm_tick writes the
// buffer that is NOT current, then flips `pub_cur`; a reader copies its 32-byte row with relaxed atomic loads
// between two reads of the buffer's counter and retries if the counter moved or was odd.  A buffer is rewritten
// only by the publish AFTER the next one, so a retry needs two publishes within one row copy.  No lock, no
// reference count, no allocation on the read path.  Buffers only grow; replaced allocations are retired, not
// freed, until the engine is destroyed (a reader may still hold the old pointer — its sequence check fails).
struct PubTable {
  std::atomic<uint64_t> seq{0};
  std::atomic<uint64_t*> words{nullptr};  // 4 x u64 per row (pm_assignment is 32 bytes, 8-byte aligned)
  PinBuf<uint64_t> own;                   // ... and their owner: what `words` points to (pub_buffer moves a replaced one to pub_retired)
  std::atomic<uint32_t> n{0};
  std::atomic<uint32_t> task_shift{0};  // added to every task position read from this buffer: tasks inserted in front
                                        // of the list since it was written (pm_tasks_insert_front) move them all alike
  std::atomic<uint32_t> cleared{0};     // the groups the rows name are gone (pm_reset_groups): every row reads as "no
                                        // group, no task" until the next publish
  size_t cap_rows = 0;
};
static_assert(sizeof(pm_assignment) == 32, "published rows are copied as four 64-bit words");
static_assert(offsetof(pm_assignment, task) == 0 && offsetof(pm_assignment, group_slot) == 4 && offsetof(pm_assignment, group_index) == 8 &&
                  offsetof(pm_assignment, group_size) == 12 && offsetof(pm_assignment, next_worker) == 16 &&
                  offsetof(pm_assignment, group_id) == 24,
              "the words pub_patch clears in place");

// The buffers of a key sort by launch_ro_radix_sort (pm_device.h): keys and side words, ping-pong, and a pass's histogram and
// its scan.  What the rollout ledger, the three directories and the address book each hold one of.
struct KeySort {
  DevBuf<uint64_t> key[2];
  DevBuf<uint32_t> val[2], hist, hist_scan;
  // buffer 0 alone: for a caller that fills it before it knows whether it sorts
  hipError_t ensure_first(size_t n) {
    const hipError_t e = key[0].ensure(n ? n : 1);
    return e != hipSuccess ? e : val[0].ensure(n ? n : 1);
  }
  // both pairs, and the histograms of n keys: [256][chunks] and one word more for the scan — the host's one statement of the
  // chunks launch_ro_radix_pass works in
  hipError_t ensure(size_t n) {
    const size_t chunks = (n + PM_RO_CHUNK - 1u) / PM_RO_CHUNK;
    hipError_t e = ensure_first(n);
    if (e == hipSuccess) e = key[1].ensure(n);
    if (e == hipSuccess) e = val[1].ensure(n);
    if (e == hipSuccess) e = hist.ensure(256 * chunks);
    if (e == hipSuccess) e = hist_scan.ensure(256 * chunks + 1);
    return e;
  }
  RoSortBufs bufs() const { return RoSortBufs{{key[0].p, key[1].p}, {val[0].p, val[1].p}, hist.p, hist_scan.p}; }
  // `passes` stable passes from the low byte over the n keys of buffer `cur`; returns the buffer that holds the result
  uint32_t sort(uint32_t n, uint32_t passes, uint32_t cur, hipStream_t s) const { return launch_ro_radix_sort(bufs(), n, passes, cur, s); }
};

// What the three directories page a list with: one flag per entry of the index space and class, their scan (a listed entry's
// place in scan order; the total behind the last flag), and the window — written by the places in scan order, a slice of the
// sorted entries in a sorted order.
struct ListPage {
  DevBuf<uint32_t> flag, off;  // [flags] (+ 1)
  DevBuf<uint32_t> win;        // scan order: the window's entries
  KeySort sort;                // a sorted order: keys and entries
  PinBuf<uint32_t> h_pin;      // [0] the scan's total, [1, 1 + n_census) the census
  // the pinned words of a call, zeroed: what a call with nothing to scan reports
  hipError_t pin(size_t n_census) {
    const hipError_t e = h_pin.ensure(1 + n_census, 1 + n_census);
    if (e == hipSuccess) std::memset(h_pin.p, 0, (1 + n_census) * sizeof(uint32_t));
    return e;
  }
};

// The counters step, behind the kernels that wrote the flags and the census: the scan, the census to h_pin[1..], ONE
// synchronisation.  *n_listed: the scan's total.
static int32_t page_counters(ListPage& pg, uint32_t n_flag, const uint32_t* census, uint32_t n_census, hipStream_t s, uint32_t* n_listed) {
  launch_mx_scan(pg.flag.p, n_flag, pg.off.p, pg.h_pin.p, s);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(pg.h_pin.p + 1, census, n_census * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *n_listed = pg.h_pin.p[0];
  return PM_OK;
}

// The list step: *list = the device's n entries of the window [offset, offset + n) of the n_listed listed ones.  passes == 0
// is scan order: window(win) has the entries whose place falls in the window write themselves.  Otherwise keys(key, val) has
// every listed entry write its key and itself at its place, and `passes` stable radix passes order them.
template <class Window, class Keys>
static int32_t page_list(ListPage& pg, uint32_t n_listed, uint32_t offset, uint32_t n, uint32_t passes, hipStream_t s, Window window,
                         Keys keys, const uint32_t** list) {
  if (!passes) {
    HIPCHK(pg.win.ensure(n));
    window(pg.win.p);
    *list = pg.win.p;
  } else {
    HIPCHK(pg.sort.ensure(n_listed));
    keys(pg.sort.key[0].p, pg.sort.val[0].p);
    *list = pg.sort.val[pg.sort.sort(n_listed, passes, 0u, s)].p + offset;
  }
  return PM_OK;
}

