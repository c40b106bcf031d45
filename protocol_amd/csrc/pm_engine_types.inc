// pm_engine_types.inc — part of pm_engine.cpp (one translation unit; included in place): SiteMap, Group, PubTable (inside namespace pm; DevBuf and the other owning types: pm_owned.h).
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

