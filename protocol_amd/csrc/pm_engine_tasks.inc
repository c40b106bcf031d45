// pm_engine_tasks.inc — part of pm_engine.cpp (one translation unit; included in place): C ABI: the task table and its deltas (upload / insert_front / delete) (inside extern "C").
// A fresh, empty task index space of capacity `cap` (a multiple of 64): host mirror and device columns zeroed.
static int32_t tasks_alloc(pm_engine* e, uint32_t cap) {
  e->h_tmask.assign(cap, 0);
  e->h_created.assign(cap, 0);
  e->h_tlive.assign(cap / 64u, 0);
  if (e->tasks_have_uid) e->h_tuid.assign(cap, 0); else e->h_tuid.clear();
  e->t_cap = cap;
  e->t_lo = cap;
  e->T = e->t_dead = 0;
  e->h_tprefix_valid = false;
  HIPCHK(e->d_tmask.ensure(cap));
  HIPCHK(e->d_created.ensure(cap));
  HIPCHK(e->d_tlive.ensure(cap / 64u));
  HIPCHK(e->d_tprefix.ensure(cap / 64u));
  HIPCHK(hipMemsetAsync(e->d_tmask.p, 0, size_t(cap) * 8, e->stream));
  HIPCHK(hipMemsetAsync(e->d_tlive.p, 0, size_t(cap / 64u) * 8, e->stream));
  e->tplanes_dirty = true;
  e->tprefix_dirty = true;
  return PM_OK;
}

// Host range [u0, u1) of the table -> HBM (masks, created_at, the live words it touches)
static int32_t tasks_push_range(pm_engine* e, uint32_t u0, uint32_t u1) {
  if (u1 <= u0) return PM_OK;
  const uint32_t w0 = u0 / 64u, w1 = (u1 + 63u) / 64u;
  HIPCHK(hipMemcpyAsync(e->d_tmask.p + u0, e->h_tmask.data() + u0, size_t(u1 - u0) * 8, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(e->d_created.p + u0, e->h_created.data() + u0, size_t(u1 - u0) * 8, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(e->d_tlive.p + w0, e->h_tlive.data() + w0, size_t(w1 - w0) * 8, hipMemcpyHostToDevice, e->stream));
  return PM_OK;
}

// Tombstones that may stand inside the swept range [t_lo, t_cap) beyond the live count: a delete that leaves more than
// T + PM_TASK_DEAD_SLACK of them rebuilds the index space before it returns (tasks_rebuild).
static constexpr uint32_t PM_TASK_DEAD_SLACK = 4096;

// A fresh index space of capacity `cap` holding the LIVE rows only, in list order, at its top: the regrowth (the table
// outgrew the room in front of it) and the compaction (too many tombstones in the swept range) both come here.  A
// handle moves by the number of tombstones behind it, so the claims (Group::task) and uid_to_u go through a per-row
// old -> new map.  Positions in the caller's list count live rows only: they do not change, and neither do the published
// rows (pub_patch / pub_shift_tasks hold positions, not handles).
static int32_t tasks_rebuild(pm_engine* e, uint32_t cap) {
  const uint32_t old_cap = e->t_cap, old_lo = e->t_lo, T = e->T;
  const uint32_t new_lo = cap - T;
  std::vector<uint32_t> to_new(old_cap - old_lo, PM_NONE);  // handle - old_lo -> new handle (PM_NONE: a tombstone)
  std::vector<uint64_t> tmask(T), tuid;
  std::vector<int64_t> created(T);
  if (e->tasks_have_uid) tuid.resize(T);
  uint32_t k = 0;
  for (uint32_t u = old_lo; u < old_cap; ++u)
    if ((e->h_tlive[u >> 6] >> (u & 63u)) & 1ull) {
      to_new[u - old_lo] = new_lo + k;
      tmask[k] = e->h_tmask[u];
      created[k] = e->h_created[u];
      if (e->tasks_have_uid) tuid[k] = e->h_tuid[u];
      ++k;
    }
  if (k != T) return set_error(PM_ESTATE, "task table: the live bitmap and the live count disagree");
  int32_t rc = tasks_alloc(e, cap);
  if (rc) return rc;
  std::copy(tmask.begin(), tmask.end(), e->h_tmask.begin() + new_lo);
  std::copy(created.begin(), created.end(), e->h_created.begin() + new_lo);
  if (e->tasks_have_uid) std::copy(tuid.begin(), tuid.end(), e->h_tuid.begin() + new_lo);
  for (uint32_t u = new_lo; u < cap; ++u) e->h_tlive[u >> 6] |= 1ull << (u & 63u);
  e->t_lo = new_lo;
  e->T = T;
  e->t_dead = 0;
  auto remap = [&](uint32_t u) { return u >= old_lo && u < old_cap ? to_new[u - old_lo] : PM_NONE; };
  for (Group& g : e->groups)  // (a standing group's task is live: a deleted task dissolves the groups that held it)
    if (g.task != PM_NONE) g.task = remap(g.task);
  e->groups_dirty = true, e->groups_delta_ok = false;  // the device's claims are handles: the list goes up whole
  e->chg.resync = true;  // (the change feed remembers handles too)
  if (e->uid_map_valid)
    for (auto& kv : e->uid_to_u) kv.second = remap(kv.second);
  rc = tasks_push_range(e, new_lo, cap);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(e->stream));
  return PM_OK;
}

static uint32_t task_capacity_for(uint32_t n) {  // room for about as many insertions as there are tasks
  const uint64_t want = uint64_t(n) * 2 + 65536;
  return uint32_t(std::min<uint64_t>((want + 63) & ~uint64_t(63), 0xFFFFFFC0ull));
}

int32_t pm_upload_tasks(pm_engine* e, const pm_task_soa* t) {
  if (!e || !t) return set_error(PM_EINVAL, "null argument");
  if (t->n && (!t->topo_mask || !t->created_at)) return set_error(PM_EINVAL, "null task column");
  if (t->n > 0x7FFFFFFFu) return set_error(PM_ERANGE, "task table too large");
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(hipSetDevice(e->cfg.device));
  if (e->dist_phase != 0) return set_error(PM_ESTATE, "a stepwise tick is in progress");
  ABSORB_PENDING(e);
  const uint32_t n = t->n;
  const bool had_uid = e->tasks_have_uid;
  e->tasks_have_uid = t->uid != nullptr;
  e->uid_to_u.clear();
  e->uid_map_valid = false;
  e->uid_dup = false;
  e->cfg_app_valid = false;
  int32_t rc;
  if (e->t_cap < n + 64u || uint64_t(e->t_cap) > uint64_t(n) * 8 + (1u << 20) || had_uid != e->tasks_have_uid) {
    rc = tasks_alloc(e, task_capacity_for(n));
    if (rc) return rc;
  }
  // the snapshot replaces the used part: position i of the caller's list -> index lo + i; whatever the old table
  // had in front of the new one is cleared (only the rows that changed hands travel)
  const uint32_t cap = e->t_cap, old_lo = e->t_lo, lo = cap - n, clear_from = std::min(old_lo, lo);
  for (uint32_t u = clear_from; u < lo; ++u) e->h_tmask[u] = 0;
  for (uint32_t w = clear_from / 64u; w < cap / 64u; ++w) e->h_tlive[w] = 0;
  std::memcpy(e->h_tmask.data() + lo, t->topo_mask, size_t(n) * 8);
  std::memcpy(e->h_created.data() + lo, t->created_at, size_t(n) * 8);
  if (t->uid) std::memcpy(e->h_tuid.data() + lo, t->uid, size_t(n) * 8);
  for (uint32_t u = lo; u < cap; ++u) e->h_tlive[u >> 6] |= 1ull << (u & 63u);
  e->t_lo = lo;
  e->T = n;
  e->t_dead = 0;
  e->h_tprefix_valid = false;
  e->chg.resync = true;  // (handles are dealt afresh: the change feed's remembered tasks name nothing)
  rc = tasks_push_range(e, clear_from, cap);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(e->stream));  // pageable sources
  e->tplanes_dirty = true;
  e->tprefix_dirty = true;
  e->have_tasks = true;
  // re-bind claimed tasks by identity; groups whose task vanished are dissolved (on_task_deleted,
  // mod.rs:1259-1288)
  // Only the claimed tasks have to be found again: an open-addressing table of their ids (a few thousand
  // entries, cache-resident), one pass over the new id column.
  size_t n_claim = 0;
  for (const Group& g : e->groups) n_claim += (!g.dead && g.task != PM_NONE);
  if (n_claim) {
    size_t hcap = 64;
    while (hcap < n_claim * 4) hcap <<= 1;
    const uint64_t EMPTY = ~0ull;  // a task id of all ones simply stays unresolved in the table path below
    std::vector<uint64_t> keys(hcap, EMPTY);
    std::vector<uint32_t> vals(hcap, PM_NONE);
    auto slot_of = [&](uint64_t k) {
      size_t h = size_t(splitmix64_mix(k)) & (hcap - 1);
      while (keys[h] != EMPTY && keys[h] != k) h = (h + 1) & (hcap - 1);
      return h;
    };
    if (e->tasks_have_uid) {
      for (const Group& g : e->groups)
        if (!g.dead && g.task != PM_NONE && g.task_uid != EMPTY) keys[slot_of(g.task_uid)] = g.task_uid;
      for (uint32_t i = 0; i < n; ++i) {
        const uint64_t k = t->uid[i];
        size_t h = size_t(splitmix64_mix(k)) & (hcap - 1);
        while (keys[h] != EMPTY && keys[h] != k) h = (h + 1) & (hcap - 1);
        if (keys[h] == k && vals[h] == PM_NONE) vals[h] = i;  // first occurrence, like a map's emplace
      }
    }
    for (size_t g = 0; g < e->groups.size(); ++g) {  // (creation order: dissolutions are logged in it)
      Group& gr = e->groups[g];
      if (gr.dead || gr.task == PM_NONE) continue;
      uint32_t ni = PM_NONE;  // position in the new list
      if (e->tasks_have_uid) {
        if (gr.task_uid != EMPTY) ni = vals[slot_of(gr.task_uid)];
      } else if (gr.task_uid < n) {
        ni = uint32_t(gr.task_uid);  // without ids the identity of a task is its position
      }
      if (ni == PM_NONE) {
        dissolve_locked(e, uint32_t(g));
      } else if (e->t_lo + ni != gr.task) {
        gr.task = e->t_lo + ni;
        e->groups_dirty = true, e->groups_delta_ok = false;
      }
    }
  }
  pub_patch(e, nullptr);  // the published positions follow the new list
  return PM_OK;
}

// on_task_created (node_groups/mod.rs:1224-1243) + TaskStore::add_task (store/domains/task_store.rs:33-55): new
// tasks are the newest, i.e. they sort in FRONT of get_all_tasks (:79, created_at desc).  Only the new rows
// travel; the bit planes are patched in the words they fall into; nothing else moves, so every claimed task
// keeps its handle.
static int32_t tasks_insert_front_locked(pm_engine* e, const pm_task_soa* t);

int32_t pm_tasks_insert_front(pm_engine* e, const pm_task_soa* t) {
  if (!e || !t) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  return tasks_insert_front_locked(e, t);
}

// pm_tasks_insert_front and, with republish != 0, pm_match's pair sweep + claim + publish on the standing groups under
// the same lock: a group that holds no task is offered the new one before the next tick, as the reference would offer
// it at that group's next heartbeat (scheduler_impl.rs:33-74).  No carve.
int32_t pm_tasks_insert_front_ex(pm_engine* e, const pm_task_soa* t, uint32_t republish) {
  if (!e || !t) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  int32_t rc = tasks_insert_front_locked(e, t);
  if (rc || !republish || !t->n) return rc;
  if (e->dist_world > 1) return set_error(PM_ESTATE, "multi-GPU engine: the republish belongs to the stepwise tick");
  if (!e->have_cfgs || !e->have_workers) return PM_OK;  // (nothing to match yet: the next tick publishes)
  ABSORB_PENDING(e);
  rc = run_match(e, false, nullptr);
  if (rc) return rc;
  return publish(e);
}

static int32_t tasks_insert_front_locked(pm_engine* e, const pm_task_soa* t) {
  if (t->n && (!t->topo_mask || !t->created_at)) return set_error(PM_EINVAL, "null task column");
  HIPCHK(hipSetDevice(e->cfg.device));
  if (!e->have_tasks) return set_error(PM_ESTATE, "tasks must be uploaded first (an empty table is fine)");
  if (e->dist_phase != 0) return set_error(PM_ESTATE, "a stepwise tick is in progress");
  if ((t->uid != nullptr) != e->tasks_have_uid && (e->T || e->t_dead))
    return set_error(PM_EINVAL, "the table was uploaded with / without task ids: the new rows must match");
  const uint32_t n = t->n;
  if (!n) return PM_OK;
  for (uint32_t i = 1; i < n; ++i)
    if (t->created_at[i] > t->created_at[i - 1])
      return set_error(PM_EINVAL, "rows must be in get_all_tasks order (created_at descending)");
  for (uint32_t u = e->t_lo; u < e->t_cap; ++u)  // the newest live task of the table
    if ((e->h_tlive[u >> 6] >> (u & 63u)) & 1ull) {
      // an equal timestamp would sort BEHIND the older task (stable sort, task_store.rs:79): not a front insertion
      if (t->created_at[n - 1] <= e->h_created[u])
        return set_error(PM_EINVAL, "not newer than the newest task of the table: use pm_upload_tasks");
      break;
    }
  ABSORB_PENDING(e);
  if (!e->T && !e->t_dead) e->tasks_have_uid = t->uid != nullptr;
  if (e->t_lo < n) {  // out of room in front: a larger index space, everything moves to its top
    if (e->tasks_have_uid && e->h_tuid.size() != e->t_cap) e->h_tuid.assign(e->t_cap, 0);
    int32_t rc = tasks_rebuild(e, task_capacity_for(e->T + n));
    if (rc) return rc;
    e->t_regrowths++;
  }
  // (no compaction here: every upload, delete and rebuild leaves t_dead <= T + PM_TASK_DEAD_SLACK, and an insertion only
  // raises T — pm_tasks_delete is the one place the bound can be crossed)
  if (e->tasks_have_uid && e->h_tuid.size() != e->t_cap) e->h_tuid.assign(e->t_cap, 0);
  const uint32_t lo = e->t_lo - n;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t u = lo + i;
    e->h_tmask[u] = t->topo_mask[i];
    e->h_created[u] = t->created_at[i];
    if (t->uid) e->h_tuid[u] = t->uid[i];
    e->h_tlive[u >> 6] |= 1ull << (u & 63u);
    if (e->cfg_app_valid) {
      uint64_t m = t->topo_mask[i];
      while (m) {
        e->cfg_app_count[__builtin_ctzll(m)]++;
        m &= m - 1;
      }
    }
  }
  if (t->uid && e->uid_map_valid) {
    // an id names the FIRST row in list order that carries it (include/pm_engine.h): the new rows stand in front of every
    // older one, and among themselves the earlier one wins (descending: it is written last)
    const size_t before = e->uid_to_u.size();
    for (uint32_t i = n; i-- > 0;) e->uid_to_u[t->uid[i]] = lo + i;
    if (e->uid_to_u.size() != before + n) e->uid_dup = true;
  }
  {
    int32_t rcp = tasks_push_range(e, lo, e->t_lo);
    if (rcp) return rcp;
  }
  if (!e->tplanes_dirty && e->d_tplanes.p)  // patch the planes: the touched words are rebuilt from the masks
    launch_build_planes(e->d_tmask.p, e->t_cap, lo, e->t_lo, e->t_cap / 64u, uint32_t(e->cfgs.size()), e->d_tplanes.p,
                        e->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(e->stream));  // pageable sources
  e->t_lo = lo;
  e->T += n;
  e->tprefix_dirty = true;
  e->h_tprefix_valid = false;
  pub_shift_tasks(e, n);  // n new tasks in front of the list: every published position moves back by n
  return PM_OK;
}

// the id map (id -> handle of the first live row in list order that carries it), built when first asked for: pm_tasks_delete,
// the rollout ledger's task table
static void ensure_uid_map(pm_engine* e) {
  if (e->uid_map_valid) return;
  e->uid_to_u.clear();
  e->uid_to_u.reserve(size_t(e->T) * 2);
  for (uint32_t u = e->t_cap; u-- > e->t_lo;)  // descending: the first occurrence in list order wins
    if ((e->h_tlive[u >> 6] >> (u & 63u)) & 1ull) e->uid_to_u[e->h_tuid[u]] = u;
  e->uid_map_valid = true;
  e->uid_dup = e->uid_to_u.size() != e->T;
}

// on_task_deleted (node_groups/mod.rs:1245-1325): the tasks leave the table (tombstones: nothing moves) and every
// group that had claimed one of them is dissolved (:1259-1288).  Unknown ids are ignored.
int32_t pm_tasks_delete(pm_engine* e, const uint64_t* uids, uint32_t n, uint32_t* n_deleted) {
  if (!e || (n && !uids)) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(hipSetDevice(e->cfg.device));
  if (n_deleted) *n_deleted = 0;
  if (!e->have_tasks) return set_error(PM_ESTATE, "tasks must be uploaded first");
  if (!e->tasks_have_uid) return set_error(PM_ESTATE, "the task table carries no ids (pm_task_soa.uid)");
  if (e->dist_phase != 0) return set_error(PM_ESTATE, "a stepwise tick is in progress");
  ABSORB_PENDING(e);
  ensure_uid_map(e);
  // what is to go (nothing is changed yet: everything that can fail comes before the first mutation, so that the
  // host mirror and the device table cannot drift apart on an error return)
  std::vector<uint32_t> slots;  // handles of the deleted tasks
  for (uint32_t k = 0; k < n; ++k) {
    auto it = e->uid_to_u.find(uids[k]);
    if (it == e->uid_to_u.end()) continue;
    slots.push_back(it->second);
  }
  if (slots.empty()) return PM_OK;
  std::sort(slots.begin(), slots.end());
  slots.erase(std::unique(slots.begin(), slots.end()), slots.end());  // (an id named twice)
  HIPCHK(e->d_tdel.ensure(slots.size()));
  if (e->tplanes_dirty || !e->d_tplanes.p) {  // no planes yet: only the columns need the update
    int32_t rc = ensure_task_planes(e);
    if (rc) return rc;
  }
  HIPCHK(hipMemcpyAsync(e->d_tdel.p, slots.data(), slots.size() * 4, hipMemcpyHostToDevice, e->stream));
  launch_task_delete(e->d_tdel.p, uint32_t(slots.size()), e->d_tmask.p, e->d_tlive.p, e->d_tplanes.p, e->t_cap / 64u,
                     uint32_t(e->cfgs.size()), e->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(e->stream));
  // ---- the device table is updated: now the host mirror, the groups, the published rows
  for (uint32_t u : slots) {
    e->uid_to_u.erase(e->h_tuid[u]);
    if (e->cfg_app_valid) {
      uint64_t m = e->h_tmask[u];
      while (m) {
        e->cfg_app_count[__builtin_ctzll(m)]--;
        m &= m - 1;
      }
    }
    e->h_tmask[u] = 0;
    e->h_tlive[u >> 6] &= ~(1ull << (u & 63u));
  }
  e->h_tprefix_valid = false;
  for (size_t g = 0; g < e->groups.size(); ++g) {  // (creation order: dissolutions are logged in it)
    const Group& gr = e->groups[g];
    if (!gr.dead && gr.task != PM_NONE && std::binary_search(slots.begin(), slots.end(), gr.task))
      dissolve_locked(e, uint32_t(g));
  }
  if (e->uid_dup) e->uid_map_valid = false;  // (an id some other row carries too names that row now: the map is built anew)
  e->T -= uint32_t(slots.size());
  e->t_dead += uint32_t(slots.size());
  while (e->t_lo < e->t_cap && !((e->h_tlive[e->t_lo >> 6] >> (e->t_lo & 63u)) & 1ull)) {  // dead rows in front
    e->t_lo++;
    e->t_dead--;
  }
  e->tprefix_dirty = true;
  e->h_tprefix_valid = false;
  if (e->t_dead > e->T + PM_TASK_DEAD_SLACK) {  // the swept range is mostly tombstones: the live rows alone, same capacity
    int32_t rc = tasks_rebuild(e, e->t_cap);
    if (rc) return rc;
    e->t_compactions++;
  }
  if (n_deleted) *n_deleted = uint32_t(slots.size());
  pub_patch(e, nullptr);  // a deleted task (and the group that held it) is gone, the tasks behind it move up
  return PM_OK;
}

