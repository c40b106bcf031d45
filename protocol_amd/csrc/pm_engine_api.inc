// pm_engine_api.inc — part of pm_engine.cpp (one translation unit; included in place): C ABI: status changes, the group life-cycle feed, dissolve, get_groups, the single phases (compat / form / merge / match / per-task / newest) (inside extern "C").
int32_t pm_on_worker_status(pm_engine* e, uint32_t worker, uint32_t flags_new, uint32_t dead) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  if (e->dist_phase != 0) return set_error(PM_ESTATE, "a stepwise tick is in progress");
  if (!e->have_workers || worker >= e->W) return set_error(PM_ERANGE, "worker index out of range");
  HIPCHK(hipSetDevice(e->cfg.device));
  ABSORB_PENDING(e);
  e->h_flags[worker] = flags_new;
  if (e->flags_delta_ok) e->delta_flags.push_back(worker);
  e->flags_dirty = true;   // uploaded once before the next kernel that reads the column (sync_flags)
  e->compat_dirty = true;  // HAS_SPECS etc. may have changed with the row
  if (dead && e->h_group_of[worker] >= 0) {  // status_update_impl.rs:17-29
    const uint32_t slot = uint32_t(e->h_group_of[worker]);
    const std::vector<uint32_t> members = e->groups[slot].members;
    dissolve_locked(e, slot);
    pub_patch(e, &members);  // its workers are in no group from now on, also for a look-up before the next tick
  }
  return PM_OK;
}

// pm_on_worker_status_many's body, under the engine mutex, every index below W (also what an applying pm_liveness_sweep runs
// its list through)
static int32_t worker_status_many_locked(pm_engine* e, const uint32_t* workers, const uint32_t* flags_new, const uint32_t* dead,
                                         uint32_t n) {
  if (!n) return PM_OK;
  HIPCHK(hipSetDevice(e->cfg.device));
#ifdef PM_HOST_MARKS_STATUS  // (a measuring build: where a status sweep's time goes)
  host_mark("status: begin");
#endif
  ABSORB_PENDING(e);
#ifdef PM_HOST_MARKS_STATUS
  host_mark("status: pending groups absorbed");
#endif
  std::vector<uint32_t> freed;  // members of the groups this sweep dissolves
  // (the rows of a sweep are anywhere in the table: a worker's group word, then its group's entry, are asked for a few rows
  // ahead of their turn — each was a miss of the host's caches in the middle of the loop)
  for (uint32_t k = 0; k < n && k < 16u; ++k) __builtin_prefetch(&e->h_group_of[workers[k]]);
  for (uint32_t k = 0; k < n; ++k) {
    if (k + 16u < n) __builtin_prefetch(&e->h_group_of[workers[k + 16u]]);
    if (k + 8u < n && dead && dead[k + 8u]) {
      const int32_t g8 = e->h_group_of[workers[k + 8u]];
      if (g8 >= 0) __builtin_prefetch(&e->groups[size_t(g8)]);
    }
    const uint32_t w = workers[k];
    e->h_flags[w] = flags_new[k];
    if (e->flags_delta_ok) e->delta_flags.push_back(w);
    if (dead && dead[k] && e->h_group_of[w] >= 0) {  // status_update_impl.rs:17-29
      const uint32_t slot = uint32_t(e->h_group_of[w]);
      freed.insert(freed.end(), e->groups[slot].members.begin(), e->groups[slot].members.end());
      dissolve_locked(e, slot);
    }
  }
#ifdef PM_HOST_MARKS_STATUS
  host_mark("status: groups dissolved");
#endif
  e->flags_dirty = true;
  e->compat_dirty = true;
  if (!freed.empty()) pub_patch(e, &freed);
#ifdef PM_HOST_MARKS_STATUS
  host_mark("status: published rows patched");
#endif
  return PM_OK;
}

int32_t pm_on_worker_status_many(pm_engine* e, const uint32_t* workers, const uint32_t* flags_new, const uint32_t* dead,
                                 uint32_t n) {
  if (!e || (n && (!workers || !flags_new))) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  if (e->dist_phase != 0) return set_error(PM_ESTATE, "a stepwise tick is in progress");
  if (!e->have_workers) return set_error(PM_ERANGE, "worker index out of range");
  for (uint32_t k = 0; k < n; ++k)
    if (workers[k] >= e->W) return set_error(PM_ERANGE, "worker index out of range");
  return worker_status_many_locked(e, workers, flags_new, dead, n);
}

int32_t pm_enable_group_events(pm_engine* e, uint32_t on) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  ABSORB_PENDING(e);  // creations of a carve that has not been absorbed yet belong to the old setting
  e->events_on = on != 0;
  if (!e->events_on) {
    e->ev_log.clear();
    e->ev_members.clear();
  }
  return PM_OK;
}

int32_t pm_drain_group_events(pm_engine* e, pm_group_event* events, uint32_t cap_events, uint32_t* members,
                              uint32_t cap_members, uint32_t* n_events, uint32_t* n_members) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  ABSORB_PENDING(e);
  const uint32_t ne = uint32_t(e->ev_log.size()), nm = uint32_t(e->ev_members.size());
  if (n_events) *n_events = ne;
  if (n_members) *n_members = nm;
  if ((ne && (!events || cap_events < ne)) || (nm && (!members || cap_members < nm)))
    return set_error(PM_ERANGE, "event buffers too small");
  std::copy(e->ev_log.begin(), e->ev_log.end(), events);
  std::copy(e->ev_members.begin(), e->ev_members.end(), members);
  e->ev_log.clear();
  e->ev_members.clear();
  return PM_OK;
}

int32_t pm_dissolve_group(pm_engine* e, uint32_t slot) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  if (e->dist_phase != 0) return set_error(PM_ESTATE, "a stepwise tick is in progress");
  ABSORB_PENDING(e);
  compact_groups(e);  // `slot` is a number of the compacted list (what pm_get_groups reports)
  if (slot >= e->groups.size()) return set_error(PM_ERANGE, "group slot out of range");
  const std::vector<uint32_t> members = e->groups[slot].members;
  dissolve_locked(e, slot);
  pub_patch(e, &members);
  compact_groups(e);
  return PM_OK;
}

// slot of the group with this id in the compacted list, or PM_NONE.  (A linear pass: the callers are API routes, the
// list holds a few thousand entries of which eight bytes each are read.)
static uint32_t slot_of_group_id(pm_engine* e, uint64_t group_id) {
  for (size_t g = 0; g < e->groups.size(); ++g)
    if (!e->groups[g].dead && e->groups[g].id == group_id) return uint32_t(g);
  return PM_NONE;
}

int32_t pm_dissolve_group_by_id(pm_engine* e, uint64_t group_id, uint32_t* dissolved) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  if (e->dist_phase != 0) return set_error(PM_ESTATE, "a stepwise tick is in progress");
  ABSORB_PENDING(e);
  if (dissolved) *dissolved = 0;
  const uint32_t slot = slot_of_group_id(e, group_id);
  if (slot == PM_NONE) return PM_OK;  // "No group found with ID" (mod.rs:1483-1484): Ok(())
  const std::vector<uint32_t> members = e->groups[slot].members;
  dissolve_locked(e, slot);
  pub_patch(e, &members);
  compact_groups(e);
  if (dissolved) *dissolved = 1;
  return PM_OK;
}

// one entry of the host list as a pm_group + its members in BTreeSet<String> order (address rank)
static int32_t give_group(pm_engine* e, uint32_t slot, pm_group* out, uint32_t* members, uint32_t cap_members) {
  const Group& gr = e->groups[slot];
  out->id = gr.id;
  out->config = gr.cfg;
  out->n_members = uint32_t(gr.members.size());
  out->member_begin = 0;
  out->task = task_position(e, gr.task);
  if (!members) return PM_OK;
  if (cap_members < gr.members.size()) return set_error(PM_ERANGE, "members buffer too small");
  std::copy(gr.members.begin(), gr.members.end(), members);
  std::sort(members, members + gr.members.size(), [&](uint32_t a, uint32_t b) { return e->h_addr_rank[a] < e->h_addr_rank[b]; });
  return PM_OK;
}

// A read between pm_dist_tick_begin and pm_dist_tick_end must not renumber the list: the carve in flight appends its groups
// behind the slots the device holds (absorb_groups, from d_n_groups on, tombstones counted) and the claim's task words are
// indexed by them.  Such a read takes nothing in and compacts nothing: it skips the tombstones, and reports the slot the
// group would have in the compacted list (what pm_get_groups would number it).
static uint32_t compacted_slot(const pm_engine* e, uint32_t g) {
  uint32_t dead = 0;
  for (uint32_t k = 0; k < g; ++k) dead += e->groups[k].dead;
  return g - dead;
}

int32_t pm_get_group_by_id(pm_engine* e, uint64_t group_id, pm_group* out, uint32_t* members, uint32_t cap_members,
                           uint32_t* slot) {
  if (!e || !out || !slot) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  const bool stepwise = e->dist_phase != 0;
  if (!stepwise) {
    ABSORB_PENDING(e);
    compact_groups(e);  // (slots are numbers of the compacted list, as in pm_get_groups)
  }
  std::memset(out, 0, sizeof(*out));
  out->task = PM_NONE;
  const uint32_t g = slot_of_group_id(e, group_id);  // (skips tombstones)
  *slot = g == PM_NONE || !stepwise ? g : compacted_slot(e, g);
  if (g == PM_NONE) return PM_OK;
  return give_group(e, g, out, members, cap_members);
}

int32_t pm_get_group_of_worker(pm_engine* e, uint32_t worker, pm_group* out, uint32_t* members, uint32_t cap_members,
                               uint32_t* slot) {
  if (!e || !out || !slot) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  const bool stepwise = e->dist_phase != 0;
  if (!stepwise) {
    ABSORB_PENDING(e);
    compact_groups(e);
  }
  if (worker >= e->W) return set_error(PM_ERANGE, "worker index out of range");
  std::memset(out, 0, sizeof(*out));
  out->task = PM_NONE;
  const int32_t g = e->h_group_of[worker];  // (a dissolved group's workers read -1: never a tombstone)
  *slot = g < 0 ? PM_NONE : (stepwise ? compacted_slot(e, uint32_t(g)) : uint32_t(g));
  if (g < 0) return PM_OK;
  return give_group(e, uint32_t(g), out, members, cap_members);
}

int32_t pm_reset_groups(pm_engine* e) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  if (e->dist_phase != 0) return set_error(PM_ESTATE, "a stepwise tick is in progress");
  reset_groups_locked(e);
  return PM_OK;
}

int32_t pm_compat_masks(pm_engine* e, uint64_t* mask_out) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(hipSetDevice(e->cfg.device));
  int32_t rc = ensure_compat(e);
  if (rc) return rc;
  if (mask_out && e->W) {
    HIPCHK(hipMemcpyAsync(mask_out, e->d_compat.p, size_t(e->W) * 8, hipMemcpyDeviceToHost, e->stream));
  }
  HIPCHK(hipStreamSynchronize(e->stream));
  return PM_OK;
}

int32_t pm_form_groups(pm_engine* e, uint32_t* n_formed) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  if (e->dist_phase != 0) return set_error(PM_ESTATE, "a stepwise tick is in progress");
  HIPCHK(hipSetDevice(e->cfg.device));
  e->tick_host_resolved = e->tick_carve_launches = e->tick_carve_steps = 0;
  e->tick_fast_steps = 0;
  e->tick_stream_aborts = 0;
  int32_t rc = run_form(e, n_formed);
  e->last_stats.carve_fast_steps = e->tick_fast_steps;
  e->last_stats.host_resolved_steps = e->tick_host_resolved;
  e->last_stats.carve_launches = e->tick_carve_launches;
  e->last_stats.carve_steps = e->tick_carve_steps;
  return rc;
}

int32_t pm_merge_solo_groups(pm_engine* e, uint32_t* n_merged) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  if (e->dist_phase != 0) return set_error(PM_ESTATE, "a stepwise tick is in progress");
  HIPCHK(hipSetDevice(e->cfg.device));
  e->tick_host_resolved = e->tick_carve_launches = e->tick_carve_steps = 0;
  int32_t rc = run_merge(e, n_merged);
  e->last_stats.host_resolved_steps = e->tick_host_resolved;
  e->last_stats.carve_launches = e->tick_carve_launches;
  e->last_stats.carve_steps = e->tick_carve_steps;
  return rc;
}

int32_t pm_get_groups(pm_engine* e, int32_t* group_of_worker, pm_group* groups, uint32_t cap_groups,
                      uint32_t* n_groups, uint32_t* members, uint32_t cap_members, uint32_t* n_members) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  const bool stepwise = e->dist_phase != 0;  // (the list is not compacted under a stepwise tick: tombstones are skipped)
  if (!stepwise) {
    ABSORB_PENDING(e);
    compact_groups(e);
  }
  const uint32_t G = uint32_t(e->groups.size() - (stepwise ? e->n_dead_groups : 0));
  uint32_t M = 0;
  for (const Group& g : e->groups) M += g.dead ? 0u : uint32_t(g.members.size());
  if (n_groups) *n_groups = G;
  if (n_members) *n_members = M;
  if (group_of_worker) {
    std::copy(e->h_group_of.begin(), e->h_group_of.end(), group_of_worker);
    if (stepwise && e->n_dead_groups) {
      std::vector<int32_t> to_slot(e->groups.size());
      for (size_t g = 0, k = 0; g < e->groups.size(); ++g) to_slot[g] = int32_t(k), k += !e->groups[g].dead;
      for (uint32_t w = 0; w < e->W; ++w)
        if (group_of_worker[w] >= 0) group_of_worker[w] = to_slot[size_t(group_of_worker[w])];
    }
  }
  if (groups && cap_groups < G) return set_error(PM_ERANGE, "groups buffer too small");
  if (members && cap_members < M) return set_error(PM_ERANGE, "members buffer too small");
  uint32_t off = 0;
  for (uint32_t g = 0, src = 0; g < G; ++g, ++src) {
    while (e->groups[src].dead) ++src;  // (none outside a stepwise tick: the list was compacted above)
    const Group& gr = e->groups[src];
    if (groups) {
      groups[g].id = gr.id;
      groups[g].config = gr.cfg;
      groups[g].n_members = uint32_t(gr.members.size());
      groups[g].member_begin = off;
      groups[g].task = task_position(e, gr.task);
    }
    if (members) {
      std::vector<uint32_t> m = gr.members;  // BTreeSet<String> order = address rank
      std::sort(m.begin(), m.end(), [&](uint32_t a, uint32_t b) { return e->h_addr_rank[a] < e->h_addr_rank[b]; });
      std::copy(m.begin(), m.end(), members + off);
    }
    off += uint32_t(gr.members.size());
  }
  return PM_OK;
}

int32_t pm_match(pm_engine* e, uint32_t* task_of_worker, uint32_t* applicable_count) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  if (e->dist_phase != 0) return set_error(PM_ESTATE, "a stepwise tick is in progress");
  HIPCHK(hipSetDevice(e->cfg.device));
  if (e->dist_world > 1) return set_error(PM_ESTATE, "multi-GPU engine: use the stepwise tick (pm_dist_tick_begin ...)");
  ABSORB_PENDING(e);
  std::vector<uint32_t> cnt;
  int32_t rc = run_match(e, applicable_count != nullptr, &cnt);
  if (rc) return rc;
  rc = publish(e);
  if (rc) return rc;
  if (task_of_worker)
    for (uint32_t w = 0; w < e->W; ++w) task_of_worker[w] = e->h_table[w].task;
  if (applicable_count) std::copy(cnt.begin(), cnt.end(), applicable_count);
  return PM_OK;
}

// north_star orientation: rows = tasks, swept axis = workers (the ones this rank owns in a multi-GPU set-up);
// leaves first / count per task in d_first / d_count (worker indices are global: every rank holds the whole table)
static int32_t run_match_per_task(pm_engine* e) {
  if (!e->have_tasks) return set_error(PM_ESTATE, "tasks must be uploaded first");
  if (e->dist_world > 1 && e->h_shard.size() != e->W)
    return set_error(PM_ESTATE, "the worker table changed size: call pm_dist_configure again");
  ABSORB_PENDING(e);
  int32_t rc = ensure_compat(e);
  if (rc) return rc;
  rc = push_groups(e);
  if (rc) return rc;
  const int variant = int(e->cfg.sweep_variant);
  const uint32_t n_planes = uint32_t(e->cfgs.size());
  rc = ensure_task_planes(e);  // (the live prefix: results are reported by list position)
  if (rc) return rc;
  const uint32_t R = e->t_cap - e->t_lo;  // rows of the sweep: the used part of the table, tombstones included
  rc = ensure_sweep_outputs(e, R);
  if (rc) return rc;
  HIPCHK(e->d_first_c.ensure(std::max<uint32_t>(e->T, 1)));
  HIPCHK(e->d_count_c.ensure(std::max<uint32_t>(e->T, 1)));
  HIPCHK(e->d_sel.ensure(std::max<uint32_t>(e->W, 1)));
  ensure_price_order(e);
  launch_eligible_selector(e->d_flags.p, e->d_group_of.p, e->d_compat.p, e->enabled, e->W,
                           e->dist_world > 1 ? e->d_shard.p : nullptr, e->dist_rank, e->d_sel.p, e->stream);
  const uint64_t* cols = e->d_sel.p;
  if (e->any_price) {  // order the swept axis by (price, index) so "first hit" is the best bid
    HIPCHK(e->d_perm.ensure(e->W));
    HIPCHK(e->d_sel_perm.ensure(e->W));
    std::vector<uint64_t> sel(e->W), selp(e->W);
    HIPCHK(hipMemcpyAsync(sel.data(), e->d_sel.p, size_t(e->W) * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (uint32_t i = 0; i < e->W; ++i) selp[i] = sel[e->price_perm[i]];
    HIPCHK(hipMemcpyAsync(e->d_sel_perm.p, selp.data(), size_t(e->W) * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    cols = e->d_sel_perm.p;
  }
  if (variant != 1) {
    const size_t n_words = (size_t(e->W) + 63) / 64;
    HIPCHK(e->d_wplanes.ensure(std::max<size_t>(n_words * (n_planes + 1), 1)));  // + the OR plane
    launch_build_planes(cols, e->W, 0, e->W, uint32_t(n_words), n_planes, e->d_wplanes.p, e->stream);
  }
  // Tasks that name the same set of configurations have the same bidders: sweep once per DISTINCT topology mask (a
  // few thousand at a million tasks) and let every task read its mask's result.  Worth it from a few hundred thousand
  // rows on (the table costs three small launches and one counter read: 0.19 against 0.13 ms at 100 k tasks, 1.5
  // against 3.2 ms at a million); a table that fills up (more than 2^16 distinct masks) falls back to one row per task.
  constexpr uint32_t H = 1u << 17, CAP_U = 1u << 16;
  bool per_mask = R >= 200000u && n_planes < 64u && variant != 1;
  uint32_t n_u = 0;
  e->pt_distinct = 0;
  if (per_mask) {
    const uint64_t valid = (1ull << n_planes) - 1ull;
    HIPCHK(e->d_ikeys.ensure(H));
    HIPCHK(e->d_ivals.ensure(H + 2));
    HIPCHK(e->d_umask.ensure(CAP_U));
    uint32_t* counter = e->d_ivals.p + H;  // [0] distinct masks, [1] table overflow
    launch_task_intern(e->d_tmask.p, e->d_tlive.p, e->t_lo, e->t_cap, valid, e->d_ikeys.p, H, e->d_ivals.p, counter,
                       e->d_umask.p, CAP_U, e->stream);
    uint32_t h[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(h, counter, 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    n_u = h[0];
    e->pt_distinct = n_u;
    if (h[1] || n_u > CAP_U) per_mask = false;
    if (per_mask) {
      rc = ensure_sweep_outputs(e, std::max<uint32_t>(n_u, 1));
      if (rc) return rc;
      launch_pair_sweep(variant, e->d_umask.p, n_u, cols, e->d_wplanes.p, 0, e->W, uint32_t((size_t(e->W) + 63) / 64),
                        n_planes, e->d_first.p, e->d_count.p, e->stream);
      launch_task_compact_class(e->d_first.p, e->d_count.p, e->d_tmask.p, valid, e->d_ikeys.p, e->d_ivals.p, H, e->t_lo,
                                e->t_cap, e->d_tlive.p, e->d_tprefix.p, e->d_first_c.p, e->d_count_c.p, e->stream);
    }
  }
  e->pt_interned = per_mask;
  if (!per_mask) {
    launch_pair_sweep(variant, e->d_tmask.p + e->t_lo, R, cols, e->d_wplanes.p, 0, e->W, uint32_t((size_t(e->W) + 63) / 64),
                      n_planes, e->d_first.p, e->d_count.p, e->stream);
    launch_task_compact(e->d_first.p, e->d_count.p, e->t_lo, e->t_cap, e->d_tlive.p, e->d_tprefix.p, e->d_first_c.p,
                        e->d_count_c.p, e->stream);
  }
  HIPCHK(hipGetLastError());
  return PM_OK;
}

int32_t pm_match_per_task(pm_engine* e, uint32_t* best_worker, uint32_t* candidate_count) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  if (e->dist_phase != 0) return set_error(PM_ESTATE, "a stepwise tick is in progress");
  HIPCHK(hipSetDevice(e->cfg.device));
  int32_t rc = run_match_per_task(e);
  if (rc) return rc;
  if (best_worker && e->T)
    HIPCHK(hipMemcpyAsync(best_worker, e->d_first_c.p, size_t(e->T) * 4, hipMemcpyDeviceToHost, e->stream));
  if (candidate_count && e->T)
    HIPCHK(hipMemcpyAsync(candidate_count, e->d_count_c.p, size_t(e->T) * 4, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  if (best_worker && e->any_price)
    for (uint32_t t = 0; t < e->T; ++t)
      if (best_worker[t] != PM_NONE) best_worker[t] = e->price_perm[best_worker[t]];
  return PM_OK;
}

int32_t pm_match_per_task_device(pm_engine* e, uint64_t* best_ptr, uint64_t* count_ptr, uint32_t* n) {
  if (!e || !best_ptr || !count_ptr || !n) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  if (e->dist_phase != 0) return set_error(PM_ESTATE, "a stepwise tick is in progress");
  HIPCHK(hipSetDevice(e->cfg.device));
  ensure_price_order(e);
  if (e->any_price) return set_error(PM_ESTATE, "device-side bids are index-ordered: not available with a price column");
  int32_t rc = run_match_per_task(e);
  if (rc) return rc;
  if (e->own_stream) HIPCHK(hipStreamSynchronize(e->stream));  // a caller-supplied stream orders the consumer itself
  *best_ptr = uint64_t(reinterpret_cast<uintptr_t>(e->d_first_c.p));
  *count_ptr = uint64_t(reinterpret_cast<uintptr_t>(e->d_count_c.p));
  *n = e->T;
  return PM_OK;
}

int32_t pm_newest_task(pm_engine* e, uint32_t* task_idx) {
  if (!e || !task_idx) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(hipSetDevice(e->cfg.device));
  if (!e->have_tasks) return set_error(PM_ESTATE, "tasks must be uploaded first");
  *task_idx = PM_NONE;
  if (e->T == 0) return PM_OK;
  const uint32_t nb = std::min<uint32_t>(1024, (e->t_cap - e->t_lo + 255u) / 256u);
  HIPCHK(e->d_nb_idx.ensure(nb));
  HIPCHK(e->d_nb_val.ensure(nb));
  launch_newest(e->d_created.p, e->d_tlive.p, e->t_lo, e->t_cap, e->d_nb_idx.p, e->d_nb_val.p, nb, e->stream);
  HIPCHK(hipGetLastError());
  std::vector<uint32_t> bi(nb);
  std::vector<long long> bv(nb);
  HIPCHK(hipMemcpyAsync(bi.data(), e->d_nb_idx.p, nb * 4, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(bv.data(), e->d_nb_val.p, nb * 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  uint32_t best = PM_NONE;
  long long bval = 0;
  for (uint32_t k = 0; k < nb; ++k) {
    if (bi[k] == PM_NONE) continue;
    if (best == PM_NONE || bv[k] > bval || (bv[k] == bval && bi[k] > best)) {
      best = bi[k];
      bval = bv[k];
    }
  }
  *task_idx = task_position(e, best);
  return PM_OK;
}

