// pm_engine_match.inc — part of pm_engine.cpp (one translation unit; included in place): pair sweep plumbing, claim, the published table (seqlock buffers, pub_patch, publish_begin / _end) (inside namespace pm).
// ------------------------------------------------------------------------------------------------
// pair sweep plumbing

static int32_t ensure_task_planes(pm_engine* e) {
  if (!e->have_tasks) return set_error(PM_ESTATE, "tasks must be uploaded first");
  const uint32_t n_planes = uint32_t(e->cfgs.size());
  const uint32_t stride = e->t_cap / 64u;
  if (e->tplanes_dirty) {  // whole table (upload, capacity change, new configurations); deltas patch the planes
    HIPCHK(e->d_tplanes.ensure(std::max<size_t>(size_t(stride) * (n_planes + 1), 1)));  // + the OR plane
    launch_build_planes(e->d_tmask.p, e->t_cap, e->t_lo, e->t_cap, stride, n_planes, e->d_tplanes.p, e->stream);
    HIPCHK(hipGetLastError());
    e->tplanes_dirty = false;
  }
  if (e->tprefix_dirty) {
    launch_task_prefix(e->d_tlive.p, e->t_lo / 64u, stride, e->d_tprefix.p, e->stream);
    HIPCHK(hipGetLastError());
    e->tprefix_dirty = false;
  }
  return PM_OK;
}

// handle -> position in the caller's current get_all_tasks list (host side; the device does the same in
// claim_publish_kernel)
static uint32_t task_position(pm_engine* e, uint32_t u) {
  if (u == PM_NONE || u < e->t_lo || u >= e->t_cap) return PM_NONE;
  if (!e->h_tprefix_valid) {
    const uint32_t stride = e->t_cap / 64u;
    e->h_tprefix.assign(stride, 0);
    uint32_t acc = 0;
    for (uint32_t j = e->t_lo / 64u; j < stride; ++j) {
      e->h_tprefix[j] = acc;
      acc += uint32_t(__builtin_popcountll(e->h_tlive[j]));
    }
    e->h_tprefix_valid = true;
  }
  const uint64_t w = e->h_tlive[u >> 6];
  if (!((w >> (u & 63u)) & 1ull)) return PM_NONE;
  return e->h_tprefix[u >> 6] + uint32_t(__builtin_popcountll(w & ((1ull << (u & 63u)) - 1ull)));
}

static int32_t ensure_sweep_outputs(pm_engine* e, uint32_t R) {
  HIPCHK(e->d_first.ensure(std::max<uint32_t>(R, 1)));
  HIPCHK(e->d_count.ensure(std::max<uint32_t>(R, 1)));
  HIPCHK(e->d_rank.ensure(std::max<uint32_t>(R, 1)));
  HIPCHK(e->d_chosen.ensure(std::max<uint32_t>(R, 1)));
  return PM_OK;
}

// rank-th applicable task for one configuration bit (merge path: find_best_task_for_group,
// mod.rs:1122-1189).  Returns PM_NONE if no task is applicable.
static int32_t pick_task_for_config(pm_engine* e, uint32_t cfg, uint64_t group_id, uint32_t* task_out) {
  *task_out = PM_NONE;
  if (!e->have_tasks || e->T == 0) return PM_OK;
  // The applicable list depends only on the configuration bit.  Per-configuration counts are kept per version
  // of the task table (one pass), so a merge costs one early-exit scan to the chosen task — not two passes over
  // a million rows.
  if (!e->cfg_app_valid) {
    std::memset(e->cfg_app_count, 0, sizeof(e->cfg_app_count));
    for (uint32_t u = e->t_lo; u < e->t_cap; ++u) {
      uint64_t m = e->h_tmask[u];  // 0 for tombstones
      while (m) {
        e->cfg_app_count[__builtin_ctzll(m)]++;
        m &= m - 1;
      }
    }
    e->cfg_app_valid = true;
  }
  const uint32_t n_app = e->cfg_app_count[cfg];
  if (!n_app) return PM_OK;
  const uint64_t bit = 1ull << cfg;
  uint32_t r = 0;
  if (e->cfg.chooser == PM_CHOOSE_SEEDED) r = uint32_t(splitmix64_mix(e->cfg.chooser_seed ^ group_id) % n_app);
  for (uint32_t u = e->t_lo; u < e->t_cap; ++u)
    if (e->h_tmask[u] & bit) {
      if (r == 0) {
        *task_out = u;  // the handle
        return PM_OK;
      }
      --r;
    }
  return PM_OK;
}

// The pair sweep + chooser + claim for every worker — or, in a multi-GPU tick (`dist`), for the workers this
// rank owns, whose rows go packed into this rank's segment of the exchange buffer (pm_dist_match_begin).
// G_ub: the task words of that many groups are carried over (0 = the device's group count: every caller but the tick that
// queues the match before it knows how many groups the carve in front of it formed)
static int32_t run_match(pm_engine* e, bool want_count, std::vector<uint32_t>* count_out, bool dist = false, size_t G_ub = 0) {
  // (publish_open's hand-over is for THIS call, whatever becomes of it)
  pm_assignment* const claim_h_table = dist ? nullptr : e->claim_h_table;
  uint32_t* const claim_h_gtask = dist ? nullptr : e->claim_h_gtask;
  e->claim_h_table = nullptr;
  e->claim_h_gtask = nullptr;
  if (!e->have_cfgs || !e->have_workers || !e->have_tasks)
    return set_error(PM_ESTATE, "configs, workers and tasks must be uploaded first");
  int32_t rc = push_groups(e);
  if (rc) return rc;
  const int variant = int(e->cfg.sweep_variant);
  host_mark("match: groups pushed");
  rc = ensure_task_planes(e);  // (also the live prefix the published positions come from)
  if (rc) return rc;
  host_mark("match: task planes");
  const uint32_t R = dist ? uint32_t(e->h_own_rows.size()) : e->W;
  const uint32_t* rows = dist ? e->d_own_rows.p : nullptr;
  rc = ensure_sweep_outputs(e, R);
  if (rc) return rc;
  HIPCHK(e->d_sel.ensure(std::max<uint32_t>(e->W, 1)));
  HIPCHK(e->d_table.ensure(std::max<uint32_t>(e->W, 1)));
  HIPCHK(e->d_task_col.ensure(std::max<uint32_t>(e->W, 1)));
  if (e->W == 0) return PM_OK;
  const uint32_t n_planes = uint32_t(e->cfgs.size());

  host_mark("match: selector launch");
  const size_t G = G_ub ? G_ub : e->d_n_groups;  // == groups.size() once the last carve is absorbed
  if (!dist) {  // selector, the sweep's outputs at their neutral values, the ranks inside the groups, the task words: one launch
    MatchPrepArgs m{};
    m.W = e->W;
    m.G = uint32_t(G);
    m.group_of = e->d_group_of.p;
    m.g_cfg = e->d_g_cfg.p;
    m.g_n = e->d_g_n.p;
    m.g_off = e->d_g_off.p;
    m.members = e->d_members.p;
    m.addr_rank = e->d_addr_rank.p;
    m.g_task = e->d_g_task.p;
    m.sel = e->d_sel.p;
    m.first = e->d_first.p;
    m.count = e->d_count.p;
    m.rank_in_group = e->d_rank_in_group.p;
    m.by_rank = e->d_by_rank.p;
    m.g_task_next = e->d_g_task_next.p;
    launch_match_prep(m, e->stream);
  } else {
    launch_worker_selector(e->d_group_of.p, e->d_g_cfg.p, R, rows, e->d_sel.p, e->stream);
  }
  // (the sweep kernel's own bracket only where a bench asks for it — pm_engine_config.time_proposer: two records are two barrier
  // packets, 11 us of an idle GPU in a match of 950; pm_stats.ms_sweep_kernel is 0 otherwise, ms_sweep is the phase as ever)
  const bool time_sweep = e->cfg.time_proposer != 0;
  if (time_sweep) HIPCHK(hipEventRecord(e->kev[4], e->stream));
  const uint32_t t_stride = e->t_cap / 64u;
  launch_pair_sweep(variant, e->d_sel.p, R, e->d_tmask.p, e->d_tplanes.p, e->t_lo, e->t_cap, t_stride, n_planes,
                    e->d_first.p, e->d_count.p, e->stream, /*inited=*/!dist);
  if (time_sweep) HIPCHK(hipEventRecord(e->kev[5], e->stream));
  e->k_sweep_recorded = time_sweep;
  const uint32_t* chosen = e->d_first.p;  // PM_CHOOSE_FIRST: the first applicable task
  if (e->cfg.chooser == PM_CHOOSE_SEEDED) {
    launch_chooser_rank(e->d_group_of.p, e->d_g_id.p, e->d_count.p, R, rows, e->cfg.chooser_seed, e->d_rank.p,
                        e->stream);
    launch_pair_select(variant, e->d_sel.p, R, e->d_tmask.p, e->d_tplanes.p, e->t_lo, e->t_cap, t_stride, n_planes,
                       e->d_rank.p, e->d_chosen.p, e->stream);
    chosen = e->d_chosen.p;
  }
  if (dist) {
    launch_group_rank(e->d_group_of.p, e->d_g_n.p, e->d_g_off.p, e->d_members.p, e->d_addr_rank.p, e->W,
                      e->d_rank_in_group.p, e->d_by_rank.p, e->stream);
    if (G) HIPCHK(hipMemcpyAsync(e->d_g_task_next.p, e->d_g_task.p, G * 4, hipMemcpyDeviceToDevice, e->stream));
  }
  ClaimArgs c{};
  c.R = R;
  c.rows = rows;
  c.group_of = e->d_group_of.p;
  c.g_n = e->d_g_n.p;
  c.g_off = e->d_g_off.p;
  c.g_task = e->d_g_task.p;
  c.g_id = e->d_g_id.p;
  c.g_task_next = e->d_g_task_next.p;
  c.chosen = chosen;
  c.rank_in_group = e->d_rank_in_group.p;
  c.by_rank = e->d_by_rank.p;
  c.t_live = e->d_tlive.p;
  c.t_prefix = e->d_tprefix.p;
  c.table = dist ? e->d_table_x.p + size_t(e->dist_rank) * e->dist_cap_t : e->d_table.p;
  c.task_col = e->d_task_col.p;
  c.h_table = claim_h_table;  // (publish_open: the claim publishes; nullptr: copies behind it)
  c.h_gtask = claim_h_gtask;
  launch_claim_publish(c, e->stream);
  HIPCHK(hipGetLastError());
  if (want_count && count_out) {
    count_out->resize(R);
    HIPCHK(hipMemcpyAsync(count_out->data(), e->d_count.p, size_t(R) * 4, hipMemcpyDeviceToHost, e->stream));
  }
  return PM_OK;
}

// The rows of a snapshot buffer, grown if need be (buffers only grow; a replaced one is retired, not freed: a reader
// may still hold it)
static int32_t pub_buffer(pm_engine* e, PubTable& t, uint32_t rows, uint64_t** out) {
  uint64_t* words = t.words.load(std::memory_order_relaxed);
  if (t.cap_rows < rows || !words) {
    const size_t cap = std::max<size_t>(size_t(rows) + rows / 8 + 64, 64);
    PinBuf<uint64_t> nb;
    if (nb.ensure(cap * 4, cap * 4) != hipSuccess || !nb.p)
      return set_error(PM_ENOMEM, "out of pinned host memory for the published table");
    uint64_t* const nw = nb.p;
    std::memset(nw, 0, cap * 32);
    const uint64_t s0 = t.seq.load(std::memory_order_relaxed);
    t.seq.store(s0 + 1, std::memory_order_relaxed);  // odd while the pointer changes
    std::atomic_thread_fence(std::memory_order_release);
    if (words) e->pub_retired.push_back(std::move(t.own));
    t.own = std::move(nb);
    words = nw;
    t.cap_rows = cap;
    t.words.store(nw, std::memory_order_relaxed);
    t.seq.store(s0 + 2, std::memory_order_release);
  }
  *out = words;
  return PM_OK;
}

// Between two ticks the published table says what the last tick computed, while a task delta changes the POSITION of
// every task behind it in the caller's list and a deleted task or a dead worker takes a group with it
// (mod.rs:1259-1288, status_update_impl.rs:17-29).  The reference binds a group to its task by id
// (get_current_group_task, scheduler_impl.rs:33): a heartbeat between two management-loop runs sees the same task
// under its new position, and nothing for a worker whose group has just been dissolved.  pub_patch applies exactly
// that to the published rows, in place (the sequence counter of the buffer is odd meanwhile: readers retry), from the
// host's group list: a row of a dissolved group becomes the row of a worker in no group, a row of a standing group gets
// the current position of the task the group holds.  `only` = just these workers (a dissolved group's members);
// nullptr = every row (a task delta).  No device work; the device-side task column waits for the next tick.
static void pub_patch(pm_engine* e, const std::vector<uint32_t>* only) {
  const int cur = e->pub_cur.load(std::memory_order_relaxed);
  if (cur < 0) return;  // nothing published
  // the published rows name their group by the slot it had then; if the list has been compacted since, by its id
  const bool by_id = e->pub_groups_epoch != e->groups_epoch;
  // (id -> slot, built once per numbering of the list — a status storm calls this once per worker: slots move only when
  // the epoch does, a group dissolved since is found and seen dead, and the published rows, written before the epoch
  // moved, name no group appended since)
  std::unordered_map<uint64_t, uint32_t>& slot_of_id = e->slot_of_id;
  if (by_id && e->slot_of_id_epoch != e->groups_epoch) {
    slot_of_id.clear();
    slot_of_id.reserve(e->groups.size() * 2);
    for (size_t g = 0; g < e->groups.size(); ++g) slot_of_id.emplace(e->groups[g].id, uint32_t(g));
    e->slot_of_id_epoch = e->groups_epoch;
  }
  PubTable& t = e->pub[cur];
  if (t.cleared.load(std::memory_order_relaxed)) return;  // (pm_reset_groups: no row of this buffer names a group of this list)
  const uint32_t n = t.n.load(std::memory_order_relaxed);
  pm_assignment* rows = reinterpret_cast<pm_assignment*>(t.words.load(std::memory_order_relaxed));
  if (!rows || !n) return;
  // one row as it reads now; keep_shift: what readers of the buffer the row goes to add to a position
  auto patched = [&](pm_assignment a, uint32_t keep_shift) -> pm_assignment {
    if (a.group_slot == PM_NONE) return a;
    uint32_t slot = a.group_slot;
    if (by_id) {
      const auto it = slot_of_id.find(a.group_id);
      slot = it == slot_of_id.end() ? PM_NONE : it->second;
    }
    const bool gone = slot >= e->groups.size() || e->groups[slot].dead;
    if (gone) {
      a.task = PM_NONE;
      a.group_slot = PM_NONE;
      a.group_index = 0;
      a.group_size = 0;
      a.next_worker = PM_NONE;
      a.group_id = 0;
    } else {
      const uint32_t h = e->groups[slot].task;
      a.task = h == PM_NONE ? PM_NONE : task_position(e, h) - keep_shift;  // (readers add the buffer's shift)
    }
    return a;
  };
  auto store_row = [](pm_assignment* dst, const pm_assignment& a) {
    uint64_t v[4];
    std::memcpy(v, &a, sizeof(a));
    uint64_t* d = reinterpret_cast<uint64_t*>(dst);
    for (int k = 0; k < 4; ++k) __atomic_store_n(&d[k], v[k], __ATOMIC_RELAXED);
  };
  if (!only) {
    // Every row: written to the buffer that is NOT current, which then becomes the current one — exactly what a
    // publish does — so a heartbeat thread never waits for a pass over W rows (in place, the buffer's sequence counter
    // would be odd for the whole pass and every look-up would spin on it).
    const int nx = cur ^ 1;
    PubTable& d = e->pub[nx];
    uint64_t* dw = nullptr;
    if (pub_buffer(e, d, n, &dw) == PM_OK && dw) {
      pm_assignment* drows = reinterpret_cast<pm_assignment*>(dw);
      const uint64_t d0 = d.seq.load(std::memory_order_relaxed);
      d.seq.store(d0 + 1, std::memory_order_relaxed);  // odd: being written
      std::atomic_thread_fence(std::memory_order_release);
      for (uint32_t w = 0; w < n; ++w) store_row(&drows[w], patched(rows[w], 0u));
      d.n.store(n, std::memory_order_relaxed);
      d.task_shift.store(0, std::memory_order_relaxed);  // (the rows hold current positions)
      d.cleared.store(0, std::memory_order_relaxed);
      d.seq.store(d0 + 2, std::memory_order_release);  // even: stable
      e->pub_cur.store(nx, std::memory_order_release);
      e->h_table = drows;
      return;
    }
    // (no pinned memory for the other buffer: in place — look-ups retry until the pass is through)
  }
  const uint64_t s0 = t.seq.load(std::memory_order_relaxed);
  t.seq.store(s0 + 1, std::memory_order_relaxed);  // odd: being written
  std::atomic_thread_fence(std::memory_order_release);
  if (only) {  // the members of groups dissolved just now: rows in place
    // A worker is in one group at a time, and `only` holds members of groups that are gone: a row of theirs that names a
    // group at all names one that is gone (the one just dissolved, or an older one the table still carried) — it reads "no
    // group" from now on, whatever it named.  No look at the group list (by slot, or by id through a hash map once the
    // list has been compacted): for the 5,000 workers a status sweep of a thousand deaths frees, those look-ups — two
    // cache misses a row — were 260 of the call's 300 us (PM_HOST_MARKS_STATUS build, tools/churn_probe.py).
    const std::vector<uint32_t>& ws = *only;
    for (size_t i = 0; i < ws.size(); ++i) {
      if (i + 12u < ws.size() && ws[i + 12u] < n) __builtin_prefetch(&rows[ws[i + 12u]], 1);  // (rows anywhere in a 3 MB table)
      const uint32_t w = ws[i];
      if (w >= n) continue;
      uint64_t* d = reinterpret_cast<uint64_t*>(&rows[w]);
      if (uint32_t(__atomic_load_n(&d[0], __ATOMIC_RELAXED) >> 32) == PM_NONE) continue;  // (no group: as it is)
      const uint64_t w2 = __atomic_load_n(&d[2], __ATOMIC_RELAXED);                        // next_worker | padding
      __atomic_store_n(&d[0], (uint64_t(PM_NONE) << 32) | PM_NONE, __ATOMIC_RELAXED);      // task, group_slot
      __atomic_store_n(&d[1], 0ull, __ATOMIC_RELAXED);                                      // group_index, group_size
      __atomic_store_n(&d[2], (w2 & 0xFFFFFFFF00000000ull) | PM_NONE, __ATOMIC_RELAXED);
      __atomic_store_n(&d[3], 0ull, __ATOMIC_RELAXED);                                      // group_id
    }
  } else {
    for (uint32_t w = 0; w < n; ++w) store_row(&rows[w], patched(rows[w], 0u));
    t.task_shift.store(0, std::memory_order_relaxed);  // (the rows hold current positions again)
  }
  t.seq.store(s0 + 2, std::memory_order_release);  // even: stable
}

// n tasks were inserted in front of the list: every published position moves back by n — one word instead of a pass
// over the rows (readers add the buffer's shift to the position they read; the seqlock makes row and shift one unit)
static void pub_shift_tasks(pm_engine* e, uint32_t n_new) {
  const int cur = e->pub_cur.load(std::memory_order_relaxed);
  if (cur < 0) return;
  PubTable& t = e->pub[cur];
  const uint64_t s0 = t.seq.load(std::memory_order_relaxed);
  t.seq.store(s0 + 1, std::memory_order_relaxed);
  std::atomic_thread_fence(std::memory_order_release);
  t.task_shift.store(t.task_shift.load(std::memory_order_relaxed) + n_new, std::memory_order_relaxed);
  t.seq.store(s0 + 2, std::memory_order_release);
}

// D2H of the assignment table + the group task words; the table lands directly in the snapshot buffer that is
// not current (pinned host memory, written by the copy engine between the odd and the even mark of its sequence
// counter — see PubTable), which then becomes the published one.  In two halves, so that a tick can queue the copies
// right behind the claim and build its host copy of the new groups (absorb_groups) while they travel: publish_begin
// marks the buffer and queues the copies, publish_end waits for them, flips the buffers and takes the groups' task
// words in (the host list must be complete by then: it has d_n_groups entries once the last carve is absorbed).
struct PubRun {
  int nx = 0;
  uint64_t s0 = 0;
  uint64_t* words = nullptr;
  size_t G = 0;
};

static void publish_abandon(pm_engine* e, const PubRun& pr) {
  (void)hipStreamSynchronize(e->stream);  // (nothing may still be writing the buffer when it reads as stable again)
  PubTable& t = e->pub[pr.nx];
  t.n.store(0, std::memory_order_relaxed);  // contents undefined: nothing to look up in this buffer
  t.seq.store(pr.s0 + 2, std::memory_order_release);
}

// G: the group count the task words are copied for — groups.size(), or, in front of absorb_groups, the device's count
// (d_n_groups == groups.size() once the last carve is absorbed)
// `direct`: no copies are queued — the run_match that follows writes the buffer and the task words from its claim kernel
// (publish_open: the buffer has to read as "being written" BEFORE that kernel can start)
static int32_t publish_begin(pm_engine* e, PubRun* pr, size_t G, bool direct = false) {
  e->claim_h_table = nullptr;
  e->claim_h_gtask = nullptr;
  HIPCHK(e->h_gtask_pinned.ensure(G, std::max<size_t>(G, std::max<uint32_t>(e->W, 1))));
  const int cur = e->pub_cur.load(std::memory_order_relaxed);
  const int nx = cur < 0 ? 0 : (cur ^ 1);
  PubTable& t = e->pub[nx];
  uint64_t* words = nullptr;
  {
    int32_t rcb = pub_buffer(e, t, e->W, &words);
    if (rcb) return rcb;
  }
  const uint64_t s0 = t.seq.load(std::memory_order_relaxed);
  t.seq.store(s0 + 1, std::memory_order_relaxed);  // odd: being written
  std::atomic_thread_fence(std::memory_order_release);
  pr->nx = nx;
  pr->s0 = s0;
  pr->words = words;
  pr->G = G;
  if (direct) {
    e->claim_h_table = reinterpret_cast<pm_assignment*>(words);
    e->claim_h_gtask = e->h_gtask_pinned.p;
    return PM_OK;
  }
  hipError_t herr = hipSuccess;
  if (e->W) herr = hipMemcpyAsync(words, e->d_table.p, sizeof(pm_assignment) * e->W, hipMemcpyDeviceToHost, e->stream);
  if (herr == hipSuccess && G)
    herr = hipMemcpyAsync(e->h_gtask_pinned.p, e->d_g_task_next.p, G * 4, hipMemcpyDeviceToHost, e->stream);
  if (herr != hipSuccess) {
    publish_abandon(e, *pr);
    HIPCHK(herr);
  }
  return PM_OK;
}

static int32_t publish_end(pm_engine* e, const PubRun& pr) {
  PubTable& t = e->pub[pr.nx];
  const hipError_t herr = hipStreamSynchronize(e->stream);
  if (herr != hipSuccess) {
    publish_abandon(e, pr);
    HIPCHK(herr);
  }
  const size_t G = e->groups.size();
  if (G != pr.G) {  // (the copies were sized by the device's group count in front of absorb_groups: see publish_begin)
    publish_abandon(e, pr);
    return set_error(PM_ESTATE, "publish: the host group list and the device group arrays disagree");
  }
  const uint32_t* g_task = e->h_gtask_pinned.p;
  t.n.store(e->W, std::memory_order_relaxed);
  t.task_shift.store(0, std::memory_order_relaxed);
  t.cleared.store(0, std::memory_order_relaxed);
  t.seq.store(pr.s0 + 2, std::memory_order_release);  // even: stable
  e->pub_cur.store(pr.nx, std::memory_order_release);
  e->h_table = reinterpret_cast<const pm_assignment*>(pr.words);
  e->pub_groups_epoch = e->groups_epoch;
  for (size_t g = 0; g < G; ++g) {
    if (e->groups[g].dead) continue;  // (a tombstone: its device record is stale)
    e->groups[g].task = g_task[g];
    e->groups[g].task_uid = g_task[g] == PM_NONE ? 0 : (e->tasks_have_uid ? e->h_tuid[g_task[g]] : task_position(e, g_task[g]));
  }
  std::swap(e->d_g_task, e->d_g_task_next);
  if (e->chg.on) return changes_publish(e);  // (the change feed: this table against the one before it, queued, not waited for)
  return PM_OK;
}

static int32_t publish_open(pm_engine* e, PubRun* pr, size_t G) { return publish_begin(e, pr, G, /*direct=*/true); }

static int32_t publish(pm_engine* e) {
  PubRun pr;
  int32_t rc = publish_begin(e, &pr, e->groups.size());
  if (rc) return rc;
  return publish_end(e, pr);
}

