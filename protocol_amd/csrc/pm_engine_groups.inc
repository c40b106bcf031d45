// pm_engine_groups.inc — part of pm_engine.cpp (one translation unit; included in place): the host group list and its device mirror: reset / dissolve / compact, push_groups (whole or as a delta), sync_flags (inside namespace pm).
// ------------------------------------------------------------------------------------------------
// small helpers

template <typename T>
static int32_t upload(DevBuf<T>& d, const T* src, size_t n, hipStream_t s) {
  HIPCHK(d.ensure(n ? n : 1));
  if (n) HIPCHK(hipMemcpyAsync(d.p, src, n * sizeof(T), hipMemcpyHostToDevice, s));
  return PM_OK;
}

// every row of the published table reads "no group, no task" until the next publish
static void pub_clear(pm_engine* e) {
  const int cur = e->pub_cur.load(std::memory_order_relaxed);
  if (cur < 0) return;
  PubTable& t = e->pub[cur];
  const uint64_t s0 = t.seq.load(std::memory_order_relaxed);
  t.seq.store(s0 + 1, std::memory_order_relaxed);
  std::atomic_thread_fence(std::memory_order_release);
  t.cleared.store(1u, std::memory_order_relaxed);
  t.seq.store(s0 + 2, std::memory_order_release);
}

static void reset_groups_locked(pm_engine* e) {
  e->groups.clear();
  e->n_dead_groups = 0;
  e->absorb_pending = false;  // records of a carve that was never absorbed belong to the old list
  e->h_group_of.assign(e->W, -1);
  e->id_rng = e->cfg.group_id_seed;
  e->groups_dirty = true, e->groups_delta_ok = false;
  // The published rows name slots and ids of the list that just went (and the id stream restarts: the same ids will
  // name other groups): a heartbeat before the next publish is told "no group", and pub_patch resolves nothing
  // against the new list.
  e->groups_epoch++;
  pub_clear(e);
  e->chg.resync = true;  // (the id stream may repeat: the change feed's remembered ids prove nothing)
}

// dissolve_group (mod.rs:1423-1487).  A status storm dissolves hundreds of groups per tick; removing each from
// the list right away would renumber every later slot (O(groups + workers) per call).  The entry is only
// marked here — the members are free at once — and compact_groups() removes all marked entries in one pass,
// in list order, before anything looks at slot numbers again.
// one entry of the group life-cycle feed; members in BTreeSet<String> order (address rank), like pm_get_groups
static void log_group_event(pm_engine* e, uint32_t kind, const Group& gr) {
  if (!e->events_on) return;
  pm_group_event ev{};
  ev.group_id = gr.id;
  ev.kind = kind;
  ev.config = gr.cfg;
  ev.member_begin = uint32_t(e->ev_members.size());
  ev.n_members = uint32_t(gr.members.size());
  e->ev_members.insert(e->ev_members.end(), gr.members.begin(), gr.members.end());
  std::sort(e->ev_members.end() - ptrdiff_t(gr.members.size()), e->ev_members.end(),
            [&](uint32_t a, uint32_t b) { return e->h_addr_rank[a] < e->h_addr_rank[b]; });
  e->ev_log.push_back(ev);
}

static void dissolve_locked(pm_engine* e, uint32_t slot) {
  if (slot >= e->groups.size() || e->groups[slot].dead) return;
  log_group_event(e, PM_GROUP_DESTROYED, e->groups[slot]);  // mod.rs:1469-1481
  for (uint32_t w : e->groups[slot].members) e->h_group_of[w] = -1;
  if (e->groups_delta_ok) e->delta_free.insert(e->delta_free.end(), e->groups[slot].members.begin(), e->groups[slot].members.end());
  e->groups[slot].dead = true;
  e->n_dead_groups++;
  e->groups_dirty = true;  // (a delta while groups_delta_ok: see push_groups)
}

static void compact_groups(pm_engine* e) {
  if (!e->n_dead_groups) return;
  e->groups.erase(std::remove_if(e->groups.begin(), e->groups.end(), [](const Group& g) { return g.dead; }),
                  e->groups.end());
  e->groups_epoch++;  // (published group slots no longer index this list)
  std::fill(e->h_group_of.begin(), e->h_group_of.end(), -1);
  for (size_t g = 0; g < e->groups.size(); ++g)
    for (uint32_t w : e->groups[g].members) e->h_group_of[w] = int32_t(g);
  e->n_dead_groups = 0;
  e->groups_dirty = true, e->groups_delta_ok = false;
}

// Mirror the host group list into HBM (packed member pool, slot = index).
// n u32 words of pinned staging + device scratch for a delta (the stream has drained since the last use: a delta goes
// up once per tick, in front of it)
static int32_t delta_stage(pm_engine* e, int which, size_t n) {
  HIPCHK(hipStreamSynchronize(e->stream));  // (nothing in flight may still read the staging: an idle stream answers at once)
  HIPCHK(e->h_delta_pin[which].ensure(n, n + n / 2 + 4096));
  HIPCHK(e->d_delta[which].ensure(n));
  return PM_OK;
}

static int32_t push_groups(pm_engine* e) {
  if (!e->groups_dirty) return PM_OK;
  // ---- the churn path: only dissolutions and new rows since the device last held the list.  The dissolved groups stay
  // where they are, in both lists, as tombstones (no worker names them any more; a slot number — what group_of and the
  // published rows hold — keeps its meaning); their workers and the new rows read "no group" on the device after one
  // scatter and one fill.  Compaction waits until a good part of the list is dead or the arrays run short of room for
  // what the next carve may append.
  const size_t room_g = std::min(e->d_g_cfg.cap, std::min(e->d_g_task.cap, std::min(e->d_g_task_next.cap, e->d_g_id.cap)));
  const size_t room_m = std::min(e->d_members.cap, std::min(e->d_by_rank.cap, e->d_rank_in_group.cap));
  if (e->groups_delta_ok && e->n_dead_groups * 4 <= e->groups.size() + 256 && size_t(e->d_n_groups) + e->W <= room_g &&
      size_t(e->d_n_members) + e->W <= room_m && e->d_n_groups == e->groups.size()) {
    HIPCHK(e->d_group_of.grow_keep(std::max<size_t>(e->W, 1), e->delta_tail_from == PM_NONE ? e->W : e->delta_tail_from, e->stream));
    if (e->delta_tail_from != PM_NONE && e->delta_tail_from < e->W)
      HIPCHK(hipMemsetAsync(e->d_group_of.p + e->delta_tail_from, 0xFF, size_t(e->W - e->delta_tail_from) * 4, e->stream));
    if (!e->delta_free.empty()) {
      const size_t n = e->delta_free.size();
      int32_t rc = delta_stage(e, 0, n);
      if (rc) return rc;
      std::memcpy(e->h_delta_pin[0].p, e->delta_free.data(), n * 4);
      HIPCHK(hipMemcpyAsync(e->d_delta[0].p, e->h_delta_pin[0].p, n * 4, hipMemcpyHostToDevice, e->stream));
      launch_scatter_const(reinterpret_cast<uint32_t*>(e->d_group_of.p), e->d_delta[0].p, uint32_t(n), 0xFFFFFFFFu, e->stream);
      HIPCHK(hipGetLastError());
    }
    e->delta_free.clear();
    e->delta_tail_from = PM_NONE;
    e->groups_dirty = false;
    e->delta_pushes++;
    return PM_OK;
  }
  compact_groups(e);
  if (!e->groups_dirty) return PM_OK;
  const size_t G = e->groups.size();
  std::vector<uint32_t> g_cfg(G), g_n(G), g_off(G), g_task(G), members;
  std::vector<uint64_t> g_id(G);
  members.reserve(e->W);
  for (size_t g = 0; g < G; ++g) {
    const Group& gr = e->groups[g];
    g_cfg[g] = gr.cfg;
    g_n[g] = uint32_t(gr.members.size());
    g_off[g] = uint32_t(members.size());
    g_task[g] = gr.task;
    g_id[g] = gr.id;
    members.insert(members.end(), gr.members.begin(), gr.members.end());
  }
  // (twice the table: room for a carve's appends on top of a list that carries tombstones — see the delta path above)
  const size_t capG = std::max<size_t>(size_t(2) * e->W, 1), capM = std::max<size_t>(size_t(2) * e->W, 1);
  HIPCHK(e->d_g_cfg.ensure(capG));
  HIPCHK(e->d_g_n.ensure(capG));
  HIPCHK(e->d_g_off.ensure(capG));
  HIPCHK(e->d_g_task.ensure(capG));
  HIPCHK(e->d_g_task_next.ensure(capG));
  HIPCHK(e->d_g_id.ensure(capG));
  HIPCHK(e->d_members.ensure(capM));
  HIPCHK(e->d_by_rank.ensure(capM));
  HIPCHK(e->d_rank_in_group.ensure(capM));
  HIPCHK(e->d_group_of.ensure(capM));
  if (G) {
    HIPCHK(hipMemcpyAsync(e->d_g_cfg.p, g_cfg.data(), G * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->d_g_n.p, g_n.data(), G * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->d_g_off.p, g_off.data(), G * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->d_g_task.p, g_task.data(), G * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->d_g_id.p, g_id.data(), G * 8, hipMemcpyHostToDevice, e->stream));
  }
  if (!members.empty())
    HIPCHK(hipMemcpyAsync(e->d_members.p, members.data(), members.size() * 4, hipMemcpyHostToDevice, e->stream));
  if (e->W) {
    if (G == 0)  // no group holds a worker (a cold match behind pm_reset_groups): every row is -1, nothing is staged
      HIPCHK(hipMemsetAsync(e->d_group_of.p, 0xFF, size_t(e->W) * 4, e->stream));
    else
      HIPCHK(hipMemcpyAsync(e->d_group_of.p, e->h_group_of.data(), size_t(e->W) * 4, hipMemcpyHostToDevice, e->stream));
  }
  if (G) HIPCHK(hipStreamSynchronize(e->stream));  // the staging vectors die here
  e->d_n_groups = uint32_t(G);
  e->d_n_members = uint32_t(members.size());
  e->groups_dirty = false;
  e->groups_delta_ok = true;  // the device holds the list: dissolutions and new rows from here on are deltas
  e->delta_free.clear();
  e->delta_tail_from = PM_NONE;
  return PM_OK;
}

// status changes only touch the host copy of the flags column; the column goes up once before its next use
static int32_t sync_flags(pm_engine* e) {
  if (!e->flags_dirty || !e->have_workers) return PM_OK;
  if (e->flags_delta_ok && e->delta_flags.size() * 8 <= size_t(e->W)) {  // a few rows: {index, value} pairs and one scatter
    const size_t n = e->delta_flags.size();
    if (n) {
      int32_t rc = delta_stage(e, 1, 2 * n);
      if (rc) return rc;
      for (size_t k = 0; k < n; ++k) {
        e->h_delta_pin[1].p[2 * k] = e->delta_flags[k];
        e->h_delta_pin[1].p[2 * k + 1] = e->h_flags[e->delta_flags[k]];
      }
      HIPCHK(hipMemcpyAsync(e->d_delta[1].p, e->h_delta_pin[1].p, n * 8, hipMemcpyHostToDevice, e->stream));
      launch_scatter_pairs(e->d_flags.p, e->d_delta[1].p, uint32_t(n), e->stream);
      HIPCHK(hipGetLastError());
    }
  } else {
    HIPCHK(hipMemcpyAsync(e->d_flags.p, e->h_flags.data(), size_t(e->W) * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));  // pageable source
  }
  e->delta_flags.clear();
  e->flags_delta_ok = true;
  e->flags_dirty = false;
  return PM_OK;
}

