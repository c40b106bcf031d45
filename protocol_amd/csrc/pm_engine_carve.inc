// pm_engine_carve.inc — part of pm_engine.cpp (one translation unit; included in place): compat sweep, carve arguments, exact host resolve, absorbing a carve's records, the carve as a run (form_begin .. form_finish) (inside namespace pm).
// end_ev: the event recorded behind the kernel instead of kev[1] (pm_tick hands in its phase event ev[1], which would follow at
// once: one barrier packet less in front of the carve, 5 us of an idle GPU a match)
static int32_t ensure_compat(pm_engine* e, hipEvent_t end_ev = nullptr) {
  if (!e->have_cfgs || !e->have_workers) return set_error(PM_ESTATE, "configs and workers must be uploaded first");
  {
    int32_t rcf = sync_flags(e);
    if (rcf) return rcf;
  }
  if (!e->compat_dirty) return PM_OK;
  for (const pm_gpu_alt_row& a : e->alts)
    if ((a.flags & PM_G_MODEL) && a.model_row >= e->model_rows)
      return set_error(PM_ESTATE, "a GPU alternative names a model row but pm_set_model_table was not called");
  // (once per change of the column or the table, not once per tick: a pass over every row on the host is 100 us at
  // 100,000 workers, a tenth of a churn tick's match)
  if (e->model_rows && e->cls_check_dirty)
    for (uint32_t w = 0; w < e->W; ++w)
      if ((e->h_flags[w] & PM_W_GPU_MODEL) && e->h_gpu_cls[w] >= e->model_classes)
        return set_error(PM_ERANGE, "worker gpu_model_class outside the model table");
  e->cls_check_dirty = false;
  HIPCHK(e->d_compat.ensure(std::max<size_t>(e->W, 1)));
  CompatArgs a{};
  a.W = e->W;
  a.n_cfgs = uint32_t(e->cfgs.size());
  a.model_words = (e->model_classes + 31u) / 32u;
  a.flags = e->d_flags.p;
  a.gpu_count = e->d_gpu_count.p;
  a.gpu_mem = e->d_gpu_mem.p;
  a.gpu_cls = e->d_gpu_cls.p;
  a.cpu_cores = e->d_cpu_cores.p;
  a.ram = e->d_ram.p;
  a.storage = e->d_storage.p;
  a.cfgs = e->d_cfgs.p;
  a.alts = e->d_alts.p;
  a.model_bits = e->d_model_bits.p;
  a.compat = e->d_compat.p;
  HIPCHK(hipEventRecord(e->kev[0], e->stream));
  launch_compat(a, e->stream);
  HIPCHK(hipEventRecord(end_ev ? end_ev : e->kev[1], e->stream));
  HIPCHK(hipGetLastError());
  e->k_compat_recorded = true;
  e->k_compat_end = end_ev ? end_ev : e->kev[1];
  e->compat_dirty = false;
  e->h_compat_valid = false;
  return PM_OK;
}

static int32_t pull_compat(pm_engine* e) {
  if (e->h_compat_valid) return PM_OK;
  e->h_compat.resize(e->W);
  if (e->W) {
    HIPCHK(hipMemcpyAsync(e->h_compat.data(), e->d_compat.p, size_t(e->W) * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  e->h_compat_valid = true;
  return PM_OK;
}

// Haversine exactly as the reference evaluates it (mod.rs:218-231) with the host libm.  Used only by
// the exact-resolve path for steps the GPU certificate could not prove (see carve_kernel).
static double host_distance(double lat1, double lon1, double lat2, double lon2) {
  const double R = 6371.0;
  const double lat1r = lat1 * PM_RAD, lat2r = lat2 * PM_RAD;
  const double dlat = (lat2 - lat1) * PM_RAD, dlon = (lon2 - lon1) * PM_RAD;
  const double s1 = std::sin(dlat / 2.0), s2 = std::sin(dlon / 2.0);
  const double a = s1 * s1 + std::cos(lat1r) * std::cos(lat2r) * (s2 * s2);
  const double c = 2.0 * std::atan2(std::sqrt(a), std::sqrt(1.0 - a));
  return R * c;
}

struct CarvePlan {
  std::vector<uint32_t> avail;  // configuration indices in carve order
};

static size_t carve_lds_bytes(uint32_t /*stride_words*/, bool* in_lds) {
  *in_lds = true;  // the kernel decides per configuration whether its candidate list fits in LDS
  return PM_CARVE_LDS_BYTES;
}

static int32_t fill_carve_args(pm_engine* e, CarveArgs* a, uint32_t mode, uint32_t n_order, bool stream = false) {
  const size_t cap = std::max<size_t>(e->W, 1);
  HIPCHK(e->d_order.ensure(cap));
  HIPCHK(e->d_c_lat.ensure(cap));
  HIPCHK(e->d_c_lon.ensure(cap));
  HIPCHK(e->d_c_cos.ensure(cap));
  HIPCHK(e->d_cc_lat.ensure(cap));
  HIPCHK(e->d_cc_lon.ensure(cap));
  HIPCHK(e->d_cc_cos.ensure(cap));
  for (int k = 0; k < 3; ++k) {
    HIPCHK(e->d_c_u[k].ensure(cap));
    HIPCHK(e->d_cc_u[k].ensure(cap));
  }
  HIPCHK(e->d_c_compat.ensure(cap));
  HIPCHK(e->d_keys.ensure(cap));
  HIPCHK(e->d_slot_pos.ensure(cap));
  HIPCHK(e->d_slot_wid.ensure(cap));
  HIPCHK(e->d_c_site.ensure(cap));
  HIPCHK(e->d_cc_site.ensure(cap));
  {  // proposal rows: at most PM_PROP_MAX_SEEDS + 63 seeds per batch
    HIPCHK(e->d_prop.ensure((size_t(PM_PROP_MAX_SEEDS) + 64) * PM_PROP_ROW));
    HIPCHK(e->d_seed_map.ensure((cap + 63) / 64 + 64));
    HIPCHK(e->d_seed_prefix.ensure((cap + 63) / 64 + 64));
    HIPCHK(e->d_seed_slots.ensure(size_t(PM_PROP_MAX_SEEDS) + 128));
    HIPCHK(e->d_prep_block_counts.ensure(((cap + 255) / 256 + 1) * PM_MAX_CONFIGS));
    HIPCHK(e->d_prep_counts.ensure(PM_MAX_CONFIGS + 8));
  }
  HIPCHK(e->d_status.ensure(1));
  HIPCHK(e->d_carve_args.ensure(1));
  HIPCHK(e->d_desc.ensure(1));
  const uint32_t stride = uint32_t((cap + 63) / 64);
  HIPCHK(e->d_bits.ensure(size_t(stride) * 4));
  HIPCHK(e->d_snap.ensure(stride));
  if (stream) {
    HIPCHK(e->d_c_pack.ensure(cap * 4));
    HIPCHK(e->d_cs_pack.ensure(cap * 4));
    HIPCHK(e->d_cfgbits.ensure(size_t(stride) * PM_MAX_CONFIGS));
    HIPCHK(e->d_stream_ctl.ensure(PM_STREAM_CTL_WORDS));
    if (!e->d_stream_sq.p) {  // (tags never repeat within 127 launches; the rings are cleared when the counter wraps)
      HIPCHK(e->d_stream_sq.ensure(PM_STREAM_SQ));
      HIPCHK(e->d_stream_row_lo.ensure(size_t(PM_STREAM_RQ) * 64));
      HIPCHK(e->d_stream_row_hi.ensure(size_t(PM_STREAM_RQ) * 64));
      e->stream_seq = 0;
    }
  }
  if (mode == CARVE_MODE_FORM && e->prune_mode && e->cfg.proximity_enabled) {
    if (!e->d_cell_cnt.p) {  // (the scan leaves the counts zero behind it: cleared once)
      HIPCHK(e->d_cell_cnt.ensure(PM_CELL_TABLE));
      HIPCHK(hipMemsetAsync(e->d_cell_cnt.p, 0, e->d_cell_cnt.cap * sizeof(uint32_t), e->stream));
    }
    if (!e->d_cell_start.p) {  // + the scan's block sums and its ticket (zero between scans)
      HIPCHK(e->d_cell_start.ensure(PM_CELL_TABLE + 384));
      HIPCHK(hipMemsetAsync(e->d_cell_start.p, 0, e->d_cell_start.cap * sizeof(uint32_t), e->stream));
    }
    HIPCHK(e->d_pos_cell.ensure(cap));
    HIPCHK(e->d_pos_rank.ensure(cap));
    HIPCHK(e->d_cs_of_pos.ensure(cap));
    HIPCHK(e->d_cs_slot.ensure(cap));
    HIPCHK(e->d_cs_site.ensure(cap));
    for (auto& u : e->d_cs_u) HIPCHK(u.ensure(cap));
  }
  std::memset(a, 0, sizeof(*a));
  a->mode = mode;
  a->W = e->W;
  a->proximity = e->cfg.proximity_enabled;
  a->debug_uncertain_every = e->cfg.debug_uncertain_every;
  a->wflags = e->d_flags.p;
  a->lat = e->d_lat.p;
  a->lon = e->d_lon.p;
  a->coslat = e->d_coslat.p;
  a->ux = e->d_ux.p;
  a->uy = e->d_uy.p;
  a->uz = e->d_uz.p;
  a->compat = e->d_compat.p;
  a->group_of = e->d_group_of.p;
  a->order = e->d_order.p;
  a->n_order = n_order;
  a->c_lat = e->d_c_lat.p;
  a->c_lon = e->d_c_lon.p;
  a->c_cos = e->d_c_cos.p;
  a->c_ux = e->d_c_u[0].p;
  a->c_uy = e->d_c_u[1].p;
  a->c_uz = e->d_c_u[2].p;
  a->c_compat = e->d_c_compat.p;
  a->alive_g = e->d_bits.p;
  a->loc_g = e->d_bits.p + stride;
  a->cc_lat = e->d_cc_lat.p;
  a->cc_lon = e->d_cc_lon.p;
  a->cc_cos = e->d_cc_cos.p;
  a->cc_ux = e->d_cc_u[0].p;
  a->cc_uy = e->d_cc_u[1].p;
  a->cc_uz = e->d_cc_u[2].p;
  a->keys = e->d_keys.p;
  a->slot_pos = e->d_slot_pos.p;
  a->slot_wid = e->d_slot_wid.p;
  a->site = e->d_site.p;
  a->c_site = e->d_c_site.p;
  a->cc_site = e->d_cc_site.p;
  a->prop = e->d_prop.p;
  a->seed_map = e->d_seed_map.p;
  a->seed_prefix = e->d_seed_prefix.p;
  a->seed_slots = e->d_seed_slots.p;
  a->count_keys = e->cfg.time_proposer ? 1u : 0u;
  a->prep_block_counts = e->d_prep_block_counts.p;
  a->prep_counts = e->d_prep_counts.p;
  a->bits_scratch = e->d_bits.p + size_t(stride) * 2;
  a->bits_stride = stride;
  a->status = e->d_status.p;
  a->desc = e->d_desc.p;
  a->alive_snap = e->d_snap.p;
  a->debug_mem_above = e->debug_mem_above;
  if (mode == CARVE_MODE_FORM && e->prune_mode && e->cfg.proximity_enabled) {
    a->prune_mode = e->prune_mode;
    a->prune_factor = e->prune_factor;
    a->walk_cap_div = e->walk_cap_div;
    a->cell_cnt = e->d_cell_cnt.p;
    a->cell_start = e->d_cell_start.p;
    a->pos_cell = e->d_pos_cell.p;
    a->pos_rank = e->d_pos_rank.p;
    a->cs_of_pos = e->d_cs_of_pos.p;
    a->cs_slot = e->d_cs_slot.p;
    a->cs_site = e->d_cs_site.p;
    a->cs_ux = e->d_cs_u[0].p;
    a->cs_uy = e->d_cs_u[1].p;
    a->cs_uz = e->d_cs_u[2].p;
  }
  if (stream) {
    // slot == position: the per-slot columns ARE the per-position columns, a slot's worker is the eligible list's
    // entry; d_bits = {published candidate bitmap, loc bitmap, the validator's master bitmap}
    a->stream = 1;
    a->cc_lat = a->c_lat;
    a->cc_lon = a->c_lon;
    a->cc_cos = a->c_cos;
    a->cc_ux = a->c_ux;
    a->cc_uy = a->c_uy;
    a->cc_uz = a->c_uz;
    a->cc_site = a->c_site;
    a->slot_wid = a->order;
    a->bits_scratch = e->d_bits.p;
    a->loc_g = e->d_bits.p + stride;
    a->alive_g = e->d_bits.p + size_t(stride) * 2;
    a->cfgbits = e->d_cfgbits.p;
    a->c_pack = e->d_c_pack.p;
    a->cs_pack = e->d_cs_pack.p;
    a->stream_sq = (unsigned long long*)e->d_stream_sq.p;
    a->stream_row_lo = (unsigned long long*)e->d_stream_row_lo.p;
    a->stream_row_hi = (unsigned long long*)e->d_stream_row_hi.p;
    a->stream_ctl = e->d_stream_ctl.p;
#if defined(PM_CARVE_PROF) || defined(PM_ROW_REC)
    HIPCHK(e->d_stream_trace.ensure(size_t(PM_STREAM_TRACE_CAP) * 2));
    a->stream_trace = (unsigned long long*)e->d_stream_trace.p;
#endif
#ifdef PM_ROW_REC  // (a measuring build: one record of time stamps per ticket, pm_debug_row_records)
    HIPCHK(hipMemsetAsync(e->d_stream_trace.p, 0, size_t(PM_STREAM_TRACE_CAP) * 16, e->stream));
#endif
    a->stream_la = e->stream_la_env;
    a->stream_la_div = e->stream_la_div_env;
    a->stream_row_spins = e->stream_row_spins_env;
    a->debug_abort_after = e->debug_abort_after;
  }
  return PM_OK;
}

// One exact carve step on the host for configuration `cfg` (FORM mode): the same rule as
// mod.rs:511-551 with glibc distances and a stable sort.  Appends the group to the device arrays.
static int32_t host_resolve_form_step(pm_engine* e, uint32_t cfg, CarveStatus* st) {
  int32_t rc = pull_compat(e);
  if (rc) return rc;
  std::vector<int32_t> group_of(e->W);
  if (e->W) {
    HIPCHK(hipMemcpyAsync(group_of.data(), e->d_group_of.p, size_t(e->W) * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  const pm_config_row& c = e->cfgs[cfg];
  std::vector<uint32_t> compat;
  size_t total_available = 0;
  for (uint32_t w = 0; w < e->W; ++w) {
    const uint32_t f = e->h_flags[w];
    if (!((f & PM_W_HEALTHY) && (f & PM_W_HAS_P2P) && group_of[w] < 0)) continue;
    ++total_available;
    if ((e->h_compat[w] >> cfg) & 1ull) compat.push_back(w);
  }
  if (total_available < c.min_group_size || compat.size() < c.min_group_size || compat.empty())
    return set_error(PM_ESTATE, "host resolve: nothing to carve (state mismatch)");
  uint32_t seed = compat[0];
  bool seed_loc = false;
  for (uint32_t w : compat)
    if (e->h_flags[w] & PM_W_HAS_LOC) {
      seed = w;
      seed_loc = true;
      break;
    }
  std::vector<uint32_t> rest;
  for (uint32_t w : compat)
    if (w != seed) rest.push_back(w);
  if (seed_loc && e->cfg.proximity_enabled) {
    std::vector<double> d(e->W, 0.0);
    for (uint32_t w : rest)
      d[w] = (e->h_flags[w] & PM_W_HAS_LOC) ? host_distance(e->h_lat[seed], e->h_lon[seed], e->h_lat[w], e->h_lon[w])
                                            : 1.7976931348623157e308;
    std::stable_sort(rest.begin(), rest.end(), [&](uint32_t a, uint32_t b) { return d[a] < d[b]; });
  }
  std::vector<uint32_t> members{seed};
  for (uint32_t w : rest) {
    if (members.size() >= c.max_group_size) break;
    members.push_back(w);
  }
  if (members.size() < c.min_group_size) return set_error(PM_ESTATE, "host resolve: group below min size");
  const uint32_t g = st->n_groups, off = st->n_members, n = uint32_t(members.size());
  if (g >= e->d_g_cfg.cap || off + n > e->d_members.cap) return set_error(PM_ENOMEM, "group arrays overflow");
  HIPCHK(hipMemcpyAsync(e->d_g_cfg.p + g, &cfg, 4, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(e->d_g_n.p + g, &n, 4, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(e->d_g_off.p + g, &off, 4, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(e->d_members.p + off, members.data(), size_t(n) * 4, hipMemcpyHostToDevice, e->stream));
  for (uint32_t w : members) group_of[w] = int32_t(g);
  HIPCHK(hipMemcpyAsync(e->d_group_of.p, group_of.data(), size_t(e->W) * 4, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  st->n_groups += 1;
  st->n_members += n;
  st->n_solo += n == 1 ? 1u : 0u;
  st->steps_total += 1;
  return PM_OK;
}

// Run the persistent carve kernel until it reports DONE, settling UNCERTAIN steps on the host.
// Append the group records of the last carve to the host list (ids from the generate_group_id stream).
static int32_t absorb_groups(pm_engine* e) {
  if (!e->absorb_pending) return PM_OK;
  HIPCHK(hipEventSynchronize(e->ev_groups));
  const uint32_t g0 = e->ab_g0, ng = e->ab_g1 - e->ab_g0, m0 = e->ab_m0;
  const uint32_t *g_cfg = e->ab_cfg_p, *g_n = e->ab_n_p, *g_off = e->ab_off_p, *members = e->ab_mem_p;
  // (geometric: an exact reserve moves the whole list — 30,000 records — at every tick that appends to a full vector)
  if (e->groups.capacity() < e->groups.size() + ng) e->groups.reserve(std::max(e->groups.size() + ng, e->groups.capacity() * 2));
  for (uint32_t k = 0; k < ng; ++k) {
    Group gr;
    gr.id = splitmix64_next(&e->id_rng);
    gr.cfg = g_cfg[k];
    gr.task = PM_NONE;
    gr.task_uid = 0;
    gr.members.assign(members + (g_off[k] - m0), members + (g_off[k] - m0) + g_n[k]);
    for (uint32_t w : gr.members) e->h_group_of[w] = int32_t(g0 + k);
    log_group_event(e, PM_GROUP_CREATED, gr);  // mod.rs:612-625
    e->groups.push_back(std::move(gr));
  }
  e->absorb_pending = false;
  return PM_OK;
}

// Every entry point that reads the host group list or h_group_of first takes in the records of a carve whose
// absorption was deferred (pm_tick defers it behind the pair sweep; a tick that failed half-way leaves it pending).
#define ABSORB_PENDING(e)                 \
  do {                                    \
    int32_t rc_abs_ = absorb_groups(e);   \
    if (rc_abs_) return rc_abs_;          \
  } while (0)

// PM_TRACE_HOST=1: host-side timestamps (us since the first mark) on stderr, to find where a match waits
static void host_mark(const char* what) {
  static const bool on = [] { const char* v = getenv("PM_TRACE_HOST"); return v && *v == '1'; }();
  if (!on) return;
  static const auto t0 = std::chrono::steady_clock::now();
  const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
  fprintf(stderr, "[pm host] %10.1f us  %s\n", us, what);
}

// One try_form_new_groups run (mod.rs:478-628) as a resumable sequence, so the same code serves the
// single-GPU tick and the stepwise multi-GPU tick, whose ranks each run the whole carve (launches queued blindly,
// status read when they are done).
struct FormRun {
  CarveArgs a;
  CarveStatus st;
  std::vector<uint32_t> avail;
  uint32_t g0 = 0, m0 = 0, start_ci = 0;
  size_t lds = 0;
  bool use_props = false;
  bool nothing = false;  // no configuration / no worker: nothing to carve
  uint32_t n_bound = 0;  // rows outside any group when the carve starts (>= the eligible list): sizes the prep grids
  uint32_t n_elig_hint = 0;  // the eligible ones among them, by the host mirror
  bool stream = false;       // one streaming launch (carve_stream_kernel) instead of the batch pipeline
  uint32_t stream_wgs = 0;   // proposer workgroups of the streaming launch
  bool rearmed = false;      // the carve took more than its first launch sequence (host-resolved step, aborted streaming launch)
  uint32_t stage_cap = 0;    // streaming carve: entries of each staging array carve_finish_kernel fills in pinned host memory
  bool args_pending = false; // `a` is not on the device yet: the first kernel of the launch sequence takes it up as its own argument
};

static int32_t launch_propose_timed(pm_engine* e, const CarveArgs* d_args, uint32_t n_bound, hipStream_t s);

static int32_t form_setup_args(pm_engine* e, FormRun* r);

// fresh: the first launch sequence of a carve — the status block (RUNNING, the group and member counts so far, zero
// otherwise) is initialised by the first kernel of the sequence instead of by a copy in front of it
static int32_t form_queue_init(pm_engine* e, FormRun* r, bool fresh = false) {
  fresh = fresh && r->use_props;  // (the proposal-free carve's one launch reads the status it is handed)
  if (!fresh) HIPCHK(hipMemcpyAsync(e->d_status.p, &r->st, sizeof(r->st), hipMemcpyHostToDevice, e->stream));
  if (r->use_props) {
    if (!r->stream) HIPCHK(hipMemsetAsync(e->d_desc.p, 0, sizeof(BatchDesc), e->stream));  // (the batch pipeline's descriptor)
    // the ordered eligible list, and the spatial index of its positions when there are enough of them to matter
    const uint32_t index_min = !r->a.prune_mode ? 0u : r->a.prune_mode >= 2u ? 1u : PM_CELL_AUTO_N;
    if (r->stream) {
      // every launch tags its tickets and rows from a range of its own (a launch re-armed behind a host-resolved step
      // must not take the rows of the one before it for its own); the rings are cleared when the counter wraps
      if (e->stream_seq == 0 || e->stream_seq >= 127) {
        HIPCHK(hipMemsetAsync(e->d_stream_sq.p, 0, size_t(PM_STREAM_SQ) * 8, e->stream));
        HIPCHK(hipMemsetAsync(e->d_stream_row_lo.p, 0, size_t(PM_STREAM_RQ) * 64 * 8, e->stream));
        HIPCHK(hipMemsetAsync(e->d_stream_row_hi.p, 0, size_t(PM_STREAM_RQ) * 64 * 8, e->stream));
        e->stream_seq = 0;
      }
      e->stream_seq += 1;
      const uint32_t tag0 = e->stream_seq << 25;
      if (r->a.stream_tag0 != tag0) {  // (the first sequence of a carve carries its tag in the argument block it uploads)
        r->a.stream_tag0 = tag0;
        if (!r->args_pending)
          HIPCHK(hipMemcpyAsync(&e->d_carve_args.p->stream_tag0, &r->a.stream_tag0, sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
      }
    }
    e->tick_carve_launches += launch_carve_elig(e->d_carve_args.p, r->args_pending ? &r->a : nullptr, e->W, r->n_bound,
                                                r->n_elig_hint >= index_min ? index_min : 0u, r->start_ci, fresh, r->st.n_groups,
                                                r->st.n_members, e->stream);
    r->args_pending = false;
    host_mark("form: eligible list queued");
    if (r->stream) {  // everything else in one launch (+ the pass that turns positions into worker ids)
      HIPCHK(launch_carve_stream(e->d_carve_args.p, r->start_ci, r->stream_wgs, e->stream));
      e->tick_carve_launches += 2;
      return PM_OK;
    }
    e->tick_carve_launches += launch_carve_prep(e->d_carve_args.p, r->n_bound, e->stream);  // the first candidate list
    HIPCHK(hipGetLastError());
  } else
    HIPCHK(launch_carve(e->d_carve_args.p, CARVE_F_INIT | CARVE_F_RUN | CARVE_F_ALL, r->start_ci, r->lds, e->stream));
  e->tick_carve_launches++;
  return PM_OK;
}

// begin_ev: an event the caller has recorded behind everything in front of the carve (nothing is queued between it and the
// carve's first kernel here): it brackets the carve's kernels instead of a record of its own — a record is a barrier packet
static int32_t form_begin(pm_engine* e, FormRun* r, hipEvent_t begin_ev = nullptr) {
  int32_t rc = absorb_groups(e);  // a match that failed half-way may have left the last carve unabsorbed
  if (rc) return rc;
  rc = ensure_compat(e);
  if (rc) return rc;
  rc = push_groups(e);
  if (rc) return rc;
  available_order(e->cfgs.data(), uint32_t(e->cfgs.size()), e->enabled, &r->avail);
  r->g0 = e->d_n_groups;
  r->m0 = e->d_n_members;
  r->start_ci = 0;
  r->nothing = r->avail.empty() || e->W == 0;
  if (r->nothing) return PM_OK;
  // the eligible list is a subset of the rows no group holds (host mirror, current after absorb_groups): the
  // per-round preparation kernels are sized by that, not by the table (an incremental tick on a standing swarm
  // prepares lists of a few thousand positions out of a hundred thousand rows)
  // ... and how many of those the kernels will find eligible (mod.rs:492-497), as far as the host mirror knows: only
  // used to decide whether the spatial index is worth its four launches (a standing swarm's tick: a few thousand).
  // (Both counts in ONE branch-free pass the compiler vectorises: at 100,000 workers two passes with branches were
  // 150 - 250 us of a churn tick's 1.3 ms.)
  if (e->h_group_of.size() == e->W && e->h_flags.size() == e->W) {
    const int32_t* const gof = e->h_group_of.data();
    const uint32_t* const fl = e->h_flags.data();
    const uint32_t need = PM_W_HEALTHY | PM_W_HAS_P2P;
    uint32_t nb = 0, ne = 0;
    for (uint32_t w = 0; w < e->W; ++w) {
      const uint32_t un = uint32_t(gof[w]) >> 31;  // 1 where no group holds the row
      nb += un;
      ne += un & uint32_t((fl[w] & need) == need);
    }
    r->n_bound = nb;
    r->n_elig_hint = ne;
  } else {
    r->n_bound = uint32_t(std::count_if(e->h_group_of.begin(), e->h_group_of.end(), [](int32_t g) { return g < 0; }));
    r->n_elig_hint = r->n_bound;
  }
  if (e->h_group_of.size() != e->W) r->n_bound = r->n_elig_hint = e->W;
  if (r->n_bound == 0) r->n_bound = 1;
  r->st = CarveStatus{};
  r->st.state = CARVE_STATE_RUNNING;
  r->st.n_groups = r->g0;
  r->st.n_members = r->m0;
  r->use_props = e->cfg.carve_variant != 1 && e->cfg.proximity_enabled;
  // The streaming carve: positions that fit the validator's LDS bitmaps.  Everything else (swarms beyond 262,144
  // unassigned rows) goes through the batch pipeline.
  r->stream = r->use_props && e->cfg.carve_variant == 0 && r->n_bound <= PM_CARVE_BIG_SLOTS &&
              !e->debug_mem_above;  // (the test hook for the all-in-HBM lists is the batch pipeline's)
  host_mark("form: begin (host mirrors counted)");
  rc = form_setup_args(e, r);
  if (rc) return rc;
  host_mark("form: arguments queued");
  if (begin_ev && r->args_pending) {  // (an argument block that went up by a launch of its own stands between the two)
    e->k_carve_begin = begin_ev;
  } else {
    HIPCHK(hipEventRecord(e->kev[2], e->stream));
    e->k_carve_begin = e->kev[2];
  }
  return form_queue_init(e, r, /*fresh=*/true);  // prepares the first candidate list (all of it when there are no proposals)
}

// The argument block(s) of a carve, filled and uploaded (again, when a streaming launch gave up and the batch
// pipeline takes over).
static int32_t form_setup_args(pm_engine* e, FormRun* r) {
  CarveArgs& a = r->a;
  int32_t rc = fill_carve_args(e, &a, CARVE_MODE_FORM, 0, r->stream);
  if (rc) return rc;
  if (r->stream) {
    // proposer workgroups: enough waves to cover a row's latency at the chain's pace, by the size of the list
    uint32_t wgs = e->stream_wgs_env ? e->stream_wgs_env : r->n_elig_hint / 64u + 48u;
    const uint32_t max_wgs = e->n_cus > 8u ? e->n_cus - 4u : 4u;
    r->stream_wgs = std::max(1u, std::min(wgs, max_wgs));
    // the tag of the launch sequence form_queue_init is about to queue (it advances the counter: see there)
    a.stream_tag0 = ((e->stream_seq == 0 || e->stream_seq >= 127) ? 1u : e->stream_seq + 1u) << 25;
    // carve_finish_kernel: group ids, empty task words, and the host's copy of records and status
    a.id_state = e->id_rng;
    a.id_g0 = r->g0;
    a.stage_m0 = r->m0;
    a.g_id_out = (unsigned long long*)e->d_g_id.p;
    a.g_task_out = e->d_g_task.p;
    r->stage_cap = std::max<uint32_t>(r->n_bound, 1u);  // (a group holds at least one of the rows no group holds yet)
    const size_t need = size_t(4) * r->stage_cap;
    if (e->h_gstage.cap < need) HIPCHK(hipStreamSynchronize(e->stream));  // (nothing in flight may still write the old buffer)
    HIPCHK(e->h_gstage.ensure(need, std::max<size_t>(need, size_t(4) * std::max<uint32_t>(e->W, 1))));
    HIPCHK(e->h_status.ensure(1, 1));
    a.stage_cap_g = a.stage_cap_m = r->stage_cap;
    a.stage_cfg = e->h_gstage.p;
    a.stage_n = e->h_gstage.p + r->stage_cap;
    a.stage_off = e->h_gstage.p + size_t(2) * r->stage_cap;
    a.stage_mem = e->h_gstage.p + size_t(3) * r->stage_cap;
    a.h_status = e->h_status.p;
    e->h_status.p->state = 0xFFFFFFFFu;  // (not yet written by this carve)
  }
  a.n_avail = uint32_t(r->avail.size());
  for (size_t i = 0; i < r->avail.size(); ++i) {
    a.avail_cfg[i] = r->avail[i];
    a.min_size[i] = e->cfgs[r->avail[i]].min_group_size;
    a.max_size[i] = e->cfgs[r->avail[i]].max_group_size;
  }
  a.g_cfg = e->d_g_cfg.p;
  a.g_n = e->d_g_n.p;
  a.g_off = e->d_g_off.p;
  a.members = e->d_members.p;
  a.cap_groups = uint32_t(std::min<size_t>(e->d_g_cfg.cap, 0xFFFFFFFFu));
  a.cap_members = uint32_t(std::min<size_t>(e->d_members.cap, 0xFFFFFFFFu));
  bool in_lds;
  r->lds = carve_lds_bytes(a.bits_stride, &in_lds);
  // (a kernel's argument, not a copy: the eligible-list kernel's own where that is the next launch — form_queue_init)
  r->args_pending = r->use_props;
  if (!r->args_pending) HIPCHK(launch_carve_args_put(a, e->d_carve_args.p, e->stream));
  return PM_OK;
}

// the proposer launch, bracketed by its own hipEvents when pm_engine_config.time_proposer asks for the split
static int32_t launch_propose_timed(pm_engine* e, const CarveArgs* d_args, uint32_t n_bound, hipStream_t s) {
  if (!e->cfg.time_proposer) {
    launch_carve_propose(d_args, n_bound, s);
    return PM_OK;
  }
  while (e->prop_ev.size() < e->prop_ev_used + 2) {
    Event x;
    HIPCHK(x.create());
    e->prop_ev.push_back(std::move(x));
  }
  HIPCHK(hipEventRecord(e->prop_ev[e->prop_ev_used], s));
  launch_carve_propose(d_args, n_bound, s);
  HIPCHK(hipEventRecord(e->prop_ev[e->prop_ev_used + 1], s));
  e->prop_ev_used += 2;
  return PM_OK;
}

// (propose, validate) pairs: one per configuration plus one per re-proposal round; launches queued behind a
// finished carve return immediately
static int32_t first_batch_snapshot(pm_engine* e, const FormRun* r);

static int32_t form_queue_pairs(pm_engine* e, FormRun* r, uint32_t count) {
  for (uint32_t k = 0; k < count; ++k) {
    int32_t rc = launch_propose_timed(e, e->d_carve_args.p, r->n_bound, e->stream);
    if (rc) return rc;
    if (e->fb_armed) {  // (pm_debug_first_batch_arm: the first batch as it stands in HBM, before the validator takes it)
      rc = first_batch_snapshot(e, r);
      if (rc) return rc;
    }
    HIPCHK(launch_carve(e->d_carve_args.p, CARVE_F_RUN | CARVE_F_PROPS | CARVE_F_EXTPREP, 0, r->lds, e->stream));
    e->tick_carve_launches += 2u + launch_carve_prep(e->d_carve_args.p, r->n_bound, e->stream);  // the next candidate list
  }
  return PM_OK;
}

// debug (pm_debug_first_batch_arm): behind the first propose launch of a formation on the batch pipeline everything the
// preparation, the index kernels and the proposer wrote is still in HBM — the validation launch is queued behind this.  The
// status and the batch's description come first (they size the rest: the host queues blindly and knows neither list length),
// then every part in stream order, into host memory the engine owns.  Nothing on the device is touched.
static int32_t first_batch_snapshot(pm_engine* e, const FormRun* r) {
  e->fb_armed = false;
  e->fb_taken = false;
  e->fb_part.assign(PM_FB_PARTS, {});
  const CarveArgs& a = r->a;
  CarveStatus st;
  BatchDesc d;
  uint32_t scan_ticket = 0;
  HIPCHK(hipMemcpyAsync(&st, e->d_status.p, sizeof(st), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(&d, e->d_desc.p, sizeof(d), hipMemcpyDeviceToHost, e->stream));
  if (a.cell_start) HIPCHK(hipMemcpyAsync(&scan_ticket, a.cell_start + PM_CELL_TABLE + 320, 4, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  const bool listed = d.planned && d.valid;
  const size_t n = st.n_eligible, nw = (n + 63) / 64;
  const size_t nl = listed ? d.n_list : 0, lw = (nl + 63) / 64, ns = listed ? d.n_seeds : 0;
  const size_t sw = listed && d.prop_k ? (size_t(d.prop_limit) + 63) / 64 : 0;
  const size_t g3 = a.cell_start ? size_t(st.cell_g) * st.cell_g * st.cell_g : 0, ni = g3 ? st.n_indexed : 0;
  if (n > e->d_order.cap || nl > e->d_slot_wid.cap || ns > PM_PROP_MAX_SEEDS + 64u || ni > n || g3 + 1 > PM_CELL_TABLE)
    return set_error(PM_ESTATE, "first batch snapshot: the device's counts exceed the buffers");
  const uint32_t head[PM_FB_HEAD_WORDS] = {d.planned, d.ci0, d.total_available, d.valid, d.none, d.ci, d.n_list, d.prop_k,
                                           d.prop_limit, d.n_seeds, d.cell_g, st.n_eligible, st.cell_g, st.n_indexed,
                                           st.prune_fallbacks, st.pruned_batches, st.n_props, uint32_t(st.prop_keys),
                                           uint32_t(st.prop_keys >> 32), scan_ticket, a.prune_mode, 0, 0, 0};
  e->fb_part[PM_FB_HEAD].assign((const unsigned char*)head, (const unsigned char*)head + sizeof(head));
  auto take = [&](uint32_t part, const void* src, size_t bytes) -> hipError_t {
    e->fb_part[part].resize(bytes);
    return bytes && src ? hipMemcpyAsync(e->fb_part[part].data(), src, bytes, hipMemcpyDeviceToHost, e->stream) : hipSuccess;
  };
  HIPCHK(take(PM_FB_ORDER, a.order, n * 4));
  HIPCHK(take(PM_FB_C_SITE, a.c_site, n * 4));
  HIPCHK(take(PM_FB_C_UX, a.c_ux, n * 8));
  HIPCHK(take(PM_FB_C_UY, a.c_uy, n * 8));
  HIPCHK(take(PM_FB_C_UZ, a.c_uz, n * 8));
  HIPCHK(take(PM_FB_C_LAT, a.c_lat, n * 8));
  HIPCHK(take(PM_FB_C_LON, a.c_lon, n * 8));
  HIPCHK(take(PM_FB_C_COS, a.c_cos, n * 8));
  HIPCHK(take(PM_FB_C_COMPAT, a.c_compat, n * 8));
  HIPCHK(take(PM_FB_LOC_G, a.loc_g, nw * 8));
  HIPCHK(take(PM_FB_ALIVE_SNAP, a.alive_snap, nw * 8));
  HIPCHK(take(PM_FB_SLOT_WID, a.slot_wid, nl * 4));
  HIPCHK(take(PM_FB_SLOT_POS, a.slot_pos, nl * 4));
  HIPCHK(take(PM_FB_CC_SITE, a.cc_site, nl * 4));
  HIPCHK(take(PM_FB_SLOT_ALIVE, a.bits_scratch, lw * 8));
  HIPCHK(take(PM_FB_SLOT_LOC, a.bits_scratch + a.bits_stride, lw * 8));
  HIPCHK(take(PM_FB_SEED_MAP, a.seed_map, sw * 8));
  HIPCHK(take(PM_FB_SEED_PREFIX, a.seed_prefix, sw * 4));
  HIPCHK(take(PM_FB_SEED_SLOTS, a.seed_slots, ns * 4));
  HIPCHK(take(PM_FB_PROP, a.prop, ns * PM_PROP_ROW * 8));
  HIPCHK(take(PM_FB_CELL_START, a.cell_start, g3 ? (g3 + 1) * 4 : 0));
  HIPCHK(take(PM_FB_CELL_CNT, a.cell_cnt, g3 * 4));
  HIPCHK(take(PM_FB_POS_CELL, a.pos_cell, g3 ? n * 4 : 0));
  HIPCHK(take(PM_FB_CS_OF_POS, a.cs_of_pos, g3 ? n * 4 : 0));
  HIPCHK(take(PM_FB_CS_SLOT, a.cs_slot, ni * 4));
  HIPCHK(take(PM_FB_CS_SITE, a.cs_site, ni * 4));
  HIPCHK(take(PM_FB_CS_UX, a.cs_ux, ni * 8));
  HIPCHK(take(PM_FB_CS_UY, a.cs_uy, ni * 8));
  HIPCHK(take(PM_FB_CS_UZ, a.cs_uz, ni * 8));
  HIPCHK(hipStreamSynchronize(e->stream));
  e->fb_taken = true;
  return PM_OK;
}

// Wait for everything queued so far and read the carve's status.  An UNCERTAIN step is settled on the host
// (glibc distances) and the carve re-armed from that configuration; the caller sees RUNNING then.
static int32_t form_poll(pm_engine* e, FormRun* r) {
  for (;;) {
    HIPCHK(hipEventRecord(e->kev[3], e->stream));
    HIPCHK(hipMemcpyAsync(&r->st, e->d_status.p, sizeof(r->st), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    {
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, e->k_carve_begin ? e->k_carve_begin : e->kev[2], e->kev[3]));
      e->k_ms_carve += ms;
      HIPCHK(hipEventRecord(e->kev[2], e->stream));
      e->k_carve_begin = e->kev[2];
      for (size_t k = 0; k + 1 < e->prop_ev_used; k += 2) {
        HIPCHK(hipEventElapsedTime(&ms, e->prop_ev[k], e->prop_ev[k + 1]));
        e->k_ms_propose += ms;
      }
      e->prop_ev_used = 0;
    }
    if (r->st.state == CARVE_STATE_OVERFLOW) return set_error(PM_ENOMEM, "carve: group arrays overflow");
    if (r->st.state == CARVE_STATE_ABORTED) {
      // A bounded wait inside a launch gave up (a GPU shared with other work can keep the proposers of a streaming
      // launch from running beside its validator).  What was committed stands — every commit is exact — and the carve
      // continues from there on the batch pipeline, whose launches depend on nothing running beside them.
      if (!r->stream) return set_error(PM_ENODEV, "carve: a hand-shake inside the validator timed out");
      e->tick_stream_aborts++;
      r->rearmed = true;
      r->stream = false;
      int32_t rca = form_setup_args(e, r);
      if (rca) return rca;
      r->start_ci = r->st.stop_ci;
      r->st.state = CARVE_STATE_RUNNING;
      rca = form_queue_init(e, r);
      if (rca) return rca;
      return PM_OK;  // (RUNNING: the caller queues propose / validate rounds)
    }
    if (r->st.state != CARVE_STATE_UNCERTAIN) return PM_OK;
    int32_t rc = host_resolve_form_step(e, r->avail[r->st.stop_ci], &r->st);
    if (rc) return rc;
    e->tick_host_resolved++;
    r->rearmed = true;
    r->start_ci = r->st.stop_ci;
    r->st.state = CARVE_STATE_RUNNING;
    rc = form_queue_init(e, r);
    if (rc) return rc;
    // read the status again: the INIT launch prepares the next list (and, without proposals, runs on to the end
    // or the next stop)
  }
}

// have_event: ev_groups has been recorded behind the carve already (and waited for)
static int32_t form_finish(pm_engine* e, FormRun* r, uint32_t* n_formed, bool defer_absorb, bool have_event = false) {
  if (n_formed) *n_formed = 0;
  e->fb_armed = false;  // (pm_debug_first_batch_arm is for ONE formation: one that had no propose launch leaves no snapshot and no arm)
  if (r->nothing) return PM_OK;
  const CarveStatus& st = r->st;
  e->tick_fast_steps += st.fast_steps;
  e->tick_carve_steps += st.steps_total;
  e->tick_cand_sum += st.cand_sum;
  e->tick_props += r->stream && !st.n_props ? st.stream_tickets : st.n_props;
  e->tick_prop_keys += st.prop_keys;
  e->tick_stream_timeouts += st.stream_timeouts;
  e->tick_stream_tickets += st.stream_tickets;
  std::memcpy(e->carve_prof, st.prof, sizeof(st.prof));
  for (int k = 0; k < 8; ++k) e->carve_why[k] = st.why[k];
  e->carve_why[8] = st.n_batches;
  e->carve_why[9] = st.n_void;
  e->carve_why[10] = st.pruned_batches;
  e->carve_why[11] = st.prune_fallbacks;
  e->carve_why[12] = st.cell_g;
  e->carve_why[13] = st.n_indexed;
  e->carve_why[14] = r->stream ? 1u : 0u;
  e->carve_why[15] = st.stream_tickets;
  e->carve_why[16] = st.stream_timeouts;
  e->carve_why[17] = st.stream_switches;
  e->carve_why[18] = st.stream_listed;
  e->carve_why[19] = r->stream_wgs;
  e->carve_why[20] = e->tick_stream_aborts;
  e->carve_why[21] = st.slow_steps;
  e->carve_why[22] = st.stream_pre_used;
  e->carve_why[23] = st.stream_pre_lost;
  e->carve_why[24] = st.stream_refreshes;
#ifdef PM_BATCH_LOG
  e->blog.assign(st.blog, st.blog + 3 * std::min<uint32_t>(st.blog_n, 512u));
#endif

  // The new group records stay in HBM for the match; their ids (generate_group_id stream) and empty task
  // words are filled in on the device, and a copy travels to pinned host memory for absorb_groups().
  const uint32_t g0 = r->g0, m0 = r->m0, g1 = st.n_groups, m1 = st.n_members;
  if (g1 > g0) {
    const uint32_t ng = g1 - g0, nm = m1 - m0;
    // One streaming launch sequence did the whole carve: carve_finish_kernel has written the records' host copy, the
    // ids and the empty task words already (the caller waited for the stream since).  Otherwise — a re-armed carve, the
    // batch pipeline — they are copied and filled in here.
    const bool staged = r->stream && !r->rearmed && ng <= r->stage_cap && nm <= r->stage_cap;
    if (staged) {
      e->ab_cfg_p = e->h_gstage.p;
      e->ab_n_p = e->h_gstage.p + r->stage_cap;
      e->ab_off_p = e->h_gstage.p + size_t(2) * r->stage_cap;
      e->ab_mem_p = e->h_gstage.p + size_t(3) * r->stage_cap;
      if (!have_event) HIPCHK(hipEventRecord(e->ev_groups, e->stream));
    } else {
      const size_t need = size_t(3) * ng + nm;
      HIPCHK(e->h_gstage.ensure(need, std::max<size_t>(need, size_t(4) * std::max<uint32_t>(e->W, 1))));
      uint32_t* st_cfg = e->h_gstage.p;
      HIPCHK(hipMemcpyAsync(st_cfg, e->d_g_cfg.p + g0, size_t(ng) * 4, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipMemcpyAsync(st_cfg + ng, e->d_g_n.p + g0, size_t(ng) * 4, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipMemcpyAsync(st_cfg + 2 * size_t(ng), e->d_g_off.p + g0, size_t(ng) * 4, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipMemcpyAsync(st_cfg + 3 * size_t(ng), e->d_members.p + m0, size_t(nm) * 4, hipMemcpyDeviceToHost, e->stream));
      e->ab_cfg_p = st_cfg;
      e->ab_n_p = st_cfg + ng;
      e->ab_off_p = st_cfg + 2 * size_t(ng);
      e->ab_mem_p = st_cfg + 3 * size_t(ng);
      HIPCHK(hipEventRecord(e->ev_groups, e->stream));
      host_mark("form: group copies queued");
      launch_group_ids(e->d_g_id.p + g0, e->d_g_task.p + g0, ng, e->id_rng, e->stream);
      HIPCHK(hipGetLastError());
    }
    e->absorb_pending = true;
    e->ab_g0 = g0;
    e->ab_g1 = g1;
    e->ab_m0 = m0;
    e->ab_m1 = m1;
    e->ab_solo = st.n_solo;
    e->d_n_groups = g1;
    e->d_n_members = m1;
    if (!defer_absorb) {
      int32_t rc = absorb_groups(e);
      if (rc) return rc;
    }
  }
  if (n_formed) *n_formed = g1 - g0;
  return PM_OK;
}

// The part of a single-call carve behind form_begin: wait for what was queued, queue more rounds if the carve needs
// them, take the result in.  (Split from the beginning so that pm_tick_many can start the carves of several engines
// before it waits for the first.)
static int32_t run_form_wait(pm_engine* e, FormRun& r) {
  int32_t rc = PM_OK;
  if (!r.nothing) {
    // (propose, validate, prepare) rounds are queued blindly and the ones behind a finished carve return at once —
    // at ~5 us per empty launch.  The first queue is sized by what the previous carve of this engine needed (a
    // periodic match changes little from tick to tick); one configuration = at least one round otherwise.
    uint32_t batch = e->form_rounds_hint ? e->form_rounds_hint + 1u : r.a.n_avail + 3u;
    for (uint32_t spins = 0;; ++spins) {
      // every poll either ends the carve or follows launches that formed at least one group or moved on to the
      // next configuration: far fewer rounds than this, or the device side is stuck — fail instead of hanging
      if (spins > 4096u + e->W / 8u) return set_error(PM_ENODEV, "carve made no progress");
      if (r.use_props && !r.stream) {
        rc = form_queue_pairs(e, &r, batch);
        if (rc) return rc;
      }
      host_mark("form: carve queued");
      rc = form_poll(e, &r);
      if (rc) return rc;
      host_mark("form: status back");
      if (r.st.state == CARVE_STATE_DONE) break;
      if (r.st.state != CARVE_STATE_RUNNING || !r.use_props) return set_error(PM_ENODEV, "carve kernel did not complete");
      if (r.stream) return set_error(PM_ENODEV, "streaming carve did not complete");  // (it ends DONE, or re-armed above)
      batch = 8u;  // more re-proposal rounds than were queued, or re-armed after a host-resolved step
    }
  }
  if (!r.nothing && r.use_props && !r.stream) e->form_rounds_hint = r.st.n_batches + r.st.n_void;
  return PM_OK;
}
static int32_t run_form_rest(pm_engine* e, FormRun& r, uint32_t* n_formed, bool defer_absorb) {
  int32_t rc = run_form_wait(e, r);
  if (rc) return rc;
  return form_finish(e, &r, n_formed, defer_absorb);
}

static int32_t run_form(pm_engine* e, uint32_t* n_formed, bool defer_absorb = false) {
  FormRun r;
  int32_t rc = form_begin(e, &r);
  if (rc) return rc;
  return run_form_rest(e, r, n_formed, defer_absorb);
}

