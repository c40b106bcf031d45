// pm_engine_report.inc — part of pm_engine.cpp (one translation unit; included in place): C ABI: the diagnostics reports
// (pm_explain_workers, pm_config_report, pm_task_report; kernels in pm_report.inc) (inside extern "C").
//
// A report answers from the state every earlier call left — the host's flags column (status changes that have not gone up
// yet included), the host's group list (dissolutions not yet pushed included) — and leaves that state as it found it: the
// pending deltas stay pending (groups_delta_ok, flags_delta_ok, delta_free, delta_flags), nothing is compacted, no cache
// flag of the tick (compat_dirty, tprefix_dirty, cls_check_dirty) is cleared, and what it needs beyond the engine's columns
// goes to scratch buffers of its own (d_rep_*).  The compat masks are not read: they may be stale.

// the checks every report makes, the model rule's bounds as ensure_compat checks them (its flag is left alone)
static int32_t report_begin(pm_engine* e, bool need_tasks) {
  if (e->dist_phase != 0) return set_error(PM_ESTATE, "a stepwise tick is in progress");
  if (!e->have_cfgs || !e->have_workers) return set_error(PM_ESTATE, "configs and workers must be uploaded first");
  if (need_tasks && !e->have_tasks) return set_error(PM_ESTATE, "tasks must be uploaded first");
  HIPCHK(hipSetDevice(e->cfg.device));
  ABSORB_PENDING(e);
  for (const pm_gpu_alt_row& a : e->alts)
    if ((a.flags & PM_G_MODEL) && a.model_row >= e->model_rows)
      return set_error(PM_ESTATE, "a GPU alternative names a model row but pm_set_model_table was not called");
  if (e->model_rows && e->cls_check_dirty)
    for (uint32_t w = 0; w < e->W; ++w)
      if ((e->h_flags[w] & PM_W_GPU_MODEL) && e->h_gpu_cls[w] >= e->model_classes)
        return set_error(PM_ERANGE, "worker gpu_model_class outside the model table");
  return PM_OK;
}

// the worker columns and configuration tables; flags = the current host column (uploaded to scratch while changes wait)
static int32_t report_compat_args(pm_engine* e, CompatArgs* a) {
  *a = CompatArgs{};
  a->W = e->W;
  a->n_cfgs = uint32_t(e->cfgs.size());
  a->model_words = (e->model_classes + 31u) / 32u;
  a->flags = e->d_flags.p;
  if (e->flags_dirty && e->W) {
    int32_t rc = upload(e->d_rep_flags, e->h_flags.data(), e->W, e->stream);
    if (rc) return rc;
    a->flags = e->d_rep_flags.p;
  }
  a->gpu_count = e->d_gpu_count.p;
  a->gpu_mem = e->d_gpu_mem.p;
  a->gpu_cls = e->d_gpu_cls.p;
  a->cpu_cores = e->d_cpu_cores.p;
  a->ram = e->d_ram.p;
  a->storage = e->d_storage.p;
  a->cfgs = e->d_cfgs.p;
  a->alts = e->d_alts.p;
  a->model_bits = e->d_model_bits.p;
  return PM_OK;
}

// The group list the kernels count.  While the device mirror holds the host list slot for slot (nothing changed since the
// last push, or only what a delta push would carry: dissolutions, new rows) it is read in place and a bitmap of the live
// slots marks the tombstones; otherwise (a list compacted, adopted or re-pointed at other task handles since) the live
// groups' (configuration, size, task handle) go up to scratch.
static int32_t report_groups(pm_engine* e, ReportArgs* a) {
  const size_t G = e->groups.size();
  const bool mirror = (!e->groups_dirty || e->groups_delta_ok) && e->d_n_groups == G && e->d_g_cfg.p && e->d_g_n.p &&
                      e->d_g_task.p;
  if (mirror) {
    a->g_cfg = e->d_g_cfg.p, a->g_n = e->d_g_n.p, a->g_task = e->d_g_task.p, a->G = uint32_t(G);
    a->live_bits = nullptr;
    if (e->n_dead_groups && G) {
      std::vector<uint32_t> live((G + 31) / 32, 0u);
      for (size_t g = 0; g < G; ++g)
        if (!e->groups[g].dead) live[g >> 5] |= 1u << (g & 31);
      int32_t rc = upload(e->d_rep_live, live.data(), live.size(), e->stream);
      if (rc) return rc;
      HIPCHK(hipStreamSynchronize(e->stream));  // (pageable source)
      a->live_bits = e->d_rep_live.p;
    }
    return PM_OK;
  }
  const size_t L = G - e->n_dead_groups;
  std::vector<uint32_t> rec(3 * std::max<size_t>(L, 1));
  size_t k = 0;
  for (const Group& gr : e->groups) {
    if (gr.dead) continue;
    rec[k] = gr.cfg, rec[L + k] = uint32_t(gr.members.size()), rec[2 * L + k] = gr.task;
    ++k;
  }
  int32_t rc = upload(e->d_rep_g, rec.data(), rec.size(), e->stream);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(e->stream));  // (pageable source)
  a->g_cfg = e->d_rep_g.p, a->g_n = e->d_rep_g.p + L, a->g_task = e->d_rep_g.p + 2 * L, a->G = uint32_t(L);
  a->live_bits = nullptr;
  return PM_OK;
}

// the task index space; the per-word live prefix is the engine's when it is current, else built into scratch
static int32_t report_tasks(pm_engine* e, ReportArgs* a) {
  if (!e->have_tasks || e->t_cap <= e->t_lo) return PM_OK;
  a->tmask = e->d_tmask.p, a->tlive = e->d_tlive.p, a->t_lo = e->t_lo, a->t_cap = e->t_cap;
  a->tprefix = e->d_tprefix.p;
  if (e->tprefix_dirty) {
    HIPCHK(e->d_rep_tprefix.ensure(std::max<uint32_t>(e->t_cap / 64u, 1)));
    launch_task_prefix(e->d_tlive.p, e->t_lo / 64u, e->t_cap / 64u, e->d_rep_tprefix.p, e->stream);
    HIPCHK(hipGetLastError());
    a->tprefix = e->d_rep_tprefix.p;
  }
  return PM_OK;
}

static uint32_t worker_state(const pm_engine* e, uint32_t w) {
  if (e->h_group_of[w] >= 0) return PM_WS_IN_GROUP;
  const uint32_t f = e->h_flags[w];
  if (!(f & PM_W_HEALTHY)) return PM_WS_UNHEALTHY;
  if (!(f & PM_W_HAS_P2P)) return PM_WS_NO_P2P;
  return PM_WS_IDLE;
}

int32_t pm_explain_workers(pm_engine* e, const uint32_t* workers, uint32_t n, uint8_t* why, uint32_t* state) {
  if (!e || (n && !workers)) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  int32_t rc = report_begin(e, false);
  if (rc) return rc;
  for (uint32_t i = 0; i < n; ++i)
    if (workers[i] >= e->W) return set_error(PM_ERANGE, "worker index out of range");
  const uint32_t C = uint32_t(e->cfgs.size());
  if (n && C && why) {
    CompatArgs a{};
    if ((rc = report_compat_args(e, &a))) return rc;
    const uint32_t stride = (C + 3u) / 4u;  // dwords a row
    if ((rc = upload(e->d_rep_rows, workers, n, e->stream))) return rc;
    HIPCHK(e->d_rep_why.ensure(size_t(n) * stride));
    launch_explain(a, e->d_rep_rows.p, n, stride, e->d_rep_why.p, e->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy2DAsync(why, C, e->d_rep_why.p, size_t(stride) * 4u, C, n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  if (state)
    for (uint32_t i = 0; i < n; ++i) state[i] = worker_state(e, workers[i]);
  return PM_OK;
}

int32_t pm_config_report(pm_engine* e, pm_config_report_row* out, uint32_t cap, uint32_t* n_cfgs) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  int32_t rc = report_begin(e, false);
  if (rc) return rc;
  const uint32_t C = uint32_t(e->cfgs.size());
  if (n_cfgs) *n_cfgs = C;
  if (cap < C || (C && !out)) return set_error(PM_ERANGE, "report buffer too small");
  if (!C) return PM_OK;
  ReportArgs a{};
  if ((rc = report_compat_args(e, &a.c))) return rc;
  a.group_of = e->d_group_of.p;
  if (e->groups_dirty && e->W) {  // (dissolutions and new rows the device has not seen yet)
    if ((rc = upload(e->d_rep_gof, e->h_group_of.data(), e->W, e->stream))) return rc;
    a.group_of = e->d_rep_gof.p;
  }
  if ((rc = report_groups(e, &a))) return rc;
  if ((rc = report_tasks(e, &a))) return rc;
  HIPCHK(e->d_rep_cnt.ensure(size_t(C) * REP_STRIDE));
  HIPCHK(hipMemsetAsync(e->d_rep_cnt.p, 0, size_t(C) * REP_STRIDE * 4u, e->stream));
  a.out = e->d_rep_cnt.p;
  launch_config_report(a, 4u * e->n_cus, e->stream);
  HIPCHK(hipGetLastError());
  std::vector<uint32_t> cnt(size_t(C) * REP_STRIDE);
  HIPCHK(hipMemcpyAsync(cnt.data(), e->d_rep_cnt.p, cnt.size() * 4u, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  for (uint32_t c = 0; c < C; ++c) {
    const uint32_t* k = &cnt[size_t(c) * REP_STRIDE];
    pm_config_report_row& r = out[c];
    r.enabled = uint32_t((e->enabled >> c) & 1ull);
    r.eligible_meets = k[REP_WHY + PM_WHY_OK];
    r.idle_meets = k[REP_IDLE];
    for (uint32_t j = 0; j < PM_WHY_N; ++j) r.why[j] = k[REP_WHY + j];
    r.groups = k[REP_GROUPS];
    r.members = k[REP_MEMBERS];
    r.groups_without_task = k[REP_NO_TASK];
    r.tasks_allowing = k[REP_TASKS];
  }
  return PM_OK;
}

int32_t pm_task_report(pm_engine* e, uint32_t* groups_running, uint32_t* workers_running, uint32_t* groups_allowed) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  int32_t rc = report_begin(e, true);
  if (rc) return rc;
  const uint32_t T = e->T, C = uint32_t(e->cfgs.size());
  if (!T || !(groups_running || workers_running || groups_allowed)) return PM_OK;
  ReportArgs a{};
  if ((rc = report_compat_args(e, &a.c))) return rc;
  if ((rc = report_groups(e, &a))) return rc;
  if ((rc = report_tasks(e, &a))) return rc;
  HIPCHK(e->d_rep_cnt.ensure(PM_MAX_CONFIGS));
  HIPCHK(e->d_rep_task.ensure(size_t(3) * T));
  HIPCHK(hipMemsetAsync(e->d_rep_cnt.p, 0, PM_MAX_CONFIGS * 4u, e->stream));
  HIPCHK(hipMemsetAsync(e->d_rep_task.p, 0, size_t(2) * T * 4u, e->stream));
  a.out = e->d_rep_cnt.p;
  a.running = e->d_rep_task.p;
  a.workers = e->d_rep_task.p + T;
  a.allowed = e->d_rep_task.p + size_t(2) * T;
  if (!C) HIPCHK(hipMemsetAsync(a.allowed, 0, size_t(T) * 4u, e->stream));
  else launch_task_report(a, 4u * e->n_cus, e->stream);
  HIPCHK(hipGetLastError());
  uint32_t* dst[3] = {groups_running, workers_running, groups_allowed};
  for (int k = 0; k < 3; ++k)
    if (dst[k]) HIPCHK(hipMemcpyAsync(dst[k], e->d_rep_task.p + size_t(k) * T, size_t(T) * 4u, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return PM_OK;
}
