// pm_engine_taskdir.inc — part of pm_engine.cpp (one translation unit; included in place): the task directory, C ABI:
// pm_task_directory (kernels in pm_taskdir.inc).  Included at file scope.
//
// The task directory owns no ledger: it joins the task table with the host's groups (their claims, the live groups of every
// configuration) and with the rollout ledger (what the nodes report, by id), per task, filters and orders them, and hands out
// one window of the list and the counters.  e->tdir is scratch of one call.  What goes up is one record per entry of the group
// list and, with rollout on, the ids of the live rows (the device has no id column: h_tuid is the host's); the task index space
// is read where the tick keeps it.  With rollout on the ledger's own read makes its per-task table first (rollout_read: what
// pm_rollout_tasks runs, taken over as it is) and the directory joins its runs to the rows.  Everything is queued on the
// engine's stream.  Like the reports it leaves the tick's state alone: no pending delta is consumed, nothing is compacted, no
// cache flag is cleared (the live prefix goes to the reports' scratch while the tick's is stale).
extern "C" {

int32_t pm_task_directory(pm_engine* e, const pm_tdir_query* q, pm_tdir_totals* totals, uint32_t* by_config, uint32_t cap_cfgs,
                          pm_tdir_row* rows, uint32_t cap_rows, uint32_t* n_rows) {
  static_assert(sizeof(pm_tdir_row) == 88 && sizeof(pm_tdir_query) == 40 && sizeof(pm_tdir_totals) == 56, "pm_tdir_* layout");
  static_assert(sizeof(TdirGroup) == 16, "TdirGroup layout");
  constexpr uint32_t all_serve = (1u << PM_TKS_N) - 1u, all_rollout = (1u << PM_TKR_N) - 1u;
  if (!e || !q || !totals || !n_rows) return set_error(PM_EINVAL, "null argument");
  if (!q->config_mask) return set_error(PM_EINVAL, "not a set of configurations");
  if (!q->serve_mask || (q->serve_mask & ~all_serve)) return set_error(PM_EINVAL, "not a set of serving classes");
  if (!q->rollout_mask || (q->rollout_mask & ~all_rollout)) return set_error(PM_EINVAL, "not a set of rollout classes");
  if (q->order > PM_TDIR_BY_REPORTERS_DESC)
    return set_error(PM_EINVAL, "not an order (PM_TDIR_BY_LIST / _BY_OLDEST / _BY_WORKERS_DESC / _BY_REPORTERS_DESC)");
  if (q->workers_min > q->workers_max) return set_error(PM_EINVAL, "workers_min > workers_max");
  std::lock_guard<std::mutex> lk(e->mu);
  if (e->dist_phase != 0) return set_error(PM_ESTATE, "a stepwise tick is in progress");
  if (e->dist_world > 1) return set_error(PM_ESTATE, "the task directory does not cover multi-GPU engines");
  if (!e->have_cfgs) return set_error(PM_ESTATE, "configurations must be set first");
  if (!e->have_workers) return set_error(PM_ESTATE, "workers must be uploaded first");
  if (!e->have_tasks) return set_error(PM_ESTATE, "tasks must be uploaded first");
  if (!e->ro.on && q->rollout_mask != all_rollout) return set_error(PM_ESTATE, "a rollout filter needs the rollout ledger, which is off");
  if (!e->ro.on && q->order == PM_TDIR_BY_REPORTERS_DESC)
    return set_error(PM_ESTATE, "the order by reporters needs the rollout ledger, which is off");
  if (e->ro.on && !e->tasks_have_uid && e->T) return set_error(PM_ESTATE, "the task table carries no ids (pm_task_soa.uid)");
  if (e->t_cap >= (1u << 28)) return set_error(PM_ERANGE, "task index space too large for the task directory");
  HIPCHK(hipSetDevice(e->cfg.device));
  ABSORB_PENDING(e);  // (the groups of a tick that has not been taken in yet: pm_get_groups would report them)
  int32_t rc;
  uint32_t D = 0;  // rows of the rollout ledger's per-task table
  if (e->ro.on) {
    RoPrepArgs ra;
    uint32_t listed = 0;
    if ((rc = rollout_read(e, true, &ra, &listed, &D))) return rc;
  }
  TaskDir& d = e->tdir;
  const uint32_t G = uint32_t(e->groups.size()), n_cfgs = uint32_t(e->cfgs.size());
  const uint32_t R = e->t_cap - e->t_lo;  // slots: the used part of the index space, tombstones included
  HIPCHK(d.pg.pin(PM_TD_CENSUS));
  TdirArgs a{};
  uint32_t n_listed = 0;
  if (R) {
    d.h_g.resize(G);
    for (uint32_t k = 0; k < G; ++k) {
      const Group& gr = e->groups[k];
      d.h_g[k] = TdirGroup{gr.cfg, uint32_t(gr.members.size()), gr.dead ? PM_NONE : gr.task, gr.dead ? 0u : 1u};
    }
    if ((rc = upload(d.g, d.h_g.data(), size_t(G), e->stream))) return rc;
    ReportArgs ta{};
    if ((rc = report_tasks(e, &ta))) return rc;
    const size_t n_cnt = size_t(R) * PM_TD_CNT + PM_MAX_CONFIGS + PM_TD_CENSUS;
    HIPCHK(d.cnt.ensure(n_cnt));
    HIPCHK(d.cls.ensure(2 * size_t(R)));
    HIPCHK(d.pg.flag.ensure(R));
    HIPCHK(d.pg.off.ensure(size_t(R) + 1));
    HIPCHK(hipMemsetAsync(d.cnt.p, 0, n_cnt * sizeof(uint32_t), e->stream));
    a.G = G, a.n_cfgs = n_cfgs, a.t_lo = e->t_lo, a.t_cap = e->t_cap;
    a.config_mask = q->config_mask;
    a.serve_mask = q->serve_mask, a.rollout_mask = q->rollout_mask;
    a.workers_min = q->workers_min, a.workers_max = q->workers_max, a.order = q->order;
    a.rollout_on = e->ro.on ? 1u : 0u;
    a.g = d.g.p;
    a.ro_gcnt = e->ro.on && G ? e->ro.cnt.p : nullptr;
    a.tmask = ta.tmask, a.tlive = ta.tlive, a.tprefix = ta.tprefix;
    a.created = e->d_created.p;
    a.cnt = d.cnt.p;
    a.g_per_cfg = d.cnt.p + size_t(R) * PM_TD_CNT;
    a.census = a.g_per_cfg + PM_MAX_CONFIGS;
    a.cls = d.cls.p;
    a.flag = d.pg.flag.p;
    a.off = d.pg.off.p;
    launch_tdir_groups(a, e->stream);
    if (D) {
      // the live rows' (id, slot) pairs in list order; sorted by id they keep that order inside a run of equal ids
      d.h_key.clear();
      d.h_val.clear();
      for (uint32_t u = e->t_lo; u < e->t_cap; ++u)
        if ((e->h_tlive[u >> 6] >> (u & 63u)) & 1ull) {
          d.h_key.push_back(e->h_tuid[u]);
          d.h_val.push_back(u - e->t_lo);
        }
      const uint32_t n_pairs = uint32_t(d.h_key.size());
      KeySort& ks = d.pg.sort;
      if ((rc = upload(ks.key[0], d.h_key.data(), size_t(n_pairs), e->stream))) return rc;
      if ((rc = upload(ks.val[0], d.h_val.data(), size_t(n_pairs), e->stream))) return rc;
      uint32_t cur = 0;
      if (n_pairs) {
        HIPCHK(ks.ensure(n_pairs));
        cur = ks.sort(n_pairs, 8u, 0u, e->stream);  // every byte of the id
      }
      launch_tdir_join(a, e->ro.task_rows.p, D, ks.key[cur].p, ks.val[cur].p, n_pairs, e->stream);
    }
    launch_tdir_tasks(a, e->stream);
    if ((rc = page_counters(d.pg, R, a.census, PM_TD_CENSUS, e->stream, &n_listed))) return rc;
  } else if (D) {
    // no slot at all: every reported id is an orphan
    d.h_rows.clear();
    std::vector<pm_ro_task_row> runs(D);
    HIPCHK(hipMemcpyAsync(runs.data(), e->ro.task_rows.p, size_t(D) * sizeof(pm_ro_task_row), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    d.pg.h_pin.p[1 + TD_C_ORPHAN_UIDS] = D;
    for (const pm_ro_task_row& r : runs)
      for (uint32_t s = 0; s < PM_TS_N; ++s) d.pg.h_pin.p[1 + TD_C_ORPHAN_REPORTERS] += r.reporters[s];
  }
  if (n_listed > e->T) return set_error(PM_ESTATE, "task directory: more listed tasks than tasks");
  const uint32_t* c = d.pg.h_pin.p + 1;
  totals->tasks = e->T;
  totals->total = n_listed;
  std::copy(c + TD_C_SERVE, c + TD_C_SERVE + PM_TKS_N, totals->by_serve);
  std::copy(c + TD_C_ROLLOUT, c + TD_C_ROLLOUT + PM_TKR_N, totals->by_rollout);
  totals->unrestricted = c[TD_C_UNRESTRICTED];
  totals->workers_running = c[TD_C_WORKERS];
  totals->reporters = c[TD_C_REPORTERS];
  totals->orphan_uids = c[TD_C_ORPHAN_UIDS];
  totals->orphan_reporters = c[TD_C_ORPHAN_REPORTERS];
  totals->n_cfgs = n_cfgs;
  const uint32_t n = q->offset >= n_listed ? 0u : std::min(q->limit, n_listed - q->offset);
  *n_rows = n;
  const bool cfgs_fit = !by_config || cap_cfgs >= n_cfgs;
  if (by_config && cfgs_fit) std::copy(c, c + n_cfgs, by_config);
  if (!cfgs_fit) return set_error(PM_ERANGE, "task directory configuration buffer too small");
  if (n && (!rows || cap_rows < n)) return set_error(PM_ERANGE, "task directory row buffer too small");
  if (!n) return PM_OK;
  a.offset = q->offset, a.n_rows = n, a.total = n_listed;
  const uint32_t* list = nullptr;
  // BY_LIST and BY_OLDEST are scan order; the _DESC orders: the four bytes of UINT32_MAX - value
  const uint32_t passes = q->order == PM_TDIR_BY_LIST || q->order == PM_TDIR_BY_OLDEST ? 0u : 4u;
  const hipStream_t s = e->stream;  // (the callables capture the arguments, the stream and the index space, by value but for a)
  rc = page_list(
      d.pg, n_listed, q->offset, n, passes, s, [&a, s, R](uint32_t* win) { a.win = win, launch_list_window(a, R, s); },
      [&a, s](uint64_t* key, uint32_t* val) { a.key = key, a.val = val, launch_tdir_keys(a, s); }, &list);
  if (rc) return rc;
  HIPCHK(d.rows.ensure(n));
  HIPCHK(d.handles.ensure(n));
  d.h_rows.resize(n);
  d.h_handles.resize(n);
  launch_tdir_emit(a, list, n, d.rows.p, d.handles.p, e->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(d.h_rows.data(), d.rows.p, size_t(n) * sizeof(pm_tdir_row), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(d.h_handles.data(), d.handles.p, size_t(n) * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  for (uint32_t k = 0; k < n; ++k) {
    const uint32_t u = d.h_handles[k];
    if (u < e->t_lo || u >= e->t_cap) return set_error(PM_ESTATE, "task directory: a row names no slot of the table");
    d.h_rows[k].uid = e->tasks_have_uid ? e->h_tuid[u] : 0ull;
  }
  std::copy(d.h_rows.begin(), d.h_rows.end(), rows);
  return PM_OK;
}

}  // extern "C"
