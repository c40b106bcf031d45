// pm_engine_groupdir.inc — part of pm_engine.cpp (one translation unit; included in place): the group directory, C ABI:
// pm_group_directory (kernels in pm_groupdir.inc).  Included at file scope.
//
// The group directory owns no ledger: it joins the host's groups with the liveness ledger (the members' statuses) and the
// rollout ledger (what the members report against the group's claim), per group, filters and orders them, and hands out one
// window of the list and the counters.  e->gdir is scratch of one call.  What goes up is what pm_directory sends: h_group_of and
// one record per list entry; the tick's device mirror (d_g_*) and its delta state are not touched.  The window's members are
// laid out from the host's own list — they never were on the device's side of the join, so they do not cross PCIe twice.
// Everything is queued on the engine's stream; a call synchronises once for the counters and once more only when it has a
// window.  Like the rollout reads it leaves the tick's state alone: no pending delta is consumed, nothing is compacted, no
// cache flag is cleared.
extern "C" {

int32_t pm_group_directory(pm_engine* e, const pm_gdir_query* q, pm_gdir_totals* totals, uint32_t* by_config, uint32_t cap_cfgs,
                           pm_gdir_row* rows, uint32_t cap_rows, uint32_t* n_rows, uint32_t* members, uint32_t cap_members,
                           uint32_t* n_members) {
  static_assert(sizeof(pm_gdir_row) == 80 && sizeof(pm_gdir_query) == 40 && sizeof(pm_gdir_totals) == 36, "pm_gdir_* layout");
  constexpr uint32_t all_health = (1u << PM_GH_N) - 1u, all_rollout = (1u << PM_GR_N) - 1u;
  if (!e || !q || !totals || !n_rows || !n_members) return set_error(PM_EINVAL, "null argument");
  if (!q->config_mask) return set_error(PM_EINVAL, "not a set of configurations");
  if (!q->health_mask || (q->health_mask & ~all_health)) return set_error(PM_EINVAL, "not a set of health classes");
  if (!q->rollout_mask || (q->rollout_mask & ~all_rollout)) return set_error(PM_EINVAL, "not a set of rollout classes");
  if (q->holds > PM_GDIR_WITHOUT_TASK) return set_error(PM_EINVAL, "not a holds (PM_GDIR_ANY / _WITH_TASK / _WITHOUT_TASK)");
  if (q->order > PM_GDIR_BY_SIZE_DESC) return set_error(PM_EINVAL, "not an order (PM_GDIR_BY_SLOT / _BY_ID_TEXT / _BY_SIZE_DESC)");
  if (q->size_min > q->size_max) return set_error(PM_EINVAL, "size_min > size_max");
  std::lock_guard<std::mutex> lk(e->mu);
  if (e->dist_phase != 0) return set_error(PM_ESTATE, "a stepwise tick is in progress");
  if (e->dist_world > 1) return set_error(PM_ESTATE, "the group directory does not cover multi-GPU engines");
  if (!e->have_cfgs) return set_error(PM_ESTATE, "configurations must be set first");
  if (!e->have_workers) return set_error(PM_ESTATE, "workers must be uploaded first");
  if (!e->live.on && q->health_mask != all_health) return set_error(PM_ESTATE, "a health filter needs liveness, which is off");
  if (!e->ro.on && q->rollout_mask != all_rollout) return set_error(PM_ESTATE, "a rollout filter needs the rollout ledger, which is off");
  if (e->ro.on && e->have_tasks && !e->tasks_have_uid && e->T)
    return set_error(PM_ESTATE, "the task table carries no ids (pm_task_soa.uid)");
  HIPCHK(hipSetDevice(e->cfg.device));
  ABSORB_PENDING(e);  // (the groups of a tick that has not been taken in yet: pm_get_groups would report them)
  if (e->groups.size() > 0x0FFFFFFFu) return set_error(PM_ERANGE, "group list too large for the group directory");
  int32_t rc;
  if (e->live.on && (rc = liveness_prepare(e))) return rc;
  if (e->ro.on && (rc = rollout_prepare(e))) return rc;
  GroupDir& d = e->gdir;
  const uint32_t W = e->W, G = uint32_t(e->groups.size()), n_cfgs = uint32_t(e->cfgs.size());
  HIPCHK(d.pg.pin(PM_GD_CENSUS));
  GdirArgs a{};
  uint32_t n_listed = 0;
  if (G) {
    group_records(e, d.h_g, &d.h_of_slot);
    a.n_cls = q->order == PM_GDIR_BY_ID_TEXT ? PM_GD_TEXT_CLASSES : 1u;
    if ((rc = upload(d.gof, e->h_group_of.data(), size_t(W), e->stream))) return rc;
    if ((rc = upload(d.g, d.h_g.data(), size_t(G), e->stream))) return rc;
    const size_t n_cnt = size_t(G) * PM_GD_CNT + PM_GD_CENSUS, n_flag = size_t(a.n_cls) * G;
    HIPCHK(d.cnt.ensure(n_cnt));
    HIPCHK(d.cls.ensure(G));
    HIPCHK(d.hr.ensure(2 * size_t(G)));
    HIPCHK(d.pg.flag.ensure(n_flag));
    HIPCHK(d.pg.off.ensure(n_flag + 1));
    HIPCHK(hipMemsetAsync(d.cnt.p, 0, n_cnt * sizeof(uint32_t), e->stream));
    a.W = W, a.G = G;
    a.config_mask = q->config_mask;
    a.holds = q->holds, a.size_min = q->size_min, a.size_max = q->size_max;
    a.health_mask = q->health_mask, a.rollout_mask = q->rollout_mask, a.order = q->order;
    a.group_of = d.gof.p;
    a.g = d.g.p;
    a.status = e->live.on ? e->live.status.p : nullptr;
    a.uid = e->ro.on ? e->ro.uid.p : nullptr;
    a.state = e->ro.on ? e->ro.state.p : nullptr;
    a.g_cnt = d.cnt.p;
    a.census = d.cnt.p + size_t(G) * PM_GD_CNT;
    a.cls = d.cls.p;
    a.hr = d.hr.p;
    a.flag = d.pg.flag.p;
    a.off = d.pg.off.p;
    launch_gdir_members(a, e->stream);
    launch_gdir_groups(a, e->stream);
    if ((rc = page_counters(d.pg, uint32_t(n_flag), a.census, PM_GD_CENSUS, e->stream, &n_listed))) return rc;
  }
  if (n_listed > G) return set_error(PM_ESTATE, "group directory: more listed groups than groups");
  const uint32_t* c = d.pg.h_pin.p + 1;
  totals->total = n_listed;
  totals->members_total = c[PM_GD_CENSUS - 1];
  std::copy(c + PM_MAX_CONFIGS, c + PM_MAX_CONFIGS + PM_GH_N, totals->by_health);
  std::copy(c + PM_MAX_CONFIGS + PM_GH_N, c + PM_MAX_CONFIGS + PM_GH_N + PM_GR_N, totals->by_rollout);
  totals->n_cfgs = n_cfgs;
  const uint32_t n = q->offset >= n_listed ? 0u : std::min(q->limit, n_listed - q->offset);
  *n_rows = n;
  *n_members = 0;
  const bool cfgs_fit = !by_config || cap_cfgs >= n_cfgs;
  if (by_config && cfgs_fit) std::copy(c, c + n_cfgs, by_config);
  if (n) {
    a.offset = q->offset, a.n_rows = n;
    const uint32_t* list = nullptr;
    // BY_ID_TEXT: every byte of A, eight passes; BY_SIZE_DESC: the four bytes of UINT32_MAX - size
    const uint32_t passes = q->order == PM_GDIR_BY_SLOT ? 0u : q->order == PM_GDIR_BY_ID_TEXT ? 8u : 4u;
    const hipStream_t s = e->stream;  // (the callables capture the arguments, the stream and the index space, by value but for a)
    rc = page_list(
        d.pg, n_listed, q->offset, n, passes, s, [&a, s, G](uint32_t* win) { a.win = win, launch_list_window(a, G, s); },
        [&a, s](uint64_t* key, uint32_t* val) { a.key = key, a.val = val, launch_gdir_keys(a, s); }, &list);
    if (rc) return rc;
    HIPCHK(d.rows.ensure(n));
    d.h_rows.resize(n);
    launch_gdir_emit(a, list, n, d.rows.p, e->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(d.h_rows.data(), d.rows.p, size_t(n) * sizeof(pm_gdir_row), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    uint64_t m_total = 0;
    for (uint32_t k = 0; k < n; ++k) {
      pm_gdir_row& r = d.h_rows[k];
      if (r.slot >= d.h_of_slot.size() || m_total > W) return set_error(PM_ESTATE, "group directory: a row names no live group");
      r.member_begin = uint32_t(m_total);
      m_total += r.size;
    }
    if (m_total > W) return set_error(PM_ESTATE, "group directory: more members than workers");
    *n_members = uint32_t(m_total);
  }
  if (!cfgs_fit) return set_error(PM_ERANGE, "group directory configuration buffer too small");
  if (n && (!rows || cap_rows < n)) return set_error(PM_ERANGE, "group directory row buffer too small");
  if (members && cap_members < *n_members) return set_error(PM_ERANGE, "group directory member buffer too small");
  if (!n) return PM_OK;
  std::copy(d.h_rows.begin(), d.h_rows.begin() + n, rows);
  if (members) {
    // a group's members in ascending addr_rank, equal ranks by ascending row: a defined order
    for (uint32_t k = 0; k < n; ++k) {
      const Group& gr = e->groups[d.h_of_slot[rows[k].slot]];
      uint32_t* m = members + rows[k].member_begin;
      std::copy(gr.members.begin(), gr.members.end(), m);
      std::sort(m, m + gr.members.size(), [&](uint32_t x, uint32_t y) {
        return e->h_addr_rank[x] != e->h_addr_rank[y] ? e->h_addr_rank[x] < e->h_addr_rank[y] : x < y;
      });
    }
  }
  return PM_OK;
}

}  // extern "C"
