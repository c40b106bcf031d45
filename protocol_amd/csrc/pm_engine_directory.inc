// pm_engine_directory.inc — part of pm_engine.cpp (one translation unit; included in place): the node directory, C ABI:
// pm_directory (kernels in pm_directory.inc).  Included at file scope.
//
// The directory owns no ledger: it joins the liveness ledger (the status), the host's groups and, where it is on, the rollout
// ledger, per worker row, in the reference's listing order (NodeStore::get_nodes), and hands out one window of the list and
// the counters.  e->dir is scratch of one call.  Everything is queued on the engine's stream; a call synchronises once for the
// counters and once more only when it copies rows.  Like the rollout reads it leaves the tick's state alone: no pending delta
// is consumed, nothing is compacted, no cache flag is cleared.
extern "C" {

int32_t pm_directory(pm_engine* e, const pm_dir_query* q, uint32_t* total, uint32_t* counts, pm_dir_row* rows, uint32_t cap,
                     uint32_t* n_rows) {
  if (!e || !q || !total || !n_rows) return set_error(PM_EINVAL, "null argument");
  if (!q->status_mask || (q->status_mask >> PM_NS_N)) return set_error(PM_EINVAL, "not a set of node statuses");
  if (q->membership > PM_DIR_UNGROUPED) return set_error(PM_EINVAL, "not a membership (PM_DIR_ANY / _GROUPED / _UNGROUPED)");
  if (q->order > PM_DIR_BY_ADDRESS) return set_error(PM_EINVAL, "not an order (PM_DIR_BY_ROW / _BY_ADDRESS)");
  std::lock_guard<std::mutex> lk(e->mu);
  int32_t rc = liveness_guard(e);  // (liveness is the status: off, there is nothing to list)
  if (rc) return rc;
  if (e->W > 0x3FFFFFFFu) return set_error(PM_ERANGE, "worker table too large for the directory");
  HIPCHK(hipSetDevice(e->cfg.device));
  ABSORB_PENDING(e);  // (the groups of a tick that has not been taken in yet: pm_get_groups would report them)
  if ((rc = liveness_prepare(e))) return rc;
  if (e->ro.on && (rc = rollout_prepare(e))) return rc;
  Directory& d = e->dir;
  const uint32_t W = e->W, G = uint32_t(e->groups.size());
  HIPCHK(d.pg.pin(PM_NS_N));
  DirArgs a{};
  uint32_t n_listed = 0;
  if (W) {
    group_records(e, d.h_g);
    if ((rc = upload(d.gof, e->h_group_of.data(), size_t(W), e->stream))) return rc;
    if ((rc = upload(d.g, d.h_g.data(), size_t(G), e->stream))) return rc;
    const size_t n_flag = size_t(PM_DC_N) * W;
    HIPCHK(d.cls.ensure(W));
    HIPCHK(d.pg.flag.ensure(n_flag));
    HIPCHK(d.pg.off.ensure(n_flag + 1));
    HIPCHK(d.census.ensure(PM_NS_N));
    HIPCHK(hipMemsetAsync(d.census.p, 0, PM_NS_N * sizeof(uint32_t), e->stream));
    a.W = W, a.G = G;
    a.status_mask = q->status_mask, a.membership = q->membership;
    a.status = e->live.status.p;
    a.counter = e->live.counter.p;
    a.group_of = d.gof.p;
    a.g = d.g.p;
    a.addr_rank = e->d_addr_rank.p;
    a.uid = e->ro.on ? e->ro.uid.p : nullptr;
    a.state = e->ro.on ? e->ro.state.p : nullptr;
    a.cls = d.cls.p;
    a.flag = d.pg.flag.p;
    a.census = d.census.p;
    a.off = d.pg.off.p;
    launch_dir_classify(a, e->stream);
    if ((rc = page_counters(d.pg, uint32_t(n_flag), d.census.p, PM_NS_N, e->stream, &n_listed))) return rc;
  }
  if (n_listed > W) return set_error(PM_ESTATE, "directory: more listed rows than rows");
  const uint32_t n = q->offset >= n_listed ? 0u : std::min(q->limit, n_listed - q->offset);
  *total = n_listed;
  if (counts) std::copy(d.pg.h_pin.p + 1, d.pg.h_pin.p + 1 + PM_NS_N, counts);
  *n_rows = n;
  if (n && (!rows || cap < n)) return set_error(PM_ERANGE, "directory row buffer too small");
  if (!n) return PM_OK;
  a.offset = q->offset, a.n_rows = n;
  const uint32_t* list = nullptr;
  const uint32_t passes = q->order == PM_DIR_BY_ROW ? 0u : 5u;  // BY_ADDRESS: 32 bits of rank, the class's two in the fifth byte
  const hipStream_t s = e->stream;  // (the callables capture the arguments, the stream and the index space, by value but for a)
  rc = page_list(
      d.pg, n_listed, q->offset, n, passes, s, [&a, s, W](uint32_t* win) { a.win = win, launch_list_window(a, W, s); },
      [&a, s](uint64_t* key, uint32_t* val) { a.key = key, a.val = val, launch_dir_keys(a, s); }, &list);
  if (rc) return rc;
  HIPCHK(d.rows.ensure(n));
  launch_dir_emit(a, list, n, d.rows.p, e->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(rows, d.rows.p, size_t(n) * sizeof(pm_dir_row), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return PM_OK;
}

}  // extern "C"
