// pm_engine_changes.inc — part of pm_engine.cpp (one translation unit; included in place): the assignment change feed: its
// buffers' growth, the resync flag, the launch behind a publish (inside namespace pm) — and, inside extern "C" (PM_CHANGES_ABI),
// C ABI: pm_enable_assignment_changes / pm_drain_assignment_changes (kernels in pm_changes.inc).
//
// publish_end calls changes_publish AFTER it has committed the table: a match that was queued and abandoned never gets here, so
// it leaves no trace in the feed's state.  The diff is launched on the engine's stream and not waited for: d_table, the committed
// task words (d_g_task behind publish_end's swap) and the feed's buffers are touched by nothing that is not queued on that stream
// behind it; the drain synchronises.  The three buffers keep the invariant that everything at or above chg_W reads zero — "in
// no group, nothing pending" — so rows appended between two publishes need no pass of their own.
#ifndef PM_CHANGES_ABI

// capacity for n elements, the first `keep` kept, everything behind them zero
template <typename T>
static int32_t changes_grow(DevBuf<T>& b, size_t n, size_t keep, hipStream_t s) {
  if (n <= b.cap) return PM_OK;
  HIPCHK(b.grow_keep(n, keep, s));
  HIPCHK(hipMemsetAsync(b.p + keep, 0, (b.cap - keep) * sizeof(T), s));
  return PM_OK;
}

static int32_t changes_clear_pending(pm_engine* e) {
  if (e->d_chg_what.p) HIPCHK(hipMemsetAsync(e->d_chg_what.p, 0, e->d_chg_what.cap, e->stream));
  if (e->d_chg_bitmap.p) HIPCHK(hipMemsetAsync(e->d_chg_bitmap.p, 0, e->d_chg_bitmap.cap * sizeof(uint64_t), e->stream));
  return PM_OK;
}

// the table in d_table has just been committed (publish_end): its difference against the remembered one joins the pending marks
static int32_t changes_publish(pm_engine* e) {
  const uint32_t W = e->W, W0 = e->chg_W;
  int32_t rc = changes_grow(e->d_chg_ident, std::max<uint32_t>(W, 1), W0, e->stream);
  if (!rc) rc = changes_grow(e->d_chg_what, std::max<uint32_t>(W, 1), W0, e->stream);
  if (!rc) rc = changes_grow(e->d_chg_bitmap, std::max<uint32_t>((W + 63u) / 64u, 1), (W0 + 63u) / 64u, e->stream);
  if (rc) return rc;
  if (e->chg_resync) {  // nothing remembered holds: every row compares as changed, and the marks of rows that may be gone go
    HIPCHK(hipMemsetAsync(e->d_chg_ident.p, 0, e->d_chg_ident.cap * sizeof(ChangeIdent), e->stream));
    if ((rc = changes_clear_pending(e))) return rc;
  }
  ChangeDiffArgs a{};
  a.W = W;
  a.G = uint32_t(std::min(e->groups.size(), e->d_g_task.cap));
  a.resync = e->chg_resync ? 1u : 0u;
  a.table = e->d_table.p;
  a.g_task = e->d_g_task.p;
  a.ident = e->d_chg_ident.p;
  a.what = e->d_chg_what.p;
  a.bitmap = e->d_chg_bitmap.p;
  launch_assign_diff(a, e->stream);
  HIPCHK(hipGetLastError());
  if (e->chg_resync) e->chg_resync = false, e->chg_resync_flag = true;
  e->chg_W = W;
  e->chg_list_valid = false;
  return PM_OK;
}

static void changes_release(pm_engine* e) {
  e->d_chg_ident.release(); e->d_chg_what.release(); e->d_chg_bitmap.release();
  e->d_chg_prefix.release(); e->d_chg_rows.release();
  if (e->h_chg_count) (void)hipHostFree(e->h_chg_count);
  e->h_chg_count = nullptr;
  e->chg_W = e->chg_n = 0;
  e->chg_resync_flag = e->chg_list_valid = false;
}

#else  // PM_CHANGES_ABI

int32_t pm_enable_assignment_changes(pm_engine* e, uint32_t on) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  if (e->dist_phase != 0) return set_error(PM_ESTATE, "a stepwise tick is in progress");
  if (on && e->dist_world > 1) return set_error(PM_ESTATE, "the assignment change feed does not cover multi-GPU engines");
  HIPCHK(hipSetDevice(e->cfg.device));
  e->chg_on = on != 0;
  if (e->chg_on) {
    e->chg_resync = true;  // (also when it was on already: the next publish lists every row)
  } else {
    HIPCHK(hipStreamSynchronize(e->stream));
    changes_release(e);
  }
  return PM_OK;
}

int32_t pm_drain_assignment_changes(pm_engine* e, pm_change_row* rows, uint32_t cap, uint32_t* n, uint32_t* flags) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  if (!e->chg_on) return set_error(PM_ESTATE, "the assignment change feed is off");
  HIPCHK(hipSetDevice(e->cfg.device));
  if (e->W < e->chg_W) {  // (the worker table was replaced by a shorter one: the marked rows are gone, the next publish lists all)
    int32_t rc = changes_clear_pending(e);
    if (rc) return rc;
    e->chg_W = e->W;
    e->chg_list_valid = false;
  }
  if (!e->chg_list_valid) {  // (a size query and the drain behind it make the list once)
    const uint32_t words = (e->chg_W + 63u) / 64u;
    e->chg_n = 0;
    if (words) {
      HIPCHK(e->d_chg_prefix.ensure(words));
      HIPCHK(e->d_chg_rows.ensure(e->chg_W));
      if (!e->h_chg_count) HIPCHK(hipHostMalloc((void**)&e->h_chg_count, sizeof(uint32_t)));
      launch_change_list(e->d_chg_bitmap.p, words, e->d_chg_what.p, e->d_chg_prefix.p, e->h_chg_count, e->d_chg_rows.p, e->stream);
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(e->stream));
      e->chg_n = *e->h_chg_count;
      if (e->chg_n > e->chg_W) return set_error(PM_ESTATE, "change feed: more pending rows than rows");
    }
    e->chg_list_valid = true;
  }
  const uint32_t pending = e->chg_n;
  if (n) *n = pending;
  if (flags) *flags = e->chg_resync_flag ? PM_CHANGES_RESYNC : 0u;
  if (!rows || cap < pending) return set_error(PM_ERANGE, "change row buffer too small");
  if (pending) {
    HIPCHK(hipMemcpyAsync(rows, e->d_chg_rows.p, size_t(pending) * sizeof(pm_change_row), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemsetAsync(e->d_chg_what.p, 0, e->chg_W, e->stream));
    HIPCHK(hipMemsetAsync(e->d_chg_bitmap.p, 0, size_t((e->chg_W + 63u) / 64u) * sizeof(uint64_t), e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  e->chg_n = 0;  // (the list stays valid: it is empty until the next publish)
  e->chg_resync_flag = false;
  return PM_OK;
}

#endif
