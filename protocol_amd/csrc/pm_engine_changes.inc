// pm_engine_changes.inc — part of pm_engine.cpp (one translation unit; included in place): the assignment change feed: its
// buffers' growth, the resync flag, the launch behind a publish (namespace pm) — and, behind them (extern "C"), C ABI:
// pm_enable_assignment_changes / pm_drain_assignment_changes (kernels in pm_changes.inc).  Included at file scope.
//
// publish_end calls changes_publish AFTER it has committed the table: a match that was queued and abandoned never gets here, so
// it leaves no trace in the feed's state.  The diff is launched on the engine's stream and not waited for: d_table, the committed
// task words (d_g_task behind publish_end's swap) and the feed's buffers are touched by nothing that is not queued on that stream
// behind it; the drain synchronises.  The three buffers keep the invariant that everything at or above chg.W reads zero — "in
// no group, nothing pending" — so rows appended between two publishes need no pass of their own.
namespace pm {

// capacity for n elements, the first `keep` kept, everything behind them zero
template <typename T>
static int32_t changes_grow(DevBuf<T>& b, size_t n, size_t keep, hipStream_t s) {
  if (n <= b.cap) return PM_OK;
  HIPCHK(b.grow_keep(n, keep, s));
  HIPCHK(hipMemsetAsync(b.p + keep, 0, (b.cap - keep) * sizeof(T), s));
  return PM_OK;
}

static int32_t changes_clear_pending(pm_engine* e) {
  if (e->chg.what.p) HIPCHK(hipMemsetAsync(e->chg.what.p, 0, e->chg.what.cap, e->stream));
  if (e->chg.bitmap.p) HIPCHK(hipMemsetAsync(e->chg.bitmap.p, 0, e->chg.bitmap.cap * sizeof(uint64_t), e->stream));
  return PM_OK;
}

// the table in d_table has just been committed (publish_end): its difference against the remembered one joins the pending marks
static int32_t changes_publish(pm_engine* e) {
  const uint32_t W = e->W, W0 = e->chg.W;
  int32_t rc = changes_grow(e->chg.ident, std::max<uint32_t>(W, 1), W0, e->stream);
  if (!rc) rc = changes_grow(e->chg.what, std::max<uint32_t>(W, 1), W0, e->stream);
  if (!rc) rc = changes_grow(e->chg.bitmap, std::max<uint32_t>((W + 63u) / 64u, 1), (W0 + 63u) / 64u, e->stream);
  if (rc) return rc;
  if (e->chg.resync) {  // nothing remembered holds: every row compares as changed, and the marks of rows that may be gone go
    HIPCHK(hipMemsetAsync(e->chg.ident.p, 0, e->chg.ident.cap * sizeof(ChangeIdent), e->stream));
    if ((rc = changes_clear_pending(e))) return rc;
  }
  ChangeDiffArgs a{};
  a.W = W;
  a.G = uint32_t(std::min(e->groups.size(), e->d_g_task.cap));
  a.resync = e->chg.resync ? 1u : 0u;
  a.table = e->d_table.p;
  a.g_task = e->d_g_task.p;
  a.ident = e->chg.ident.p;
  a.what = e->chg.what.p;
  a.bitmap = e->chg.bitmap.p;
  launch_assign_diff(a, e->stream);
  HIPCHK(hipGetLastError());
  if (e->chg.resync) e->chg.resync = false, e->chg.resync_flag = true;
  e->chg.W = W;
  e->chg.list_valid = false;
  return PM_OK;
}

// a fresh feed: every buffer goes back; whether it is on, and that the next publish lists every row, stay
static void changes_release(pm_engine* e) {
  ChangeFeed fresh;
  fresh.on = e->chg.on, fresh.resync = e->chg.resync;
  e->chg = std::move(fresh);
}

}  // namespace pm

extern "C" {

int32_t pm_enable_assignment_changes(pm_engine* e, uint32_t on) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  if (e->dist_phase != 0) return set_error(PM_ESTATE, "a stepwise tick is in progress");
  if (on && e->dist_world > 1) return set_error(PM_ESTATE, "the assignment change feed does not cover multi-GPU engines");
  HIPCHK(hipSetDevice(e->cfg.device));
  e->chg.on = on != 0;
  if (e->chg.on) {
    e->chg.resync = true;  // (also when it was on already: the next publish lists every row)
  } else {
    HIPCHK(hipStreamSynchronize(e->stream));
    changes_release(e);
  }
  return PM_OK;
}

int32_t pm_drain_assignment_changes(pm_engine* e, pm_change_row* rows, uint32_t cap, uint32_t* n, uint32_t* flags) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  if (!e->chg.on) return set_error(PM_ESTATE, "the assignment change feed is off");
  HIPCHK(hipSetDevice(e->cfg.device));
  if (e->W < e->chg.W) {  // (the worker table was replaced by a shorter one: the marked rows are gone, the next publish lists all)
    int32_t rc = changes_clear_pending(e);
    if (rc) return rc;
    e->chg.W = e->W;
    e->chg.list_valid = false;
  }
  if (!e->chg.list_valid) {  // (a size query and the drain behind it make the list once)
    const uint32_t words = (e->chg.W + 63u) / 64u;
    e->chg.n = 0;
    if (words) {
      HIPCHK(e->chg.prefix.ensure(words));
      HIPCHK(e->chg.rows.ensure(e->chg.W));
      HIPCHK(e->chg.h_count.ensure(1, 1));
      launch_change_list(e->chg.bitmap.p, words, e->chg.what.p, e->chg.prefix.p, e->chg.h_count.p, e->chg.rows.p, e->stream);
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(e->stream));
      e->chg.n = *e->chg.h_count.p;
      if (e->chg.n > e->chg.W) return set_error(PM_ESTATE, "change feed: more pending rows than rows");
    }
    e->chg.list_valid = true;
  }
  const uint32_t pending = e->chg.n;
  if (n) *n = pending;
  if (flags) *flags = e->chg.resync_flag ? PM_CHANGES_RESYNC : 0u;
  if (!rows || cap < pending) return set_error(PM_ERANGE, "change row buffer too small");
  if (pending) {
    HIPCHK(hipMemcpyAsync(rows, e->chg.rows.p, size_t(pending) * sizeof(pm_change_row), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemsetAsync(e->chg.what.p, 0, e->chg.W, e->stream));
    HIPCHK(hipMemsetAsync(e->chg.bitmap.p, 0, size_t((e->chg.W + 63u) / 64u) * sizeof(uint64_t), e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  e->chg.n = 0;  // (the list stays valid: it is empty until the next publish)
  e->chg.resync_flag = false;
  return PM_OK;
}

}  // extern "C"
