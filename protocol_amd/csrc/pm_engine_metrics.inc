// pm_engine_metrics.inc — part of pm_engine.cpp (one translation unit; included in place): the metrics ledger: its buffers, their
// growth, the rebuild every change of the table goes through, the liveness hook (namespace pm) — and, behind them (extern "C"),
// C ABI: pm_metrics_enable / _ingest / _totals / _rows (kernels in pm_metrics.inc).  Included at file scope.
//
// The table is a CSR over the internal rows [0, mx.R): row 0 is the manual row, row w + 1 worker w, so the manual row's entries
// are the first of the arrays and "ascending row, the manual row first" is the arrays' own order.  It lives in two buffers: a
// change writes the other one from the current one and swaps when everything has been written, so a refused batch leaves
// nothing behind.  pm_upload_workers(keep_groups = 0) sets mx.reinit, the one hook in the upload path; everything else happens
// when the next metrics call runs metrics_prepare.  Everything is queued on the engine's stream.  Like the reports, a metrics
// call leaves the tick's state alone: no pending delta is consumed, nothing is compacted, no cache flag is cleared.
namespace pm {

// a fresh ledger: every buffer goes back; whether it is on stays
static void metrics_release(pm_engine* e) {
  Metrics fresh;
  fresh.on = e->mx.on;
  e->mx = std::move(fresh);
}

// the table covers the manual row and the workers [0, W): creates it, extends the offsets over appended rows, empties the
// worker rows behind an upload that dropped the row identities (queued, not waited for)
static int32_t metrics_prepare(pm_engine* e) {
  const uint32_t R = (e->have_workers ? e->W : 0u) + 1u;
  if (!e->mx.h_pin.p) {
    HIPCHK(e->mx.h_pin.ensure(4, 4));
    std::memset(e->mx.h_pin.p, 0, 4 * sizeof(uint32_t));
  }
  DevBuf<uint32_t>& off = e->mx.off[e->mx.cur];
  if (!e->mx.R) {  // a fresh ledger: every row empty
    HIPCHK(off.ensure(size_t(R) + 1));
    launch_mx_fill(off.p, 0, R + 1u, 0u, e->stream);
    HIPCHK(hipGetLastError());
    e->mx.R = R, e->mx.N = 0;
    e->mx.reinit = e->mx.totals_valid = false;
    return PM_OK;
  }
  if (e->mx.reinit || R < e->mx.R) {  // (a shorter table is a new table) the manual row's entries are the arrays' first off[1]
    uint32_t n0 = 0;
    HIPCHK(hipMemcpyAsync(&n0, off.p + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(off.grow_keep(size_t(R) + 1, 2, e->stream));
    launch_mx_fill(off.p, 1u, R + 1u, n0, e->stream);
    HIPCHK(hipGetLastError());
    e->mx.R = R, e->mx.N = n0;
    e->mx.reinit = e->mx.totals_valid = false;
    return PM_OK;
  }
  if (R > e->mx.R) {  // appended workers start empty
    HIPCHK(off.grow_keep(size_t(R) + 1, size_t(e->mx.R) + 1, e->stream));
    launch_mx_fill(off.p, e->mx.R + 1u, R + 1u, e->mx.N, e->stream);
    HIPCHK(hipGetLastError());
    e->mx.R = R;
  }
  return PM_OK;
}

// what every metrics call but pm_metrics_enable asks first
static int32_t metrics_guard(pm_engine* e) {
  if (!e->mx.on) return set_error(PM_ESTATE, "the metrics ledger is off");
  if (e->dist_phase != 0) return set_error(PM_ESTATE, "a stepwise tick is in progress");
  if (e->dist_world > 1) return set_error(PM_ESTATE, "the metrics ledger does not cover multi-GPU engines");
  return PM_OK;
}

// The other buffer from the current one.  mx.new_n holds every row's new length (queued); `fold`: the rows marked
// PM_MX_TOUCHED are written by the fold's write pass, else they are empty.  `refused`: the word (pinned, written by what is
// queued) that says the change must not happen.  Swaps when everything has been written.
static int32_t metrics_rebuild(pm_engine* e, MxFoldArgs* fold, const uint32_t* refused, bool* swapped) {
  const uint32_t cur = e->mx.cur, nxt = cur ^ 1u, R = e->mx.R;
  *swapped = false;
  HIPCHK(e->mx.off[nxt].ensure(size_t(R) + 1));
  launch_mx_scan(e->mx.new_n.p, R, e->mx.off[nxt].p, e->mx.h_pin.p, e->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(e->stream));
  if (refused && *refused) return PM_OK;
  const uint32_t N = e->mx.h_pin.p[0];
  HIPCHK(e->mx.ser[nxt].ensure(N ? N : 1));
  HIPCHK(e->mx.val[nxt].ensure(N ? N : 1));
  if (fold) {
    fold->off_new = e->mx.off[nxt].p;
    fold->ser_new = e->mx.ser[nxt].p;
    fold->val_new = e->mx.val[nxt].p;
    launch_mx_fold(*fold, true, e->stream);
  }
  launch_mx_copy(e->mx.off[cur].p, e->mx.new_n.p, e->mx.off[nxt].p, R, e->mx.N, e->mx.ser[cur].p, e->mx.val[cur].p,
                 e->mx.ser[nxt].p, e->mx.val[nxt].p, e->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(e->stream));
  e->mx.cur = nxt;
  e->mx.N = N;
  e->mx.totals_valid = false;
  *swapped = true;
  return PM_OK;
}

// the liveness hook (status_update/mod.rs:314-343): the rows of the sweep's list (live.rows, live.n) that became Dead are
// emptied; the table is rebuilt only if one of them held anything
static int32_t metrics_clear_dead(pm_engine* e) {
  int32_t rc = metrics_prepare(e);
  if (rc) return rc;
  if (!e->mx.N || !e->live.n) return PM_OK;
  HIPCHK(e->mx.new_n.ensure(e->mx.R));
  launch_mx_lengths(e->mx.off[e->mx.cur].p, e->mx.R, e->mx.new_n.p, e->stream);
  e->mx.h_pin.p[2] = 0u;
  launch_mx_mark_dead(e->live.rows.p, e->live.n, e->mx.R, e->mx.off[e->mx.cur].p, e->mx.new_n.p, e->mx.h_pin.p + 2, e->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(e->stream));
  if (!e->mx.h_pin.p[2]) return PM_OK;
  bool swapped = false;
  return metrics_rebuild(e, nullptr, nullptr, &swapped);
}

}  // namespace pm

extern "C" {

int32_t pm_metrics_enable(pm_engine* e, uint32_t on) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  if (e->dist_phase != 0) return set_error(PM_ESTATE, "a stepwise tick is in progress");
  if (on && e->dist_world > 1) return set_error(PM_ESTATE, "the metrics ledger does not cover multi-GPU engines");
  HIPCHK(hipSetDevice(e->cfg.device));
  HIPCHK(hipStreamSynchronize(e->stream));
  metrics_release(e);
  e->mx.on = on != 0;
  if (!e->mx.on) return PM_OK;
  int32_t rc = metrics_prepare(e);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(e->stream));
  return PM_OK;
}

int32_t pm_metrics_ingest(pm_engine* e, const pm_mx_beat* beats, uint32_t n_beats, const pm_mx_entry* entries, uint32_t n_entries,
                          uint32_t n_series) {
  if (!e || (n_beats && !beats) || (n_entries && !entries)) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  int32_t rc = metrics_guard(e);
  if (rc) return rc;
  const uint32_t W = e->have_workers ? e->W : 0u;
  bool sorted = true;
  for (uint32_t b = 0; b < n_beats; ++b) {
    const pm_mx_beat& bt = beats[b];
    if (bt.kind != PM_MXB_REPLACE && bt.kind != PM_MXB_MERGE && bt.kind != PM_MXB_DELETE)
      return set_error(PM_EINVAL, "not a beat kind");
    if (uint64_t(bt.first) + bt.n > n_entries) return set_error(PM_EINVAL, "a beat's entries lie outside the entry array");
    if (bt.row != PM_MX_MANUAL) {
      if (!e->have_workers) return set_error(PM_ESTATE, "workers must be uploaded first");
      if (bt.row >= W) return set_error(PM_ERANGE, "worker index out of range");
    }
    for (uint32_t j = bt.first; j < bt.first + bt.n; ++j) {
      if (bt.kind != PM_MXB_DELETE && (entries[j].flags & ~uint32_t(PM_MXF_MAX))) return set_error(PM_EINVAL, "unknown entry flag");
      if (entries[j].series >= n_series) return set_error(PM_ERANGE, "series out of range");
    }
    if (b && uint32_t(beats[b - 1].row + 1u) > uint32_t(bt.row + 1u)) sorted = false;
  }
  if (uint64_t(e->mx.N) + n_entries >= (1ull << 31)) return set_error(PM_ENOMEM, "the metrics ledger is full");
  HIPCHK(hipSetDevice(e->cfg.device));
  if ((rc = metrics_prepare(e))) return rc;
  if (n_series > e->mx.n_series) {
    e->mx.n_series = n_series;
    e->mx.totals_valid = false;  // (the totals' arrays are longer now)
  }
  if (!n_beats) return PM_OK;
  // a row's beats side by side, in batch order (internal row = row + 1; the manual row wraps to 0)
  std::vector<pm_mx_beat>& sb = e->mx.h_beats;
  sb.assign(beats, beats + n_beats);
  if (!sorted)
    std::stable_sort(sb.begin(), sb.end(), [](const pm_mx_beat& a, const pm_mx_beat& b) { return uint32_t(a.row + 1u) < uint32_t(b.row + 1u); });
  uint32_t n_touched = 0;
  for (uint32_t b = 0; b < n_beats; ++b) n_touched += !b || sb[b].row != sb[b - 1].row;
  std::vector<uint32_t>& st = e->mx.h_stage;
  st.assign(3 * size_t(n_touched), 0u);
  for (uint32_t b = 0, k = 0; b < n_beats; ++b) {
    if (b && sb[b].row == sb[b - 1].row) {
      ++st[2 * size_t(n_touched) + k - 1];
      continue;
    }
    st[k] = sb[b].row + 1u;
    st[n_touched + k] = b;
    st[2 * size_t(n_touched) + k] = 1u;
    ++k;
  }
  HIPCHK(e->mx.beats.ensure(n_beats));
  HIPCHK(e->mx.entries.ensure(n_entries ? n_entries : 1));
  HIPCHK(e->mx.stage.ensure(st.size()));
  HIPCHK(e->mx.flag.ensure(1));
  HIPCHK(e->mx.new_n.ensure(e->mx.R));
  HIPCHK(hipMemcpyAsync(e->mx.beats.p, sb.data(), size_t(n_beats) * sizeof(pm_mx_beat), hipMemcpyHostToDevice, e->stream));
  if (n_entries)
    HIPCHK(hipMemcpyAsync(e->mx.entries.p, entries, size_t(n_entries) * sizeof(pm_mx_entry), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(e->mx.stage.p, st.data(), st.size() * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemsetAsync(e->mx.flag.p, 0, sizeof(uint32_t), e->stream));
  launch_mx_lengths(e->mx.off[e->mx.cur].p, e->mx.R, e->mx.new_n.p, e->stream);
  MxFoldArgs a{};
  a.n_touched = n_touched;
  a.t_row = e->mx.stage.p;
  a.t_first = e->mx.stage.p + n_touched;
  a.t_nb = e->mx.stage.p + 2 * size_t(n_touched);
  a.beats = e->mx.beats.p;
  a.entries = e->mx.entries.p;
  a.off_old = e->mx.off[e->mx.cur].p;
  a.ser_old = e->mx.ser[e->mx.cur].p;
  a.val_old = e->mx.val[e->mx.cur].p;
  a.new_n = e->mx.new_n.p;
  a.over = e->mx.flag.p;
  launch_mx_fold(a, false, e->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(e->mx.h_pin.p + 1, e->mx.flag.p, sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
  bool swapped = false;
  if ((rc = metrics_rebuild(e, &a, e->mx.h_pin.p + 1, &swapped))) return rc;
  if (!swapped) return set_error(PM_ERANGE, "a row would hold more than PM_MX_ROW_MAX series");
  return PM_OK;
}

int32_t pm_metrics_totals(pm_engine* e, double* sum, uint32_t* count, uint32_t cap, uint32_t* n_series) {
  if (!e || !n_series) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  int32_t rc = metrics_guard(e);
  if (rc) return rc;
  HIPCHK(hipSetDevice(e->cfg.device));
  if ((rc = metrics_prepare(e))) return rc;
  const uint32_t S = e->mx.n_series, N = e->mx.N;
  *n_series = S;
  if (S && (!sum || !count || cap < S)) return set_error(PM_ERANGE, "totals buffers too small");
  if (!S) return PM_OK;
  if (!e->mx.totals_valid) {
    e->mx.h_sum.assign(S, 0.0);
    e->mx.h_cnt.assign(S, 0u);
    if (N) {
      uint32_t passes = 1;
      while (passes < 4u && ((S - 1u) >> (8u * passes))) ++passes;
      const uint32_t chunks = (N + PM_MX_CHUNK - 1u) / PM_MX_CHUNK;
      HIPCHK(e->mx.hist.ensure(256 * size_t(chunks)));
      HIPCHK(e->mx.hist_scan.ensure(256 * size_t(chunks) + 1));
      HIPCHK(e->mx.sum.ensure(S));
      HIPCHK(e->mx.cnt.ensure(S));
      const uint32_t* ser = e->mx.ser[e->mx.cur].p;
      const double* val = e->mx.val[e->mx.cur].p;
      for (uint32_t p = 0; p < passes; ++p) {
        DevBuf<uint32_t>& ds = e->mx.sort_ser[p & 1u];
        DevBuf<double>& dv = e->mx.sort_val[p & 1u];
        HIPCHK(ds.ensure(N));
        HIPCHK(dv.ensure(N));
        launch_mx_radix_pass(ser, val, N, 8u * p, e->mx.hist.p, e->mx.hist_scan.p, ds.p, dv.p, e->stream);
        ser = ds.p, val = dv.p;
      }
      launch_mx_sums(ser, val, N, S, e->mx.sum.p, e->mx.cnt.p, e->stream);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(e->mx.h_sum.data(), e->mx.sum.p, size_t(S) * sizeof(double), hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipMemcpyAsync(e->mx.h_cnt.data(), e->mx.cnt.p, size_t(S) * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipStreamSynchronize(e->stream));
    }
    e->mx.totals_valid = true;
  }
  std::copy(e->mx.h_sum.begin(), e->mx.h_sum.end(), sum);
  std::copy(e->mx.h_cnt.begin(), e->mx.h_cnt.end(), count);
  return PM_OK;
}

int32_t pm_metrics_rows(pm_engine* e, const uint32_t* rows, uint32_t n, pm_mx_row* out, uint32_t cap, uint32_t* n_out) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  int32_t rc = metrics_guard(e);
  if (rc) return rc;
  const uint32_t W = e->have_workers ? e->W : 0u;
  for (uint32_t k = 0; rows && k < n; ++k) {
    if (rows[k] == PM_MX_MANUAL) continue;
    if (!e->have_workers) return set_error(PM_ESTATE, "workers must be uploaded first");
    if (rows[k] >= W) return set_error(PM_ERANGE, "worker index out of range");
  }
  HIPCHK(hipSetDevice(e->cfg.device));
  ABSORB_PENDING(e);  // (the groups of a tick that has not been taken in yet: pm_get_groups would report them)
  if ((rc = metrics_prepare(e))) return rc;
  MxRowsArgs a{};
  a.off = e->mx.off[e->mx.cur].p;
  a.ser = e->mx.ser[e->mx.cur].p;
  a.val = e->mx.val[e->mx.cur].p;
  if (!rows) {
    a.n = e->mx.R;
    a.total = e->mx.N;
    a.out_off = a.off;
  } else {
    if (!n) {
      if (n_out) *n_out = 0;
      return PM_OK;
    }
    std::vector<uint32_t>& st = e->mx.h_stage;
    st.resize(n);
    for (uint32_t k = 0; k < n; ++k) st[k] = rows[k] + 1u;  // (the manual row wraps to 0)
    HIPCHK(e->mx.stage.ensure(3 * size_t(n) + 1));
    uint32_t* const d_rows = e->mx.stage.p, * const d_len = d_rows + n, * const d_off = d_len + n;
    HIPCHK(hipMemcpyAsync(d_rows, st.data(), size_t(n) * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    launch_mx_row_lengths(d_rows, n, a.off, d_len, e->stream);
    launch_mx_scan(d_len, n, d_off, e->mx.h_pin.p, e->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    a.n = n;
    a.total = e->mx.h_pin.p[0];
    a.rows = d_rows;
    a.out_off = d_off;
  }
  if (n_out) *n_out = a.total;
  if (a.total && (!out || cap < a.total)) return set_error(PM_ERANGE, "metrics row buffer too small");
  if (!a.total) return PM_OK;
  // the join's other side: the host's truth, as the reports take it
  const size_t G = e->groups.size();
  e->mx.h_gid.resize(G);
  e->mx.h_gcfg.resize(G);
  for (size_t g = 0; g < G; ++g) e->mx.h_gid[g] = e->groups[g].id, e->mx.h_gcfg[g] = e->groups[g].cfg;
  if ((rc = upload(e->mx.gof, e->h_group_of.data(), size_t(W), e->stream))) return rc;
  if ((rc = upload(e->mx.gid, e->mx.h_gid.data(), G, e->stream))) return rc;
  if ((rc = upload(e->mx.gcfg, e->mx.h_gcfg.data(), G, e->stream))) return rc;
  a.group_of = e->mx.gof.p;
  a.g_id = e->mx.gid.p;
  a.g_cfg = e->mx.gcfg.p;
  HIPCHK(e->mx.out.ensure(a.total));
  a.out = e->mx.out.p;
  launch_mx_rows(a, e->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, e->mx.out.p, size_t(a.total) * sizeof(pm_mx_row), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return PM_OK;
}

}  // extern "C"
