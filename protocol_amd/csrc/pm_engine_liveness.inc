// pm_engine_liveness.inc — part of pm_engine.cpp (one translation unit; included in place): the liveness sweep: the ledger's
// buffers, their growth and initialisation (namespace pm) — and, behind them (extern "C"), C ABI:
// pm_liveness_enable / _set / _get / _sweep / _transitions (kernels in pm_liveness.inc).  Included at file scope.
//
// Unlike the change feed's buffers, where zero means "nothing", a fresh ledger row is not zero: the rows [live.W, W) are written
// by liveness_init_kernel from the HOST's flags (h_flags: the device's flags column may be behind it, and bringing it up to date
// is the tick's business — a liveness call consumes no pending delta).  pm_upload_workers(keep_groups = 0) sets live.reinit, the
// one hook in the upload path; everything else happens when the next liveness call runs liveness_prepare.  Everything is queued
// on the engine's stream; a call synchronises once before it returns (an apply sweep once more, for the rows).
namespace pm {

// a fresh ledger, and with it a fresh discovery scratch: every buffer goes back; whether liveness is on, and its threshold, stay
static void liveness_release(pm_engine* e) {
  Liveness fresh;
  fresh.on = e->live.on, fresh.m = e->live.m;
  e->live = std::move(fresh);
  e->disc = Discovery();
}

// the ledger covers [0, W): grows the two columns and initialises the rows it has not seen (queued, not waited for)
static int32_t liveness_prepare(pm_engine* e) {
  if (e->live.reinit || e->W < e->live.W) {  // (a shorter table is a new table)
    e->live.W = e->live.n = 0;
    e->live.rows_host = false;
    e->live.reinit = false;
  }
  const uint32_t W = e->W, W0 = e->live.W;
  if (W0 >= W) return PM_OK;
  HIPCHK(e->live.status.grow_keep(W, W0, e->stream));
  HIPCHK(e->live.counter.grow_keep(W, W0, e->stream));
  HIPCHK(e->live.stage.ensure(W - W0));
  HIPCHK(hipMemcpyAsync(e->live.stage.p, e->h_flags.data() + W0, size_t(W - W0) * sizeof(uint32_t), hipMemcpyHostToDevice,
                        e->stream));
  launch_liveness_init(e->live.stage.p, W0, W, e->live.status.p, e->live.counter.p, e->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(e->stream));  // (a pageable source, and the stage is reused by the call that brought us here)
  e->live.W = W;
  return PM_OK;
}

// what every liveness call but pm_liveness_enable asks first
static int32_t liveness_guard(pm_engine* e) {
  if (!e->live.on) return set_error(PM_ESTATE, "liveness is off");
  if (e->dist_phase != 0) return set_error(PM_ESTATE, "a stepwise tick is in progress");
  if (e->dist_world > 1) return set_error(PM_ESTATE, "liveness does not cover multi-GPU engines");
  if (!e->have_workers) return set_error(PM_ESTATE, "workers must be uploaded first");
  return PM_OK;
}

// the sweep behind its guard, under the engine mutex.  A row's beat: last_beat_ms[w] from the host, or — dev_beats given
// (pm_liveness_sweep_beats: a device column that covers the table) — the later of the two, or that column alone
static int32_t liveness_sweep_locked(pm_engine* e, uint64_t now_ms, const uint64_t* last_beat_ms, const uint64_t* dev_beats,
                                     const uint64_t* in_pool_bits, uint32_t apply, uint32_t* n_transitions, uint32_t* census) {
  int32_t rc;
  HIPCHK(hipSetDevice(e->cfg.device));
  if ((rc = liveness_prepare(e))) return rc;
  const uint32_t W = e->W, words = (W + 63u) / 64u;
  HIPCHK(e->live.h_count.ensure(1 + PM_NS_N, 1 + PM_NS_N));
  uint32_t* const h_count = e->live.h_count.p;
  e->live.n = 0;
  e->live.rows_host = false;
  std::memset(h_count, 0, (1 + PM_NS_N) * sizeof(uint32_t));
  if (W) {
    HIPCHK(e->live.old.ensure(W));
    HIPCHK(e->live.bitmap.ensure(words));
    HIPCHK(e->live.prefix.ensure(words));
    HIPCHK(e->live.rows.ensure(W));
    HIPCHK(e->live.census.ensure(PM_NS_N));
    HIPCHK(e->live.beat.ensure(size_t(W) + words));
    if (last_beat_ms) HIPCHK(hipMemcpyAsync(e->live.beat.p, last_beat_ms, size_t(W) * sizeof(uint64_t), hipMemcpyHostToDevice, e->stream));
    if (last_beat_ms && dev_beats) launch_ad_beat_max(dev_beats, W, e->live.beat.p, e->stream);
    if (in_pool_bits)
      HIPCHK(hipMemcpyAsync(e->live.beat.p + W, in_pool_bits, size_t(words) * sizeof(uint64_t), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemsetAsync(e->live.census.p, 0, PM_NS_N * sizeof(uint32_t), e->stream));
    LiveSweepArgs a{};
    a.W = W;
    a.m = e->live.m;
    a.now_ms = now_ms;
    a.beat = last_beat_ms ? e->live.beat.p : dev_beats;
    a.pool = in_pool_bits ? e->live.beat.p + W : nullptr;
    a.status = e->live.status.p;
    a.counter = e->live.counter.p;
    a.old_status = e->live.old.p;
    a.bitmap = e->live.bitmap.p;
    a.census = e->live.census.p;
    launch_liveness_sweep(a, e->stream);
    launch_liveness_list(e->live.bitmap.p, words, e->live.old.p, e->live.status.p, e->live.counter.p, e->live.prefix.p,
                         h_count, e->live.rows.p, e->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_count + 1, e->live.census.p, PM_NS_N * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (h_count[0] > W) return set_error(PM_ESTATE, "liveness: more listed rows than rows");
    e->live.n = h_count[0];
    // (metrics on: the rows that became Dead lose their metrics, status_update/mod.rs:314-343 — on the device, from the list)
    if (e->mx.on && e->live.n && (rc = metrics_clear_dead(e))) return rc;
  }
  if (n_transitions) *n_transitions = e->live.n;
  if (census) std::copy(h_count + 1, h_count + 1 + PM_NS_N, census);
  if (!apply || !e->live.n) return PM_OK;
  // the list in list order through pm_on_worker_status_many's body (status_update_impl.rs:8-39 behind mod.rs:360-368), still
  // under the engine mutex: nothing can come between the sweep and what it applies
  const uint32_t n = e->live.n;
  e->live.h_rows.resize(n);
  HIPCHK(hipMemcpyAsync(e->live.h_rows.data(), e->live.rows.p, size_t(n) * sizeof(pm_live_row), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  e->live.rows_host = true;
  std::vector<uint32_t> col(3 * size_t(n));
  uint32_t* const workers = col.data(), * const flags_new = workers + n, * const dead = flags_new + n;
  for (uint32_t k = 0; k < n; ++k) {
    const pm_live_row& r = e->live.h_rows[k];
    if (r.worker >= W) return set_error(PM_ESTATE, "liveness: a listed row the table does not hold");
    workers[k] = r.worker;
    flags_new[k] = r.new_status == PM_NS_HEALTHY ? (e->h_flags[r.worker] | PM_W_HEALTHY) : (e->h_flags[r.worker] & ~uint32_t(PM_W_HEALTHY));
    dead[k] = r.new_status == PM_NS_DEAD ? 1u : 0u;
  }
  return worker_status_many_locked(e, workers, flags_new, dead, n);
}

}  // namespace pm

extern "C" {

int32_t pm_liveness_enable(pm_engine* e, uint32_t on, uint32_t missing_heartbeat_threshold) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  if (e->dist_phase != 0) return set_error(PM_ESTATE, "a stepwise tick is in progress");
  if (on && e->dist_world > 1) return set_error(PM_ESTATE, "liveness does not cover multi-GPU engines");
  HIPCHK(hipSetDevice(e->cfg.device));
  HIPCHK(hipStreamSynchronize(e->stream));
  liveness_release(e);
  e->live.on = on != 0;
  e->live.m = missing_heartbeat_threshold;
  if (!e->live.on || !e->have_workers) return PM_OK;  // (no table yet: the first call behind an upload initialises)
  return liveness_prepare(e);
}

int32_t pm_liveness_set(pm_engine* e, const uint32_t* idx, const uint8_t* status, const uint32_t* counter, uint32_t n) {
  if (!e || (n && (!idx || !status))) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  int32_t rc = liveness_guard(e);
  if (rc) return rc;
  for (uint32_t k = 0; k < n; ++k)
    if (idx[k] >= e->W) return set_error(PM_ERANGE, "worker index out of range");
  for (uint32_t k = 0; k < n; ++k)
    if (status[k] >= PM_NS_N) return set_error(PM_EINVAL, "not a node status");
  HIPCHK(hipSetDevice(e->cfg.device));
  if ((rc = liveness_prepare(e))) return rc;
  if (!n) return PM_OK;
  // an index given twice takes its last entry: the kernel's rows must be distinct
  std::vector<uint32_t> order(n);
  for (uint32_t k = 0; k < n; ++k) order[k] = k;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return idx[a] < idx[b]; });
  uint32_t u = 0;
  for (uint32_t k = 0; k < n; ++k)
    if (k + 1 == n || idx[order[k + 1]] != idx[order[k]]) order[u++] = order[k];
  std::vector<uint32_t>& st = e->live.h_stage;
  st.assign(2 * size_t(u) + (u + 3) / 4, 0u);
  uint8_t* const bytes = reinterpret_cast<uint8_t*>(st.data() + 2 * size_t(u));
  for (uint32_t k = 0; k < u; ++k) {
    st[k] = idx[order[k]];
    st[u + k] = counter ? counter[order[k]] : 0u;
    bytes[k] = status[order[k]];
  }
  HIPCHK(e->live.stage.ensure(st.size()));
  HIPCHK(hipMemcpyAsync(e->live.stage.p, st.data(), st.size() * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
  launch_liveness_set(e->live.stage.p, u, e->live.status.p, e->live.counter.p, e->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(e->stream));
  return PM_OK;
}

int32_t pm_liveness_get(pm_engine* e, const uint32_t* idx, uint32_t n, uint8_t* status, uint32_t* counter) {
  if (!e || (n && !idx)) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  int32_t rc = liveness_guard(e);
  if (rc) return rc;
  for (uint32_t k = 0; k < n; ++k)
    if (idx[k] >= e->W) return set_error(PM_ERANGE, "worker index out of range");
  HIPCHK(hipSetDevice(e->cfg.device));
  if ((rc = liveness_prepare(e))) return rc;
  if (!n) return PM_OK;
  const size_t out_words = size_t(n) + (n + 3) / 4;
  HIPCHK(e->live.stage.ensure(size_t(n) + out_words));
  std::vector<uint32_t>& st = e->live.h_stage;
  st.assign(out_words, 0u);
  HIPCHK(hipMemcpyAsync(e->live.stage.p, idx, size_t(n) * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
  launch_liveness_get(e->live.stage.p, n, e->live.status.p, e->live.counter.p, e->live.stage.p + n, e->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(st.data(), e->live.stage.p + n, out_words * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  if (counter) std::copy(st.begin(), st.begin() + n, counter);
  if (status) std::memcpy(status, st.data() + n, n);
  return PM_OK;
}

int32_t pm_liveness_sweep(pm_engine* e, uint64_t now_ms, const uint64_t* last_beat_ms, const uint64_t* in_pool_bits,
                          uint32_t apply, uint32_t* n_transitions, uint32_t* census) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  int32_t rc = liveness_guard(e);
  if (rc) return rc;
  if (e->W && !last_beat_ms) return set_error(PM_EINVAL, "null beat column");
  return liveness_sweep_locked(e, now_ms, last_beat_ms, nullptr, in_pool_bits, apply, n_transitions, census);
}

int32_t pm_liveness_transitions(pm_engine* e, pm_live_row* rows, uint32_t cap, uint32_t* n) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  int32_t rc = liveness_guard(e);
  if (rc) return rc;
  const uint32_t have = e->live.reinit ? 0u : e->live.n;  // (a replaced table: the list named rows that are gone)
  if (n) *n = have;
  if (!rows || cap < have) return set_error(PM_ERANGE, "transition row buffer too small");
  if (!have) return PM_OK;
  if (e->live.rows_host) {
    std::copy(e->live.h_rows.begin(), e->live.h_rows.begin() + have, rows);
    return PM_OK;
  }
  HIPCHK(hipSetDevice(e->cfg.device));
  HIPCHK(hipMemcpyAsync(rows, e->live.rows.p, size_t(have) * sizeof(pm_live_row), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return PM_OK;
}

}  // extern "C"
