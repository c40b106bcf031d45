// pm_engine_admission.inc — part of pm_engine.cpp (one translation unit; included in place, behind pm_engine_gate.inc, whose
// check and queue steps it calls): the request gate's admission ledger: the rate windows and the beat column by worker row, the
// standing nonce set (namespace pm) — and, behind them (extern "C"), C ABI: pm_admission_enable, pm_admit_requests,
// pm_admission_rate_get / _set, pm_admission_nonces, pm_beats_get / _set, pm_liveness_sweep_beats (kernels in pm_admission.inc).
// Included at file scope.
//
// The two row ledgers follow the liveness ledger's rules: rows [ad.W, W) are zeroed by the next admission call, and
// pm_upload_workers(keep_groups = 0) sets ad.reinit, the one hook in the upload path.  The nonce set is tied to no row and is
// touched by pm_admit_requests and pm_admission_enable alone.  pm_admit_requests checks everything it can refuse and makes
// all its room before the first kernel that writes a ledger is queued: a failing call changes no ledger.  Everything is queued
// on the engine's stream; a call synchronises once before it returns.
namespace pm {

// fresh ledgers: every buffer goes back; whether admission is on, and the key's width, stay
static void admission_release(pm_engine* e) {
  Admission fresh;
  fresh.on = e->ad.on, fresh.kbits = e->ad.kbits;
  e->ad = std::move(fresh);
}

// the row ledgers cover [0, W): grown, and the rows they have not seen zeroed (queued, not waited for)
static int32_t admission_prepare(pm_engine* e) {
  Admission& ad = e->ad;
  if (ad.reinit || e->W < ad.W) ad.W = 0;  // (a shorter table is a new table)
  ad.reinit = false;
  const uint32_t W = e->W, W0 = ad.W;
  if (W0 >= W) return PM_OK;
  HIPCHK(ad.win.grow_keep(W, W0, e->stream));
  HIPCHK(ad.cnt.grow_keep(W, W0, e->stream));
  HIPCHK(ad.beat.grow_keep(W, W0, e->stream));
  HIPCHK(hipMemsetAsync(ad.win.p + W0, 0, size_t(W - W0) * sizeof(uint64_t), e->stream));
  HIPCHK(hipMemsetAsync(ad.cnt.p + W0, 0, size_t(W - W0) * sizeof(uint32_t), e->stream));
  HIPCHK(hipMemsetAsync(ad.beat.p + W0, 0, size_t(W - W0) * sizeof(uint64_t), e->stream));
  ad.W = W;
  return PM_OK;
}

// what every admission call but pm_admission_enable asks first
static int32_t admission_guard(pm_engine* e) {
  if (!e->ad.on) return set_error(PM_ESTATE, "admission is off");
  return addresses_guard(e);
}

// idx[0, n) name rows of the table
static int32_t admission_rows_ok(pm_engine* e, const uint32_t* idx, uint32_t n) {
  for (uint32_t k = 0; k < n; ++k)
    if (idx[k] >= e->W) return set_error(PM_ERANGE, "worker index out of range");
  return PM_OK;
}

// rows idx[0, n) of a 64-bit column and, where there is one, of its 32-bit companion, to the host
static int32_t admission_get(pm_engine* e, const uint32_t* idx, uint32_t n, const uint64_t* col64, const uint32_t* col32, uint64_t* out64,
                             uint32_t* out32) {
  Admission& ad = e->ad;
  HIPCHK(ad.idx.ensure(n));
  HIPCHK(ad.io64.ensure(n));
  HIPCHK(ad.io32.ensure(n));
  HIPCHK(hipMemcpyAsync(ad.idx.p, idx, size_t(n) * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
  launch_ad_gather(ad.idx.p, n, col64, out32 ? col32 : nullptr, ad.io64.p, ad.io32.p, e->stream);
  HIPCHK(hipGetLastError());
  if (out64) HIPCHK(hipMemcpyAsync(out64, ad.io64.p, size_t(n) * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
  if (out32) HIPCHK(hipMemcpyAsync(out32, ad.io32.p, size_t(n) * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return PM_OK;
}

// the reverse; an index given twice takes its last entry (the kernel's rows must be distinct)
static int32_t admission_set(pm_engine* e, const uint32_t* idx, uint32_t n, const uint64_t* in64, const uint32_t* in32, uint64_t* col64,
                             uint32_t* col32) {
  Admission& ad = e->ad;
  std::vector<uint32_t> order(n);
  for (uint32_t k = 0; k < n; ++k) order[k] = k;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return idx[a] < idx[b]; });
  uint32_t u = 0;
  for (uint32_t k = 0; k < n; ++k)
    if (k + 1 == n || idx[order[k + 1]] != idx[order[k]]) order[u++] = order[k];
  std::vector<uint32_t> h_idx(u), h32(u);
  std::vector<uint64_t> h64(u);
  for (uint32_t k = 0; k < u; ++k) h_idx[k] = idx[order[k]], h64[k] = in64[order[k]], h32[k] = in32 ? in32[order[k]] : 0u;
  HIPCHK(ad.idx.ensure(u));
  HIPCHK(ad.io64.ensure(u));
  HIPCHK(ad.io32.ensure(u));
  HIPCHK(hipMemcpyAsync(ad.idx.p, h_idx.data(), size_t(u) * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(ad.io64.p, h64.data(), size_t(u) * sizeof(uint64_t), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(ad.io32.p, h32.data(), size_t(u) * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
  launch_ad_scatter(ad.idx.p, u, e->W, ad.io64.p, ad.io32.p, col64, in32 ? col32 : nullptr, e->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(e->stream));  // (the staging vectors go when this returns)
  return PM_OK;
}

}  // namespace pm

extern "C" {

int32_t pm_admission_enable(pm_engine* e, uint32_t on) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  if (e->dist_phase != 0) return set_error(PM_ESTATE, "a stepwise tick is in progress");
  const uint32_t kbits = (on >> 8) & 0xFFu;  // (pm_engine_debug.h: PM_AD_DEBUG_PREFIX_BITS)
  if (on && kbits > 64u) return set_error(PM_EINVAL, "a key has at most 64 bits");
  if (on && !e->ab.on) return set_error(PM_ESTATE, "the address book is off");
  HIPCHK(hipSetDevice(e->cfg.device));
  HIPCHK(hipStreamSynchronize(e->stream));
  admission_release(e);
  e->ad.on = on != 0;
  e->ad.kbits = kbits ? kbits : 64u;
  return PM_OK;
}

int32_t pm_admit_requests(pm_engine* e, uint64_t now_ms, const uint8_t* bytes, const uint32_t* offsets, const uint8_t* sig65,
                          const uint8_t* claimed20, const uint8_t* flags, const uint64_t* timestamp_s, const uint8_t* nonce_bytes,
                          const uint32_t* nonce_offsets, uint32_t n, pm_rq_verdict* out, uint32_t* counts) {
  if (!e || (n && (!offsets || !sig65 || !claimed20 || !out || !counts))) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  int32_t rc = admission_guard(e);
  if (rc) return rc;
  if (!n) return PM_OK;
  if ((rc = gate_check(bytes, offsets, n))) return rc;
  bool all_no_ts = flags != nullptr, all_no_nonce = flags != nullptr;
  for (uint32_t i = 0; i < n && flags; ++i) {
    all_no_ts = all_no_ts && (flags[i] & PM_RQ_FLAG_NO_TIMESTAMP);
    all_no_nonce = all_no_nonce && (flags[i] & PM_RQ_FLAG_NO_NONCE);
  }
  if (!timestamp_s && !all_no_ts) return set_error(PM_EINVAL, "null timestamps");
  if (!nonce_offsets && !all_no_nonce) return set_error(PM_EINVAL, "null nonces");
  uint32_t nonce_total = 0;
  if (nonce_offsets) {
    for (uint32_t i = 0; i < n; ++i)
      if (nonce_offsets[i + 1] < nonce_offsets[i]) return set_error(PM_EINVAL, "the nonce offsets must not descend");
    nonce_total = nonce_offsets[n];
    if (nonce_total && !nonce_bytes) return set_error(PM_EINVAL, "null nonces");
    if (nonce_total > 0xFFFFFF00u) return set_error(PM_ERANGE, "too many nonce bytes in one call");
  }
  Admission& ad = e->ad;
  if (uint64_t(ad.N) + n > 0x7FFFFFFFull) return set_error(PM_ERANGE, "the nonce set is full");
  HIPCHK(hipSetDevice(e->cfg.device));
  // room first: nothing below this block can fail but the runtime itself
  const uint32_t N = ad.N, cap = N + n, nxt = ad.cur ^ 1u;
  HIPCHK(ad.sort.ensure(n));
  HIPCHK(ad.text.ensure(size_t(nonce_total) + 8));  // (keccak reads whole aligned words)
  HIPCHK(ad.off.ensure(size_t(n) + 1));
  HIPCHK(ad.ndig.ensure(4 * size_t(n)));
  HIPCHK(ad.ts.ensure(n));
  HIPCHK(ad.stage.ensure(n));
  HIPCHK(ad.replay.ensure(n));
  HIPCHK(ad.keep_new.ensure(n));
  HIPCHK(ad.rank_new.ensure(size_t(n) + 1));
  HIPCHK(ad.keep_old.ensure(N ? N : 1));
  HIPCHK(ad.rank_old.ensure(size_t(N) + 1));
  HIPCHK(ad.counts.ensure(PM_AD_N_CODES));
  HIPCHK(ad.dig[nxt].ensure(4 * size_t(cap)));
  HIPCHK(ad.ms[nxt].ensure(cap));
  HIPCHK(ad.dig[ad.cur].ensure(1));  // (an empty set still has an address)
  HIPCHK(ad.ms[ad.cur].ensure(1));
  HIPCHK(ad.h_pin.ensure(2, 2));
  if ((rc = admission_prepare(e))) return rc;
  if ((rc = gate_queue(e, bytes, offsets, sig65, claimed20, flags, n))) return rc;
  Gate& g = e->gate;
  const uint32_t W = e->W;
  const uint8_t* d_flags = flags ? g.flags.p : nullptr;
  if (timestamp_s) HIPCHK(hipMemcpyAsync(ad.ts.p, timestamp_s, size_t(n) * sizeof(uint64_t), hipMemcpyHostToDevice, e->stream));
  if (nonce_offsets) {
    if (nonce_total) HIPCHK(hipMemcpyAsync(ad.text.p, nonce_bytes, nonce_total, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(ad.off.p, nonce_offsets, (size_t(n) + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
  } else {
    HIPCHK(hipMemsetAsync(ad.off.p, 0, (size_t(n) + 1) * sizeof(uint32_t), e->stream));  // (n empty nonces: none is looked at)
  }
  HIPCHK(hipMemsetAsync(ad.counts.p, 0, PM_AD_N_CODES * sizeof(uint32_t), e->stream));
  launch_keccak_many(ad.text.p, ad.off.p, n, ad.ndig.p, e->stream);
  // the rate limit, the age and the format, by row in batch order; then the heads write the windows
  AdRateArgs ra{};
  ra.n = n, ra.W = W, ra.now_ms = now_ms;
  ra.win = ad.win.p, ra.cnt = ad.cnt.p;
  ra.flags = d_flags, ra.ts = timestamp_s ? ad.ts.p : nullptr;
  ra.nonce = ad.text.p, ra.noff = nonce_offsets ? ad.off.p : nullptr;
  ra.stage = ad.stage.p;
  const uint32_t by_row = launch_ad_rate(ra, g.out.p, ad.sort.bufs(), e->stream);
  launch_ad_rate_commit(ad.sort.key[by_row].p, n, W, now_ms, ad.win.p, ad.cnt.p, e->stream);
  // the nonce set: the batch by key, the replays, what is kept on both sides, the merge into the other buffer
  AdNonceArgs na{};
  na.n = n, na.N = N, na.kbits = ad.kbits, na.now_ms = now_ms;
  na.stage = ad.stage.p, na.dig = ad.ndig.p;
  na.old_dig = ad.dig[ad.cur].p, na.old_ms = ad.ms[ad.cur].p;
  na.replay = ad.replay.p, na.keep_new = ad.keep_new.p;
  const uint32_t by_key = launch_ad_nonces(na, ad.sort.bufs(), ad.keep_old.p, e->stream);
  launch_mx_scan(ad.keep_new.p, n, ad.rank_new.p, ad.h_pin.p, e->stream);
  launch_mx_scan(ad.keep_old.p, N, ad.rank_old.p, ad.h_pin.p + 1, e->stream);
  AdMergeArgs ma{};
  ma.key = ad.sort.key[by_key].p, ma.val = ad.sort.val[by_key].p;
  ma.n = n, ma.N = N, ma.kbits = ad.kbits, ma.cap = cap, ma.now_ms = now_ms;
  ma.dig = ad.ndig.p, ma.keep_new = ad.keep_new.p, ma.rank_new = ad.rank_new.p;
  ma.old_dig = ad.dig[ad.cur].p, ma.old_ms = ad.ms[ad.cur].p, ma.keep_old = ad.keep_old.p, ma.rank_old = ad.rank_old.p;
  ma.out_dig = ad.dig[nxt].p, ma.out_ms = ad.ms[nxt].p;
  launch_ad_merge(ma, e->stream);
  launch_ad_final(g.out.p, n, W, ad.stage.p, ad.replay.p, d_flags, now_ms, ad.beat.p, ad.counts.p, e->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, g.out.p, sizeof(pm_rq_verdict) * size_t(n), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(counts, ad.counts.p, PM_AD_N_CODES * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  if (uint64_t(ad.h_pin.p[0]) + ad.h_pin.p[1] > cap) return set_error(PM_ESTATE, "admission: more nonces kept than there are");
  ad.N = ad.h_pin.p[0] + ad.h_pin.p[1];
  ad.cur = nxt;
  return PM_OK;
}

int32_t pm_admission_rate_get(pm_engine* e, const uint32_t* idx, uint32_t n, uint64_t* window_start_ms, uint32_t* count) {
  if (!e || (n && !idx)) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  int32_t rc = admission_guard(e);
  if (rc) return rc;
  if ((rc = admission_rows_ok(e, idx, n))) return rc;
  HIPCHK(hipSetDevice(e->cfg.device));
  if ((rc = admission_prepare(e))) return rc;
  if (!n) return PM_OK;
  return admission_get(e, idx, n, e->ad.win.p, e->ad.cnt.p, window_start_ms, count);
}

int32_t pm_admission_rate_set(pm_engine* e, const uint32_t* idx, const uint64_t* window_start_ms, const uint32_t* count, uint32_t n) {
  if (!e || (n && (!idx || !window_start_ms || !count))) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  int32_t rc = admission_guard(e);
  if (rc) return rc;
  if ((rc = admission_rows_ok(e, idx, n))) return rc;
  HIPCHK(hipSetDevice(e->cfg.device));
  if ((rc = admission_prepare(e))) return rc;
  if (!n) return PM_OK;
  return admission_set(e, idx, n, window_start_ms, count, e->ad.win.p, e->ad.cnt.p);
}

int32_t pm_admission_nonces(pm_engine* e, uint64_t now_ms, uint32_t* n_live, uint32_t* n_held) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  int32_t rc = admission_guard(e);
  if (rc) return rc;
  Admission& ad = e->ad;
  if (n_held) *n_held = ad.N;
  if (n_live) *n_live = 0;
  if (!ad.N || !n_live) return PM_OK;
  HIPCHK(hipSetDevice(e->cfg.device));
  HIPCHK(ad.keep_old.ensure(ad.N));
  HIPCHK(ad.rank_old.ensure(size_t(ad.N) + 1));
  HIPCHK(ad.h_pin.ensure(2, 2));
  launch_ad_old_live(ad.ms[ad.cur].p, ad.N, now_ms, ad.keep_old.p, e->stream);
  launch_mx_scan(ad.keep_old.p, ad.N, ad.rank_old.p, ad.h_pin.p, e->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(e->stream));
  *n_live = ad.h_pin.p[0];
  return PM_OK;
}

int32_t pm_beats_get(pm_engine* e, const uint32_t* idx, uint32_t n, uint64_t* last_beat_ms) {
  if (!e || (n && (!idx || !last_beat_ms))) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  int32_t rc = admission_guard(e);
  if (rc) return rc;
  if ((rc = admission_rows_ok(e, idx, n))) return rc;
  HIPCHK(hipSetDevice(e->cfg.device));
  if ((rc = admission_prepare(e))) return rc;
  if (!n) return PM_OK;
  return admission_get(e, idx, n, e->ad.beat.p, nullptr, last_beat_ms, nullptr);
}

int32_t pm_beats_set(pm_engine* e, const uint32_t* idx, const uint64_t* last_beat_ms, uint32_t n) {
  if (!e || (n && (!idx || !last_beat_ms))) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  int32_t rc = admission_guard(e);
  if (rc) return rc;
  if ((rc = admission_rows_ok(e, idx, n))) return rc;
  HIPCHK(hipSetDevice(e->cfg.device));
  if ((rc = admission_prepare(e))) return rc;
  if (!n) return PM_OK;
  return admission_set(e, idx, n, last_beat_ms, nullptr, e->ad.beat.p, nullptr);
}

int32_t pm_liveness_sweep_beats(pm_engine* e, uint64_t now_ms, const uint64_t* last_beat_ms, const uint64_t* in_pool_bits,
                                uint32_t apply, uint32_t* n_transitions, uint32_t* census) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  if (!e->ad.on) return set_error(PM_ESTATE, "admission is off");
  int32_t rc = liveness_guard(e);
  if (rc) return rc;
  HIPCHK(hipSetDevice(e->cfg.device));
  if ((rc = admission_prepare(e))) return rc;
  HIPCHK(e->ad.beat.ensure(1));  // (an empty table still has an address)
  return liveness_sweep_locked(e, now_ms, last_beat_ms, e->ad.beat.p, in_pool_bits, apply, n_transitions, census);
}

}  // extern "C"
