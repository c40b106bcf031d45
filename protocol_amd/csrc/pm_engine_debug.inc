// pm_engine_debug.inc — part of pm_engine.cpp (one translation unit; included in place): C ABI: test and measuring hooks of include/pm_engine_debug.h (inside extern "C").
// debug (include/pm_engine_debug.h): counters of the last carve and of the engine's incremental state; copies min(cap, 100) words
int32_t pm_debug_carve_prof(pm_engine* e, unsigned long long* out, uint32_t cap) {
  if (!e || !out) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  const uint32_t n = std::min<uint32_t>(cap, 32u);
  std::memcpy(out, e->carve_prof, size_t(n) * sizeof(unsigned long long));
  for (uint32_t k = 32; k < cap && k < 56; ++k) out[k] = e->carve_why[k - 32];
  for (uint32_t k = 56; k < cap && k < 88; ++k) out[k] = e->carve_prof[k - 56 + 32];  // (phase counters 32..47)  // (how the validation launches ended; the index)
  // (the incremental state a long-running engine keeps: the task index space, the group list, the snapshot buffers)
  const unsigned long long inc[9] = {e->t_lo, e->t_cap, e->T, e->t_dead, e->t_regrowths, e->t_compactions,
                                     e->groups.size(), e->n_dead_groups, e->pub_retired.size()};
  for (uint32_t k = 88; k < cap && k < 97; ++k) out[k] = inc[k - 88];
  if (cap > 97u) out[97] = e->carve_why[24];  // (the last carve's again: times the streaming carve dropped a configuration's tickets and issued them afresh)
  if (cap > 98u) out[98] = e->ab.shallow;  // (the address book's ranks by sort path, since creation)
  if (cap > 99u) out[99] = e->ab.deep;
  return PM_OK;
}

// debug (PM_CARVE_PROF builds): the timeline of the last streaming carve launch — up to cap events of two u64 each
// {s_memtime, type | a << 8 | b << 32}; *n = events recorded
int32_t pm_debug_stream_trace(pm_engine* e, unsigned long long* out, uint32_t cap, uint32_t* n) {
  if (!e || !out || !n) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  *n = 0;
  if (!e->d_stream_trace.p || !e->d_stream_ctl.p) return PM_OK;
  uint32_t cnt = 0;
  HIPCHK(hipMemcpy(&cnt, e->d_stream_ctl.p + SC_TRACE, 4, hipMemcpyDeviceToHost));
#ifdef PM_ROW_REC  // (the validator's events live in the second half of the buffer there)
  cnt = std::min<uint32_t>(cnt, std::min<uint32_t>(cap, PM_STREAM_TRACE_CAP / 8u));
  if (cnt) HIPCHK(hipMemcpy(out, e->d_stream_trace.p + PM_STREAM_TRACE_CAP, size_t(cnt) * 16, hipMemcpyDeviceToHost));
#else
  cnt = std::min<uint32_t>(cnt, std::min<uint32_t>(cap, PM_STREAM_TRACE_CAP));
  if (cnt) HIPCHK(hipMemcpy(out, e->d_stream_trace.p, size_t(cnt) * 16, hipMemcpyDeviceToHost));
#endif
  *n = cnt;
  return PM_OK;
}

// debug (include/pm_engine_debug.h): candidate lists longer than `n` slots take the all-in-HBM carve path (carve_step_mem), which
// otherwise needs more than 262,144 candidates for one configuration; 0 = off
// debug (PM_ROW_REC builds, tools/row_rec.py): the time stamps the row makers of the last streaming launch left, eight words
// per ticket (see stream_proposer); 0 rows from any other build
int32_t pm_debug_row_records(pm_engine* e, unsigned long long* out, uint32_t cap_rows, uint32_t* n_rows) {
  if (!e || !out || !n_rows) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  *n_rows = 0;
#ifdef PM_ROW_REC
  if (!e->d_stream_trace.p) return PM_OK;
  const uint32_t n = std::min<uint32_t>(cap_rows, PM_STREAM_TRACE_CAP / 8u);
  HIPCHK(hipMemcpy(out, e->d_stream_trace.p, size_t(n) * 64, hipMemcpyDeviceToHost));
  *n_rows = n;
#endif
  return PM_OK;
}
// debug (PM_ROW_REC builds, tools/pipeline_probe.py): the batches of steps the chain of the last streaming launch took up, four
// words each {clock at the loop's top, first entry | entries << 24 | live ones << 32 | commits so far << 40, clock when the entries
// had been looked at, clock behind the steps}; 0 from any other build
int32_t pm_debug_chain_batches(pm_engine* e, unsigned long long* out, uint32_t cap, uint32_t* n) {
  if (!e || !out || !n) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  *n = 0;
#ifdef PM_ROW_REC
  if (!e->d_stream_trace.p || !e->d_stream_ctl.p) return PM_OK;
  uint32_t cnt = 0;
  HIPCHK(hipMemcpy(&cnt, e->d_stream_ctl.p + SC_BATCHES, 4, hipMemcpyDeviceToHost));
  cnt = std::min<uint32_t>(cnt, std::min<uint32_t>(cap, PM_STREAM_TRACE_CAP / 8u));
  if (cnt) HIPCHK(hipMemcpy(out, e->d_stream_trace.p + PM_STREAM_TRACE_CAP + PM_STREAM_TRACE_CAP / 2u, size_t(cnt) * 32, hipMemcpyDeviceToHost));
  *n = cnt;
#endif
  return PM_OK;
}
// ... and the parkers' blocks: eight words each, indexed by the block's first ticket / 16 (see stream_park); cap_blocks <= 4096
int32_t pm_debug_park_records(pm_engine* e, unsigned long long* out, uint32_t cap_blocks, uint32_t* n_blocks) {
  if (!e || !out || !n_blocks) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  *n_blocks = 0;
#ifdef PM_ROW_REC
  if (!e->d_stream_trace.p) return PM_OK;
  const uint32_t n = std::min<uint32_t>(cap_blocks, PM_STREAM_TRACE_CAP / 32u);
  HIPCHK(hipMemcpy(out, e->d_stream_trace.p + PM_STREAM_TRACE_CAP + PM_STREAM_TRACE_CAP / 4u, size_t(n) * 64, hipMemcpyDeviceToHost));
  *n_blocks = n;
#endif
  return PM_OK;
}
int32_t pm_debug_mem_lists_above(pm_engine* e, uint32_t n) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  e->debug_mem_above = n;
  return PM_OK;
}

// debug (include/pm_engine_debug.h): the streaming carve's chain gives its launch up (CARVE_STATE_ABORTED, as a lost
// hand-shake inside the validator would) once n steps of the carve are committed; the engine continues on the batch
// pipeline from there (form_poll).  0 = off
int32_t pm_debug_stream_abort_after(pm_engine* e, uint32_t n) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  e->debug_abort_after = n;
  return PM_OK;
}

// debug (include/pm_engine_debug.h): merge configurations (pm_merge_solo_groups, pm_tick) whose selections went through the
// streaming carve since the engine was created
int32_t pm_debug_merge_streamed(pm_engine* e, uint32_t* n) {
  if (!e || !n) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  *n = e->merge_streamed;
  return PM_OK;
}

// debug (include/pm_engine_debug.h): times the device's group state was brought up to date by a delta (dissolved groups'
// workers + new rows) instead of the whole list, since the engine was created
int32_t pm_debug_delta_pushes(pm_engine* e, uint32_t* n) {
  if (!e || !n) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  *n = e->delta_pushes;
  return PM_OK;
}

// debug (include/pm_engine_debug.h): which way the last per-task call (pm_match_per_task, pm_match_per_task_device) took —
// the distinct valid masks it counted (0: fewer than 200,000 rows, 64 configurations or sweep_variant 1: it did not count)
// and whether it swept once per distinct mask
int32_t pm_debug_per_task_path(pm_engine* e, uint32_t* distinct_masks, uint32_t* interned) {
  if (!e || !distinct_masks || !interned) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  *distinct_masks = e->pt_distinct;
  *interned = e->pt_interned ? 1u : 0u;
  return PM_OK;
}

// debug (include/pm_engine_debug.h): when the proposer walks the spatial index instead of sweeping the whole candidate list —
// 0 never, 1 when it pays (default), 2 whenever the carve has one (built for any swarm of 64+ positions),
// 3 = 2 with every seed sent through the whole-list fallback
int32_t pm_debug_prune_mode(pm_engine* e, uint32_t mode) {
  if (!e || mode > 3u) return set_error(PM_EINVAL, "prune mode 0..3");
  std::lock_guard<std::mutex> lk(e->mu);
  e->prune_mode = mode;
  return PM_OK;
}

#ifdef PM_BATCH_LOG
extern "C" int32_t pm_debug_batch_log(pm_engine* e, uint32_t* out, uint32_t cap_words, uint32_t* n_words) {
  if (!e || !out || !n_words) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  *n_words = uint32_t(e->blog.size());
  std::memcpy(out, e->blog.data(), sizeof(uint32_t) * std::min<size_t>(cap_words, e->blog.size()));
  return PM_OK;
}
#endif

// debug (include/pm_engine_debug.h): stream triad over 3 x n_doubles f64 on the engine's stream, best of `reps` -> GB/s
int32_t pm_debug_hbm_triad(pm_engine* e, uint64_t n_doubles, uint32_t reps, double* gb_per_s) {
  if (!e || !gb_per_s || !n_doubles) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(hipSetDevice(e->cfg.device));
  DevBuf<double> d_a, d_b, d_c;  // (freed on every way out)
  HIPCHK(d_a.ensure(n_doubles));
  if (d_b.ensure(n_doubles) != hipSuccess || d_c.ensure(n_doubles) != hipSuccess) return set_error(PM_ENOMEM, "triad buffers");
  double *const a = d_a.p, *const b = d_b.p, *const c = d_c.p;
  (void)hipMemsetAsync(b, 0, n_doubles * 8, e->stream);
  (void)hipMemsetAsync(c, 0, n_doubles * 8, e->stream);
  float best = 1e30f;
  for (uint32_t r = 0; r < reps + 1; ++r) {
    (void)hipEventRecord(e->kev[0], e->stream);
    launch_triad(b, c, a, size_t(n_doubles), e->stream);
    (void)hipEventRecord(e->kev[1], e->stream);
    (void)hipEventSynchronize(e->kev[1]);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e->kev[0], e->kev[1]);
    if (r > 0 && ms < best) best = ms;
  }
  *gb_per_s = double(n_doubles) * 24.0 / (double(best) * 1e-3) / 1e9;
  return PM_OK;
}

// debug (include/pm_engine_debug.h): rows built by the insertion and by the networks from the same keys, compared on the
// device (mismatches[0]: 1 = a register differs, 2 = a threshold, 4 = what a tracker answers; [1] = rows that differ); the
// networks' rows come back for the caller's own sort
int32_t pm_debug_row_networks(pm_engine* e, const uint64_t* keys, const uint32_t* sites, uint32_t n_waves, uint32_t n_per_wave,
                              uint32_t slot_bits, uint64_t ulps, uint32_t upto, uint64_t* rows_out, uint32_t* mismatches) {
  if (!e || !keys || !sites || !rows_out || !mismatches || !n_waves || (n_waves & 3u) || !n_per_wave || slot_bits == 0 || slot_bits > 24)
    return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(hipSetDevice(e->cfg.device));
  const size_t nk = size_t(n_waves) * n_per_wave, ns = size_t(1) << slot_bits;
  DevBuf<uint64_t> d_k, d_rows;
  DevBuf<uint32_t> d_s, d_m;
  if (d_k.ensure(nk) != hipSuccess || d_rows.ensure(size_t(n_waves) * 64) != hipSuccess || d_s.ensure(ns) != hipSuccess ||
      d_m.ensure(2) != hipSuccess)
    return set_error(PM_ENOMEM, "row network test buffers");
  (void)hipMemcpyAsync(d_k.p, keys, nk * 8, hipMemcpyHostToDevice, e->stream);
  (void)hipMemcpyAsync(d_s.p, sites, ns * 4, hipMemcpyHostToDevice, e->stream);
  (void)hipMemsetAsync(d_m.p, 0, 8, e->stream);
  launch_row_network_test(d_k.p, d_s.p, n_waves, n_per_wave, slot_bits, ulps, upto, d_rows.p, d_m.p, e->stream);
  (void)hipMemcpyAsync(rows_out, d_rows.p, size_t(n_waves) * 64 * 8, hipMemcpyDeviceToHost, e->stream);
  (void)hipMemcpyAsync(mismatches, d_m.p, 8, hipMemcpyDeviceToHost, e->stream);
  if (hipStreamSynchronize(e->stream) != hipSuccess) return set_error(PM_ENODEV, "row network test");
  return PM_OK;
}

// debug (include/pm_engine_debug.h): the same kernel with a third row through the networks' inline copy, and everything the three
// rows hold and near_row_finish says about them at every K, for the caller's own reference (tests/test_gpu_row_certificates.py)
int32_t pm_debug_row_certificates(pm_engine* e, const uint64_t* keys, const uint32_t* sites, uint32_t n_waves, uint32_t n_per_wave,
                                  uint32_t slot_bits, uint64_t ulps, uint32_t upto, double tie_band, uint64_t* rows_out,
                                  uint64_t* track_out, uint32_t* flags_out, uint64_t* mine_out, uint32_t* mismatches) {
  if (!e || !keys || !sites || !rows_out || !track_out || !flags_out || !mine_out || !mismatches || !n_waves || (n_waves & 3u) ||
      n_waves > 4096u || !n_per_wave || (slot_bits != PM_CARVE_SLOT_BITS && slot_bits != PM_CARVE_SLOT_BITS_BIG))
    return set_error(PM_EINVAL, "row certificates: null argument, not 4 .. 4096 waves in fours, or a slot width rows do not run at");
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(hipSetDevice(e->cfg.device));
  const size_t nk = size_t(n_waves) * n_per_wave, ns = size_t(1) << slot_bits, nr = size_t(n_waves) * 3;
  DevBuf<uint64_t> d_k, d_rows, d_cr, d_ct, d_cm;
  DevBuf<uint32_t> d_s, d_m, d_cf;
  if (d_k.ensure(nk) != hipSuccess || d_rows.ensure(size_t(n_waves) * 64) != hipSuccess || d_s.ensure(ns) != hipSuccess ||
      d_m.ensure(2) != hipSuccess || d_cr.ensure(nr * 64) != hipSuccess || d_ct.ensure(nr * 5) != hipSuccess ||
      d_cf.ensure(nr * PM_PROP_KMAX) != hipSuccess || d_cm.ensure(nr * PM_PROP_KMAX * 64) != hipSuccess)
    return set_error(PM_ENOMEM, "row certificate test buffers");
  (void)hipMemcpyAsync(d_k.p, keys, nk * 8, hipMemcpyHostToDevice, e->stream);
  (void)hipMemcpyAsync(d_s.p, sites, ns * 4, hipMemcpyHostToDevice, e->stream);
  (void)hipMemsetAsync(d_m.p, 0, 8, e->stream);
  launch_row_network_test(d_k.p, d_s.p, n_waves, n_per_wave, slot_bits, ulps, upto, d_rows.p, d_m.p, e->stream, tie_band, d_cr.p, d_ct.p,
                          d_cf.p, d_cm.p);
  (void)hipMemcpyAsync(rows_out, d_cr.p, nr * 64 * 8, hipMemcpyDeviceToHost, e->stream);
  (void)hipMemcpyAsync(track_out, d_ct.p, nr * 5 * 8, hipMemcpyDeviceToHost, e->stream);
  (void)hipMemcpyAsync(flags_out, d_cf.p, nr * PM_PROP_KMAX * 4, hipMemcpyDeviceToHost, e->stream);
  (void)hipMemcpyAsync(mine_out, d_cm.p, nr * PM_PROP_KMAX * 64 * 8, hipMemcpyDeviceToHost, e->stream);
  (void)hipMemcpyAsync(mismatches, d_m.p, 8, hipMemcpyDeviceToHost, e->stream);
  if (hipStreamSynchronize(e->stream) != hipSuccess) return set_error(PM_ENODEV, "row certificate test");
  return PM_OK;
}

// debug (include/pm_engine_debug.h): the distance key of n pairs by geo_kernel and the carve's own device functions
int32_t pm_debug_distance_keys(pm_engine* e, const double* in, uint32_t n, uint32_t mode, double* out) {
  if (!e || !out || mode > 3u) return set_error(PM_EINVAL, "null argument");
  const bool key_only = mode == 3u;  // (the same launch as mode 0; one column of its records comes back)
  if (key_only) mode = 0u;
  if (mode == 2u) {
    const double c[8] = {PM_A_CHORD_MIN, PM_A_MAX_SAFE, PM_TIE_BAND, PM_TIE_BAND_BIG, PM_TIE_BAND_MEM,
                         double(PM_CARVE_SLOT_BITS), double(PM_CARVE_SLOT_BITS_BIG), double(PM_CARVE_SLOT_BITS_MEM)};
    std::memcpy(out, c, sizeof(c));
    return PM_OK;
  }
  if (!in || n == 0 || n > (1u << 26)) return set_error(PM_EINVAL, "distance keys: 1 to 2^26 inputs");
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(hipSetDevice(e->cfg.device));
  const size_t n_in = mode == 0u ? size_t(5) * n : n, n_out = mode == 0u ? size_t(PM_DK_WORDS) * n : n;
  DevBuf<double> b_in, b_geo, b_out;
  if (b_in.ensure(n_in) != hipSuccess || b_out.ensure(n_out) != hipSuccess || (mode == 0u && b_geo.ensure(size_t(8) * n) != hipSuccess))
    return set_error(PM_ENOMEM, "distance key test buffers");
  double *const d_in = b_in.p, *const d_geo = b_geo.p, *const d_out = b_out.p;
  (void)hipMemcpyAsync(d_in, in, n_in * 8, hipMemcpyHostToDevice, e->stream);
  if (mode == 0u)  // cos(lat), ux, uy, uz of the 2n points, by the kernel that makes the worker table's columns
    launch_geo(d_in, d_in + size_t(2) * n, d_geo, d_geo + size_t(2) * n, d_geo + size_t(4) * n, d_geo + size_t(6) * n, 2u * n,
               e->stream);
  launch_distance_key_test(d_in, d_geo, n, mode, d_out, e->stream);
  if (key_only)  // word 13 of every record: n rows of one f64, PM_DK_WORDS f64 apart
    (void)hipMemcpy2DAsync(out, 8, d_out + 13, size_t(PM_DK_WORDS) * 8, 8, n, hipMemcpyDeviceToHost, e->stream);
  else
    (void)hipMemcpyAsync(out, d_out, n_out * 8, hipMemcpyDeviceToHost, e->stream);
  if (hipStreamSynchronize(e->stream) != hipSuccess) return set_error(PM_ENODEV, "distance key test");
  return PM_OK;
}

// debug (include/pm_engine_debug.h): arm a snapshot of the next formation's first batch (form_queue_pairs takes it:
// first_batch_snapshot, pm_engine_carve.inc); the batch pipeline only
int32_t pm_debug_first_batch_arm(pm_engine* e) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  if (e->cfg.carve_variant != 3) return set_error(PM_ESTATE, "first batch snapshot: the batch pipeline (carve_variant 3) only");
  e->fb_armed = true;
  e->fb_taken = false;
  e->fb_part.clear();
  return PM_OK;
}
// ... and one part of it (PM_FB_*): its size, and with `out` its bytes
int32_t pm_debug_first_batch_get(pm_engine* e, uint32_t part, void* out, uint64_t cap_bytes, uint64_t* n_bytes) {
  if (!e || !n_bytes || part >= PM_FB_PARTS) return set_error(PM_EINVAL, "first batch snapshot: null argument or no such part");
  std::lock_guard<std::mutex> lk(e->mu);
  if (!e->fb_taken || e->fb_part.size() != PM_FB_PARTS) return set_error(PM_ESTATE, "first batch snapshot: none taken");
  const std::vector<unsigned char>& p = e->fb_part[part];
  *n_bytes = p.size();
  if (!out) return PM_OK;
  if (cap_bytes < p.size()) return set_error(PM_ERANGE, "first batch snapshot: buffer too small");
  if (!p.empty()) std::memcpy(out, p.data(), p.size());
  return PM_OK;
}

#ifdef PM_ROW_BENCH
// A measuring build's entry (tools/row_bench.py; not in the headers: the product does not have it): the row of the kth candidate
// of the ci-th available configuration of the LAST match, made `reps` times by one wave alone, every position of the
// configuration's bitmap a candidate.  out[8]: see carve_row_bench_kernel; out[7] = the seed's position.  mode: what is left out
// (bits: 1 the row, 2 the key arithmetic, 4 the gathers, 8 everything but the passes over the bitmap).
extern "C" int32_t pm_debug_row_bench(pm_engine* e, uint32_t ci, uint32_t kth, uint32_t reps, uint32_t mode, unsigned long long* out) {
  if (!e || !out) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(hipSetDevice(e->cfg.device));
  if (!e->d_carve_args.p) return set_error(PM_ESTATE, "no match yet");
  CarveArgs h;
  HIPCHK(hipMemcpy(&h, e->d_carve_args.p, sizeof(h), hipMemcpyDeviceToHost));
  if (!h.cfgbits || !h.bits_stride || ci >= h.n_avail) return set_error(PM_ESTATE, "no configuration bitmaps");
  std::vector<uint64_t> row(h.bits_stride);
  HIPCHK(hipMemcpy(row.data(), h.cfgbits + size_t(ci) * h.bits_stride, h.bits_stride * 8, hipMemcpyDeviceToHost));
  uint32_t seed = PM_NONE, seen = 0;
  for (size_t j = 0; j < row.size() && seed == PM_NONE; ++j)
    for (uint64_t w = row[j]; w; w &= w - 1)
      if (seen++ == kth) {
        seed = uint32_t(j * 64 + __builtin_ctzll(w));
        break;
      }
  if (seed == PM_NONE) return set_error(PM_EINVAL, "fewer candidates than that");
  DevBuf<unsigned long long> d_ones, d_out;
  DevBuf<CarveArgs> d_h;
  if (d_ones.ensure(h.bits_stride) != hipSuccess || d_out.ensure(8) != hipSuccess || d_h.ensure(1) != hipSuccess)
    return set_error(PM_ENOMEM, "row bench buffers");
  int32_t rc = PM_OK;
  (void)hipMemset(d_ones.p, 0xFF, h.bits_stride * 8);
  (void)hipMemset(d_out.p, 0, 64);
  h.bits_scratch = (uint64_t*)d_ones.p;
  (void)hipMemcpy(d_h.p, &h, sizeof(h), hipMemcpyHostToDevice);
  if (launch_row_bench(d_h.p, seed, ci, reps, mode, d_out.p, e->stream) != hipSuccess || hipStreamSynchronize(e->stream) != hipSuccess)
    rc = set_error(PM_ENODEV, "row bench");
  else
    (void)hipMemcpy(out, d_out.p, 64, hipMemcpyDeviceToHost);
  out[7] = seed;
  return rc;
}
#endif

// debug (include/pm_engine_debug.h): what the owning types of pm_owned.h hold in this process right now
void pm_debug_live_allocations(uint64_t out[3]) {
  for (int k = 0; k < 3; ++k) out[k] = g_live_allocs[k].load(std::memory_order_relaxed);
}

int32_t pm_last_stats(pm_engine* e, pm_stats* stats) {
  if (!e || !stats) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  *stats = e->last_stats;
  return PM_OK;
}

