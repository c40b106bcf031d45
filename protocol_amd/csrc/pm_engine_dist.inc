// pm_engine_dist.inc — part of pm_engine.cpp (one translation unit; included in place): C ABI: multi-GPU stepwise tick, pm_set_stream, and the lock-free look-up (inside extern "C").
// ------------------------------------------------------------------------------------------------
// multi-GPU: ownership, the stepwise tick and its two exchanges (see include/pm_engine.h)

// Pools sharing one GPU: the carve's launch keeps one workgroup per CU resident from its first configuration to its
// last (the validator + its row-making workgroups), so K engines matching at the same time fit side by side only if
// each asks for its share of the CUs.  0 = by the size of the eligible list (a pool with the GPU to itself).
int32_t pm_set_carve_workgroups(pm_engine* e, uint32_t n) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  if (n > 4096u) return set_error(PM_EINVAL, "carve workgroups 0..4096");
  std::lock_guard<std::mutex> lk(e->mu);
  e->stream_wgs_env = n;
  return PM_OK;
}

int32_t pm_set_stream(pm_engine* e, void* hip_stream) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(hipSetDevice(e->cfg.device));
  if (e->dist_phase != 0) return set_error(PM_ESTATE, "a stepwise tick is in progress");
  HIPCHK(hipStreamSynchronize(e->stream));
  if (hip_stream) {
    e->stream = static_cast<hipStream_t>(hip_stream);
    e->own_stream = false;
  } else {
    e->stream = e->stream_owned;
    e->own_stream = true;
  }
  return PM_OK;
}

static void dist_abort(pm_engine* e) {
  e->form.reset();
  e->dist_phase = 0;
}

int32_t pm_dist_configure(pm_engine* e, uint32_t rank, uint32_t world, const uint8_t* shard_of_worker) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  if (world == 0 || world > 64 || rank >= world) return set_error(PM_EINVAL, "rank / world out of range (world <= 64)");
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(hipSetDevice(e->cfg.device));
  if (e->dist_phase != 0) return set_error(PM_ESTATE, "a stepwise tick is in progress");
  if (world > 1 && e->chg.on) return set_error(PM_ESTATE, "the assignment change feed is on: it does not cover multi-GPU engines");
  if (world > 1 && e->live.on) return set_error(PM_ESTATE, "liveness is on: it does not cover multi-GPU engines");
  if (world > 1 && e->mx.on) return set_error(PM_ESTATE, "the metrics ledger is on: it does not cover multi-GPU engines");
  if (world > 1 && e->ro.on) return set_error(PM_ESTATE, "the rollout ledger is on: it does not cover multi-GPU engines");
  if (world > 1 && !e->have_workers) return set_error(PM_ESTATE, "workers must be uploaded first");
  if (world > 1 && e->W && !shard_of_worker) return set_error(PM_EINVAL, "null shard column");
  e->dist_rank = world > 1 ? rank : 0;
  e->dist_world = world;
  e->h_shard.clear();
  e->h_own_rows.clear();
  e->dist_cap_t = 0;
  if (world == 1) return PM_OK;
  const uint32_t W = e->W;
  for (uint32_t w = 0; w < W; ++w)
    if (shard_of_worker[w] >= world) return set_error(PM_ERANGE, "shard index outside the world");
  e->h_shard.assign(shard_of_worker, shard_of_worker + W);
  std::vector<uint32_t> count(world, 0), xrow(W);
  for (uint32_t w = 0; w < W; ++w) xrow[w] = count[e->h_shard[w]]++;  // index within the shard, in worker order
  const uint32_t cap_t = std::max<uint32_t>(*std::max_element(count.begin(), count.end()), 1u);
  for (uint32_t w = 0; w < W; ++w) {
    xrow[w] += uint32_t(e->h_shard[w]) * cap_t;
    if (e->h_shard[w] == rank) e->h_own_rows.push_back(w);
  }
  e->dist_cap_t = cap_t;
  int32_t rc = upload(e->d_shard, e->h_shard.data(), W, e->stream);
  if (rc) return rc;
  rc = upload(e->d_own_rows, e->h_own_rows.data(), e->h_own_rows.size(), e->stream);
  if (rc) return rc;
  rc = upload(e->d_xrow, xrow.data(), W, e->stream);
  if (rc) return rc;
  HIPCHK(e->d_table_x.ensure(size_t(cap_t) * world));
  HIPCHK(hipMemsetAsync(e->d_table_x.p, 0xFF, sizeof(pm_assignment) * size_t(cap_t) * world, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));  // the staging vectors die here
  return PM_OK;
}

int32_t pm_dist_tick_begin(pm_engine* e) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(hipSetDevice(e->cfg.device));
  if (!e->have_cfgs || !e->have_workers || !e->have_tasks)
    return set_error(PM_ESTATE, "configs, workers and tasks must be uploaded first");
  if (e->dist_phase != 0) dist_abort(e);  // an abandoned stepwise tick
  if (e->dist_world > 1 && e->h_shard.size() != e->W)
    return set_error(PM_ESTATE, "the worker table changed size: call pm_dist_configure again");
  tick_reset(e);
  HIPCHK(hipEventRecord(e->ev[0], e->stream));
  e->compat_dirty = true;
  int32_t rc = ensure_compat(e);
  if (rc) return rc;
  HIPCHK(hipEventRecord(e->ev[1], e->stream));
  e->form.reset(new (std::nothrow) FormRun());
  if (!e->form) return set_error(PM_ENOMEM, "out of host memory");
  // The carve is REPLICATED: every rank runs the whole of it — the streaming launch, as on one GPU — and ends with the
  // identical groups and ids, because the result does not depend on how the launch went (which rows arrived when), only
  // on the reference's rule: nothing is exchanged until the published table (DESIGN.md section 7).
  rc = form_begin(e, e->form.get());
  if (rc) {
    dist_abort(e);
    return rc;
  }
  e->dist_phase = 1;
  return PM_OK;
}

int32_t pm_dist_carve_wait(pm_engine* e) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(hipSetDevice(e->cfg.device));
  if (e->dist_phase != 1) return set_error(PM_ESTATE, "pm_dist_tick_begin first");
  FormRun* r = e->form.get();
  if (!r->nothing) {
    int32_t rc = run_form_wait(e, *r);
    if (rc) {
      dist_abort(e);
      return rc;
    }
    if (r->st.state != CARVE_STATE_DONE) {
      dist_abort(e);
      return set_error(PM_ENODEV, "carve kernel did not complete");
    }
  }
  e->dist_phase = 2;
  return PM_OK;
}

int32_t pm_dist_match_begin(pm_engine* e, pm_dist_xfer* x) {
  if (!e || !x) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(hipSetDevice(e->cfg.device));
  if (e->dist_phase != 2) return set_error(PM_ESTATE, "the carve is not finished (pm_dist_carve_wait first)");
  std::memset(x, 0, sizeof(*x));
  int32_t rc = form_finish(e, e->form.get(), &e->dist_n_formed, /*defer_absorb=*/true);
  e->form.reset();
  if (rc == PM_OK) {
    HIPCHK(hipEventRecord(e->ev[2], e->stream));
    rc = run_merge(e, &e->dist_n_merged);
  }
  if (rc == PM_OK) {
    HIPCHK(hipEventRecord(e->ev[3], e->stream));
    rc = run_match(e, false, nullptr, e->dist_world > 1);
  }
  if (rc) {
    e->dist_phase = 0;
    return rc;
  }
  HIPCHK(hipEventRecord(e->ev[4], e->stream));
  if (e->dist_world > 1) {
    x->recv_ptr = uint64_t(reinterpret_cast<uintptr_t>(e->d_table_x.p));
    x->send_ptr = uint64_t(reinterpret_cast<uintptr_t>(e->d_table_x.p + size_t(e->dist_rank) * e->dist_cap_t));
    x->bytes_per_rank = uint64_t(e->dist_cap_t) * sizeof(pm_assignment);
  }
  e->dist_phase = 3;
  return PM_OK;
}

int32_t pm_dist_tick_end(pm_engine* e, pm_stats* stats) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(hipSetDevice(e->cfg.device));
  if (e->dist_phase != 3) return set_error(PM_ESTATE, "pm_dist_match_begin first");
  e->dist_phase = 0;
  if (e->dist_world > 1) {
    launch_table_scatter(e->d_table_x.p, e->d_xrow.p, e->W, e->d_table.p, e->d_task_col.p, e->d_g_task_next.p,
                         e->d_tlive.p, e->d_tprefix.p, e->stream);
    HIPCHK(hipGetLastError());
  }
  int32_t rc = absorb_groups(e);
  if (rc) return rc;
  rc = publish(e);
  if (rc) return rc;
  return tick_stats(e, stats, e->dist_n_formed, e->dist_n_merged);
}

int32_t pm_lookup_task_for_worker(pm_engine* e, uint32_t worker, pm_assignment* out) {
  if (!e || !out) return set_error(PM_EINVAL, "null argument");
  for (;;) {
    const int cur = e->pub_cur.load(std::memory_order_acquire);
    if (cur < 0) return set_error(PM_ESTATE, "no assignment table published yet");
    const PubTable& t = e->pub[cur];
    const uint64_t s1 = t.seq.load(std::memory_order_acquire);
    if (s1 & 1u) continue;  // two publishes since `cur` was read: take the newer buffer
    const uint64_t* words = t.words.load(std::memory_order_relaxed);
    const uint32_t n = t.n.load(std::memory_order_relaxed);
    const uint32_t shift = t.task_shift.load(std::memory_order_relaxed);
    const uint32_t cleared = t.cleared.load(std::memory_order_relaxed);
    uint64_t row[4] = {0, 0, 0, 0};
    const bool in_range = worker < n;
    if (in_range)
      for (int k = 0; k < 4; ++k) row[k] = __atomic_load_n(&words[size_t(worker) * 4 + k], __ATOMIC_RELAXED);
    std::atomic_thread_fence(std::memory_order_acquire);
    if (t.seq.load(std::memory_order_relaxed) != s1) continue;
    if (!in_range) return set_error(PM_ERANGE, "worker index out of range");
    std::memcpy(out, row, sizeof(*out));
    if (cleared) {  // (pm_reset_groups since this buffer was written)
      std::memset(out, 0, sizeof(*out));
      out->task = PM_NONE;
      out->group_slot = PM_NONE;
      out->next_worker = PM_NONE;
    }
    if (out->task != PM_NONE) out->task += shift;
    return PM_OK;
  }
}

int32_t pm_device_task_column(pm_engine* e, uint64_t* device_ptr, uint32_t* n) {
  if (!e || !device_ptr || !n) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  if (!e->d_task_col.p) return set_error(PM_ESTATE, "no assignment table computed yet");
  *device_ptr = uint64_t(reinterpret_cast<uintptr_t>(e->d_task_col.p));
  *n = e->W;
  return PM_OK;
}

