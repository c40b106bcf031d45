// pm_engine_workers.inc — part of pm_engine.cpp (one translation unit; included in place): C ABI: worker table ingestion (upload / update / append / address ranks) (inside extern "C").
// ---- worker table ingestion.  Coordinates are interned into site ids (the carve certificate needs "same place"
// as an exact integer compare); the map persists so that row deltas intern incrementally.

static inline void site_key(double lat, double lon, uint64_t* a, uint64_t* b) {
  std::memcpy(a, &lat, 8);
  std::memcpy(b, &lon, 8);
  if (lat == 0.0) *a = 0;  // +0.0 and -0.0 compare equal in the reference's f64 arithmetic
  if (lon == 0.0) *b = 0;
}

static uint32_t site_of_row(pm_engine* e, size_t w) {
  uint64_t a, b;
  site_key(e->h_lat[w], e->h_lon[w], &a, &b);
  const uint32_t id = e->site_map.find_or_insert(a, b);
  if (id >= e->site_pop.size()) e->site_pop.push_back(0);
  return id;
}

static void refresh_site_bits(pm_engine* e) {
  for (size_t w = 0; w < e->W; ++w) {
    const uint32_t id = e->h_site[w] & 0x7FFFFFFFu;
    e->h_site[w] = id | (e->site_pop[id] >= 2 ? 0x80000000u : 0u);
  }
  e->site_bits_dirty = false;
}

// the whole table: host mirror -> HBM columns
static int32_t upload_worker_columns(pm_engine* e) {
  const size_t W = e->W;
  int32_t rc;
  if ((rc = upload(e->d_flags, e->h_flags.data(), W, e->stream))) return rc;
  if ((rc = upload(e->d_gpu_count, e->h_gpu_count.data(), W, e->stream))) return rc;
  if ((rc = upload(e->d_gpu_mem, e->h_gpu_mem.data(), W, e->stream))) return rc;
  if ((rc = upload(e->d_gpu_cls, e->h_gpu_cls.data(), W, e->stream))) return rc;
  if ((rc = upload(e->d_cpu_cores, e->h_cpu_cores.data(), W, e->stream))) return rc;
  if ((rc = upload(e->d_ram, e->h_ram.data(), W, e->stream))) return rc;
  if ((rc = upload(e->d_storage, e->h_storage.data(), W, e->stream))) return rc;
  if ((rc = upload(e->d_addr_rank, e->h_addr_rank.data(), W, e->stream))) return rc;
  if ((rc = upload(e->d_lat, e->h_lat.data(), W, e->stream))) return rc;
  if ((rc = upload(e->d_lon, e->h_lon.data(), W, e->stream))) return rc;
  e->site_map.clear();
  e->site_map.reserve(W * 2);
  e->site_pop.clear();
  e->h_site.resize(W);
  for (size_t w = 0; w < W; ++w) {
    e->h_site[w] = site_of_row(e, w);
    e->site_pop[e->h_site[w]] += (e->h_flags[w] & PM_W_HAS_LOC) ? 1u : 0u;
  }
  refresh_site_bits(e);
  if ((rc = upload(e->d_site, e->h_site.data(), W, e->stream))) return rc;
  HIPCHK(e->d_coslat.ensure(W ? W : 1));
  HIPCHK(e->d_ux.ensure(W ? W : 1));
  HIPCHK(e->d_uy.ensure(W ? W : 1));
  HIPCHK(e->d_uz.ensure(W ? W : 1));
  launch_geo(e->d_lat.p, e->d_lon.p, e->d_coslat.p, e->d_ux.p, e->d_uy.p, e->d_uz.p, uint32_t(W), e->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(e->stream));
  e->flags_dirty = false;
  e->flags_delta_ok = true;  // (the whole column has just gone up)
  e->delta_flags.clear();
  e->price_dirty = true;
  e->compat_dirty = true;
  return PM_OK;
}

// (price, index) order of the swept axis for pm_match_per_task; rebuilt only when a price changed
static void ensure_price_order(pm_engine* e) {
  if (!e->price_dirty) return;
  e->any_price = std::any_of(e->h_price.begin(), e->h_price.end(), [](uint32_t p) { return p != 0; });
  e->price_perm.clear();
  if (e->any_price) {
    e->price_perm.resize(e->W);
    for (uint32_t i = 0; i < e->W; ++i) e->price_perm[i] = i;
    std::stable_sort(e->price_perm.begin(), e->price_perm.end(),
                     [&](uint32_t a, uint32_t b) { return e->h_price[a] < e->h_price[b]; });
  }
  e->price_dirty = false;
}

static bool worker_soa_complete(const pm_worker_soa* w) {
  return !w->n || (w->flags && w->gpu_count && w->gpu_mem_mb && w->gpu_model_class && w->cpu_cores && w->ram_mb &&
                   w->storage_gb && w->lat && w->lon);
}

int32_t pm_upload_workers(pm_engine* e, const pm_worker_soa* w, uint32_t keep_groups) {
  if (!e || !w) return set_error(PM_EINVAL, "null argument");
  const uint32_t n = w->n;
  if (!worker_soa_complete(w)) return set_error(PM_EINVAL, "null worker column");
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(hipSetDevice(e->cfg.device));
  if (e->dist_phase != 0) return set_error(PM_ESTATE, "a stepwise tick is in progress");
  ABSORB_PENDING(e);
  if (keep_groups && e->have_workers && n < e->W)
    return set_error(PM_EINVAL, "keep_groups requires the rows the engine has, in the same order, in front (rows behind them "
                                "are new ones, as pm_append_workers would add them)");
  if (n != e->W && e->dist_world > 1) {  // ownership is per worker row: pm_dist_configure must follow
    e->h_shard.clear();
    e->h_own_rows.clear();
  }
  e->W = n;
  e->h_flags.assign(w->flags, w->flags + n);
  e->h_gpu_count.assign(w->gpu_count, w->gpu_count + n);
  e->h_gpu_mem.assign(w->gpu_mem_mb, w->gpu_mem_mb + n);
  e->h_gpu_cls.assign(w->gpu_model_class, w->gpu_model_class + n);
  e->cls_check_dirty = true;
  e->h_cpu_cores.assign(w->cpu_cores, w->cpu_cores + n);
  e->h_ram.assign(w->ram_mb, w->ram_mb + n);
  e->h_storage.assign(w->storage_gb, w->storage_gb + n);
  if (w->price) e->h_price.assign(w->price, w->price + n); else e->h_price.assign(n, 0);
  if (w->addr_rank) {
    e->h_addr_rank.assign(w->addr_rank, w->addr_rank + n);
  } else {
    e->h_addr_rank.resize(n);
    for (uint32_t i = 0; i < n; ++i) e->h_addr_rank[i] = i;
  }
  e->h_lat.assign(w->lat, w->lat + n);
  e->h_lon.assign(w->lon, w->lon + n);
  int32_t rc = upload_worker_columns(e);
  if (rc) return rc;
  e->have_workers = true;
  if (!keep_groups || e->h_group_of.size() > n) {
    e->live.reinit = true;  // (liveness: the row identities are gone, the next liveness call starts the ledger over)
    e->mx.reinit = true;    // (metrics: the next metrics call empties every worker row)
    e->ro.reinit = true;    // (rollout: the next rollout call empties every row)
    e->ab.reinit = true;    // (address book: the next book call clears every row's flag)
    e->ad.reinit = true;    // (admission: the next admission call empties the rate ledger and the beats; the nonce set stays)
    reset_groups_locked(e);
  } else {
    e->h_group_of.resize(n, -1);  // (rows behind the known ones are new: in no group)
  }
  e->groups_dirty = true, e->groups_delta_ok = false;
  return PM_OK;
}

// Rows idx[0..n) <- rows: host mirror, incremental site interning, then ONE packed H2D copy and a scatter kernel
// (update_rows_kernel also refreshes cos(lat)).  Shared by pm_update_workers and pm_append_workers.
static int32_t scatter_rows(pm_engine* e, const uint32_t* idx, const pm_worker_soa* rows, uint32_t first_new) {
  const uint32_t n = rows->n;
  if (!n) return PM_OK;
  constexpr uint32_t AHEAD = 12;  // rows whose slot of the site map is asked for ahead of their turn (SiteMap::prefetch)
  for (uint32_t k = 0; k < n && k < AHEAD; ++k) {
    uint64_t a, b;
    site_key(rows->lat[k], rows->lon[k], &a, &b);
    e->site_map.prefetch(a, b);
  }
  for (uint32_t k = 0; k < n; ++k) {
    if (k + AHEAD < n) {
      uint64_t a, b;
      site_key(rows->lat[k + AHEAD], rows->lon[k + AHEAD], &a, &b);
      e->site_map.prefetch(a, b);
    }
    const uint32_t w = idx[k];
    if (w < first_new) {  // an existing row leaves its old site (rows from first_new on are being appended)
      const uint32_t old = e->h_site[w] & 0x7FFFFFFFu;
      if ((e->h_flags[w] & PM_W_HAS_LOC) && old < e->site_pop.size()) {
        if (e->site_pop[old] == 2) e->site_bits_dirty = true;
        if (e->site_pop[old]) e->site_pop[old]--;
      }
    }
    e->h_flags[w] = rows->flags[k];
    e->h_gpu_count[w] = rows->gpu_count[k];
    e->h_gpu_mem[w] = rows->gpu_mem_mb[k];
    e->h_gpu_cls[w] = rows->gpu_model_class[k];
    e->cls_check_dirty = true;
    e->h_cpu_cores[w] = rows->cpu_cores[k];
    e->h_ram[w] = rows->ram_mb[k];
    e->h_storage[w] = rows->storage_gb[k];
    if (rows->price) {
      if (e->h_price[w] != rows->price[k]) e->price_dirty = true;
      e->h_price[w] = rows->price[k];
    }
    if (rows->addr_rank) e->h_addr_rank[w] = rows->addr_rank[k];
    e->h_lat[w] = rows->lat[k];
    e->h_lon[w] = rows->lon[k];
    const uint32_t id = site_of_row(e, w);
    if (rows->flags[k] & PM_W_HAS_LOC) {
      if (e->site_pop[id] == 1) e->site_bits_dirty = true;
      e->site_pop[id]++;
    }
    e->h_site[w] = id | (e->site_pop[id] >= 2 ? 0x80000000u : 0u);
  }
  // packed staging: [lat n][lon n] f64, then 10 u32 columns: idx, flags, gpu_count, gpu_mem, gpu_cls, cpu_cores,
  // ram, storage, addr_rank, site
  const size_t bytes = size_t(n) * (16 + 10 * 4);
  // pinned staging, reused: whatever was last sent from it (and read from the device stage) must be through — an idle
  // stream answers at once, and a delta arrives between two ticks
  // (asked through an event: the wait on an idle stream was 13 us of an append)
  host_mark("rows: host mirror written");
  if (!e->ev_row_stage) HIPCHK(e->ev_row_stage.create(hipEventDisableTiming));
  else if (hipEventQuery(e->ev_row_stage) != hipSuccess) HIPCHK(hipStreamSynchronize(e->stream));
  host_mark("rows: staging free");
  HIPCHK(e->h_row_pin.ensure(bytes, bytes + bytes / 2 + 4096));
  double* hd = reinterpret_cast<double*>(e->h_row_pin.p);
  uint32_t* hu = reinterpret_cast<uint32_t*>(e->h_row_pin.p + size_t(n) * 16);
  for (uint32_t k = 0; k < n; ++k) {
    const uint32_t w = idx[k];
    hd[k] = e->h_lat[w];
    hd[n + k] = e->h_lon[w];
    hu[0 * size_t(n) + k] = w;
    hu[1 * size_t(n) + k] = e->h_flags[w];
    hu[2 * size_t(n) + k] = e->h_gpu_count[w];
    hu[3 * size_t(n) + k] = e->h_gpu_mem[w];
    hu[4 * size_t(n) + k] = e->h_gpu_cls[w];
    hu[5 * size_t(n) + k] = e->h_cpu_cores[w];
    hu[6 * size_t(n) + k] = e->h_ram[w];
    hu[7 * size_t(n) + k] = e->h_storage[w];
    hu[8 * size_t(n) + k] = e->h_addr_rank[w];
    hu[9 * size_t(n) + k] = e->h_site[w];
  }
  HIPCHK(e->d_row_stage.ensure(bytes));
  HIPCHK(hipMemcpyAsync(e->d_row_stage.p, e->h_row_pin.p, bytes, hipMemcpyHostToDevice, e->stream));
  RowUpdateArgs a{};
  a.n = n;
  a.lat_in = reinterpret_cast<const double*>(e->d_row_stage.p);
  a.lon_in = a.lat_in + n;
  a.u32_in = reinterpret_cast<const uint32_t*>(e->d_row_stage.p + size_t(n) * 16);
  a.flags = e->d_flags.p;
  a.gpu_count = e->d_gpu_count.p;
  a.gpu_mem = e->d_gpu_mem.p;
  a.gpu_cls = e->d_gpu_cls.p;
  a.cpu_cores = e->d_cpu_cores.p;
  a.ram = e->d_ram.p;
  a.storage = e->d_storage.p;
  a.addr_rank = e->d_addr_rank.p;
  a.site = e->d_site.p;
  a.lat = e->d_lat.p;
  a.lon = e->d_lon.p;
  a.coslat = e->d_coslat.p;
  a.ux = e->d_ux.p;
  a.uy = e->d_uy.p;
  a.uz = e->d_uz.p;
  launch_update_rows(a, e->stream);
  HIPCHK(hipGetLastError());   // (not waited for: the staging is pinned and the engine's own; the next use of it waits)
  HIPCHK(hipEventRecord(e->ev_row_stage, e->stream));
  host_mark("rows: copy and scatter queued");
  if (e->site_bits_dirty) {  // a site crossed the one <-> two located workers line: refresh the hint bits
    refresh_site_bits(e);
    int32_t rc = upload(e->d_site, e->h_site.data(), e->W, e->stream);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  e->compat_dirty = true;
  e->h_compat_valid = false;
  return PM_OK;
}

int32_t pm_update_workers(pm_engine* e, const uint32_t* idx, const pm_worker_soa* rows) {
  if (!e || !rows || (rows->n && !idx)) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  if (!e->have_workers) return set_error(PM_ESTATE, "workers must be uploaded first");
  if (!worker_soa_complete(rows)) return set_error(PM_EINVAL, "null worker column");
  HIPCHK(hipSetDevice(e->cfg.device));
  if (e->dist_phase != 0) return set_error(PM_ESTATE, "a stepwise tick is in progress");
  for (uint32_t k = 0; k < rows->n; ++k)
    if (idx[k] >= e->W) return set_error(PM_ERANGE, "worker index out of range");
  // (status-only changes made since the last upload stay pending, see pm_append_workers: what goes up later is the host
  // column's value at that time, which this call has written)
  return scatter_rows(e, idx, rows, e->W);
}

int32_t pm_append_workers(pm_engine* e, const pm_worker_soa* rows, uint32_t* first_index) {
  if (!e || !rows) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  if (!e->have_workers) return set_error(PM_ESTATE, "workers must be uploaded first (an empty table is fine)");
  if (!worker_soa_complete(rows)) return set_error(PM_EINVAL, "null worker column");
  HIPCHK(hipSetDevice(e->cfg.device));
  if (e->dist_phase != 0) return set_error(PM_ESTATE, "a stepwise tick is in progress");
  ABSORB_PENDING(e);
  const uint32_t w0 = e->W, n = rows->n;
  if (first_index) *first_index = w0;
  if (!n) return PM_OK;
  if (uint64_t(w0) + n > 0x7FFFFFFFull) return set_error(PM_ERANGE, "worker table too large");
  host_mark("append: begin");
  // (status-only changes made since the last upload stay pending: they are {index, value-at-upload-time} pairs — or the whole
  // host column — applied on this stream before the next kernel that reads the flags (sync_flags in ensure_compat), behind the
  // scatter below; a copy and a launch here were a tenth of an append)
  int32_t rc = PM_OK;
  const size_t W1 = size_t(w0) + n;
  HIPCHK(e->d_flags.grow_keep(W1, w0, e->stream));
  HIPCHK(e->d_gpu_count.grow_keep(W1, w0, e->stream));
  HIPCHK(e->d_gpu_mem.grow_keep(W1, w0, e->stream));
  HIPCHK(e->d_gpu_cls.grow_keep(W1, w0, e->stream));
  HIPCHK(e->d_cpu_cores.grow_keep(W1, w0, e->stream));
  HIPCHK(e->d_ram.grow_keep(W1, w0, e->stream));
  HIPCHK(e->d_storage.grow_keep(W1, w0, e->stream));
  HIPCHK(e->d_addr_rank.grow_keep(W1, w0, e->stream));
  HIPCHK(e->d_site.grow_keep(W1, w0, e->stream));
  HIPCHK(e->d_lat.grow_keep(W1, w0, e->stream));
  HIPCHK(e->d_lon.grow_keep(W1, w0, e->stream));
  HIPCHK(e->d_coslat.grow_keep(W1, w0, e->stream));
  HIPCHK(e->d_ux.grow_keep(W1, w0, e->stream));
  HIPCHK(e->d_uy.grow_keep(W1, w0, e->stream));
  HIPCHK(e->d_uz.grow_keep(W1, w0, e->stream));
  e->h_flags.resize(W1, 0);
  e->h_gpu_count.resize(W1, 0);
  e->h_gpu_mem.resize(W1, 0);
  e->h_gpu_cls.resize(W1, 0);
  e->h_cpu_cores.resize(W1, 0);
  e->h_ram.resize(W1, 0);
  e->h_storage.resize(W1, 0);
  e->h_price.resize(W1, 0);
  e->h_addr_rank.resize(W1, 0);
  e->h_lat.resize(W1, 0.0);
  e->h_lon.resize(W1, 0.0);
  e->h_site.resize(W1, 0);
  std::vector<uint32_t> idx(n);
  for (uint32_t k = 0; k < n; ++k) {
    idx[k] = w0 + k;
    if (!rows->addr_rank) e->h_addr_rank[w0 + k] = w0 + k;
  }
  // a new row joins no group: the existing groups and their claimed tasks stay as they are (mod.rs:487-497)
  e->h_group_of.resize(W1, -1);
  e->W = uint32_t(W1);
  host_mark("append: columns grown");
  rc = scatter_rows(e, idx.data(), rows, w0);
  if (rc) return rc;
  if (e->dist_world > 1) {  // ownership is per worker row: pm_dist_configure must follow
    e->h_shard.clear();
    e->h_own_rows.clear();
  }
  e->price_dirty = true;
  if (e->groups_delta_ok && e->delta_tail_from == PM_NONE) e->delta_tail_from = w0;
  e->groups_dirty = true;  // group_of is sized by W (a delta while groups_delta_ok: see push_groups)
  return PM_OK;
}

int32_t pm_set_addr_ranks(pm_engine* e, const uint32_t* addr_rank, uint32_t n) {
  if (!e || (n && !addr_rank)) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  if (!e->have_workers || n != e->W) return set_error(PM_ERANGE, "one rank per worker row");
  HIPCHK(hipSetDevice(e->cfg.device));
  e->h_addr_rank.assign(addr_rank, addr_rank + n);
  int32_t rc = upload(e->d_addr_rank, e->h_addr_rank.data(), n, e->stream);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(e->stream));
  return PM_OK;
}

