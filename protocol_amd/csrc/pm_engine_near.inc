// pm_engine_near.inc — part of pm_engine.cpp (one translation unit; included in place): C ABI: pm_nearest_workers (kernel in
// pm_near.inc) (inside extern "C").
//
// The call keeps the promises of pm_engine_report.inc: it answers from the state every earlier call left (the host's flags
// column and group_of, pending changes included, through the reports' scratch uploads), consumes no pending delta, compacts
// nothing, clears no flag of the tick, and writes scratch of its own (d_near_*).  One launch, one packed copy out, one
// synchronisation.

int32_t pm_nearest_workers(pm_engine* e, const pm_near_query* q, uint32_t n_q, uint32_t pool, uint32_t k, pm_near_row* rows,
                           uint32_t* workers, double* km) {
  if (!e || (n_q && (!q || !rows || !workers))) return set_error(PM_EINVAL, "null argument");
  if (k == 0u || k > PM_NEAR_MAX_K) return set_error(PM_EINVAL, "k must be in [1, PM_NEAR_MAX_K]");
  if (n_q > PM_NEAR_MAX_QUERIES) return set_error(PM_EINVAL, "more than PM_NEAR_MAX_QUERIES queries");
  if (pool > PM_NEAR_ELIGIBLE) return set_error(PM_EINVAL, "unknown pool");
  std::lock_guard<std::mutex> lk(e->mu);
  int32_t rc = report_begin(e, false);
  if (rc) return rc;
  for (uint32_t i = 0; i < n_q; ++i) {
    if (q[i].origin >= e->W && q[i].origin != PM_NEAR_SEED) return set_error(PM_ERANGE, "origin worker index out of range");
    if (q[i].config >= e->cfgs.size()) return set_error(PM_ERANGE, "configuration index out of range");
  }
  if (!n_q) return PM_OK;
  NearArgs a{};
  if ((rc = report_compat_args(e, &a.c))) return rc;
  a.group_of = e->d_group_of.p;
  if (e->groups_dirty && e->W) {  // (dissolutions and new rows the device has not seen yet)
    if ((rc = upload(e->d_rep_gof, e->h_group_of.data(), e->W, e->stream))) return rc;
    a.group_of = e->d_rep_gof.p;
  }
  a.lat = e->d_lat.p, a.lon = e->d_lon.p, a.coslat = e->d_coslat.p;
  if ((rc = upload(e->d_near_q, q, n_q, e->stream))) return rc;
  a.q = e->d_near_q.p;
  a.n_q = n_q, a.pool = pool, a.k = k;
  // [km n_q * k f64][rows n_q x 16 B][workers n_q * k u32], in f64 words
  const size_t n_km = size_t(n_q) * k, o_rows = n_km, o_w = o_rows + 2u * size_t(n_q), words = o_w + (n_km + 1u) / 2u;
  HIPCHK(e->d_near_out.ensure(words));
  a.km = e->d_near_out.p;
  a.rows = reinterpret_cast<pm_near_row*>(e->d_near_out.p + o_rows);
  a.workers = reinterpret_cast<uint32_t*>(e->d_near_out.p + o_w);
  launch_nearest(a, e->stream);
  HIPCHK(hipGetLastError());
  e->h_near_out.resize(words);
  HIPCHK(hipMemcpyAsync(e->h_near_out.data(), e->d_near_out.p, words * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));  // (the pageable sources of the uploads die here too)
  const double* h = e->h_near_out.data();
  if (km) std::memcpy(km, h, n_km * sizeof(double));
  std::memcpy(rows, h + o_rows, size_t(n_q) * sizeof(pm_near_row));
  std::memcpy(workers, h + o_w, n_km * sizeof(uint32_t));
  return PM_OK;
}
