// pm_engine_discovery.inc — part of pm_engine.cpp (one translation unit; included in place): the discovery sync, C ABI:
// pm_discovery_sync (kernels in pm_discovery.inc).  Its scratch (struct Discovery) is released with the liveness ledger
// (liveness_release).  Included at file scope, behind pm_engine_liveness.inc.
//
// Everything a kernel indexes with is checked here first, on the host, in one pass over the rows and one over the endpoint
// column: a failing call has then touched neither the device nor the ledger.  The inputs travel as one staged copy (the rows,
// behind them the column), the results as one copy back, behind one stream synchronisation; an applying call builds its update
// list from those results on the host.
extern "C" {

int32_t pm_discovery_sync(pm_engine* e, uint64_t now_ms, const uint32_t* row_endpoint, uint32_t n_endpoints,
                          uint32_t max_healthy_same_endpoint, const pm_disc_row* rows, uint32_t n_rows, uint32_t apply,
                          pm_disc_result* out, uint32_t* n_updates_total) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  int32_t rc = liveness_guard(e);
  if (rc) return rc;
  const uint32_t W = e->W, D = n_rows, E = n_endpoints;
  if (D && !rows) return set_error(PM_EINVAL, "null rows");
  if (W && !row_endpoint) return set_error(PM_EINVAL, "null endpoint column");
  if (uint64_t(E) > uint64_t(W) + 2ull * D) return set_error(PM_EINVAL, "more endpoint ids than the table and the list can name");
  const uint32_t all_flags = PM_DF_VALIDATED | PM_DF_WHITELISTED | PM_DF_ACTIVE | PM_DF_LOCATION_NEW | PM_DF_SPECS_DIFFER | PM_DF_BALANCE_ZERO;
  for (uint32_t j = 0; j < D; ++j)
    if (rows[j].flags & ~all_flags) return set_error(PM_EINVAL, "unknown discovery flag bits");
  for (uint32_t j = 0; j < D; ++j) {
    const pm_disc_row& r = rows[j];
    if (r.row != PM_DISC_NEW && r.row >= W) return set_error(PM_ERANGE, "discovery row: table row out of range");
    if (r.endpoint >= E || (r.row != PM_DISC_NEW && r.endpoint_after >= E))
      return set_error(PM_ERANGE, "discovery row: endpoint id out of range");
  }
  for (uint32_t w = 0; w < W; ++w)
    if (row_endpoint[w] != PM_EP_NONE && row_endpoint[w] >= E) return set_error(PM_ERANGE, "endpoint column: id out of range");
  if (e->disc.h_seen.size() != W || e->disc.epoch == 0xFFFFFFFFu) {  // (a stamp of an earlier table, or of 2^32 calls ago)
    e->disc.h_seen.assign(W, 0u);
    e->disc.epoch = 0;
  }
  const uint32_t epoch = ++e->disc.epoch;
  for (uint32_t j = 0; j < D; ++j) {
    if (rows[j].row == PM_DISC_NEW) continue;
    if (e->disc.h_seen[rows[j].row] == epoch) return set_error(PM_EINVAL, "a table row listed twice");
    e->disc.h_seen[rows[j].row] = epoch;
  }
  HIPCHK(hipSetDevice(e->cfg.device));
  if ((rc = liveness_prepare(e))) return rc;
  if (n_updates_total) *n_updates_total = 0;
  if (!D) return PM_OK;

  static_assert(sizeof(pm_disc_row) == 32 && sizeof(pm_disc_result) == 16, "the layouts the kernels read and write");
  const size_t row_words = size_t(D) * 4, col_words = (size_t(W) + 1) / 2;  // (u64 words)
  std::vector<uint64_t>& in = e->disc.h_in;
  in.resize(row_words + col_words);
  std::memcpy(in.data(), rows, size_t(D) * sizeof(pm_disc_row));
  if (W) std::memcpy(in.data() + row_words, row_endpoint, size_t(W) * sizeof(uint32_t));
  const size_t zeroed = 3 * size_t(E) + 1;
  HIPCHK(e->disc.in.ensure(in.size()));
  HIPCHK(e->disc.work.ensure(size_t(W) + zeroed + E));
  HIPCHK(e->disc.events.ensure(2 * size_t(D)));
  HIPCHK(e->disc.out.ensure(D));
  HIPCHK(hipMemcpyAsync(e->disc.in.p, in.data(), in.size() * sizeof(uint64_t), hipMemcpyHostToDevice, e->stream));
  uint32_t* const work = e->disc.work.p;
  if (W) HIPCHK(hipMemsetAsync(work, 0xFF, size_t(W) * sizeof(uint32_t), e->stream));  // (PM_DISC_NEW: unlisted)
  HIPCHK(hipMemsetAsync(work + W, 0, zeroed * sizeof(uint32_t), e->stream));
  DiscArgs a{};
  a.W = W;
  a.D = D;
  a.E = E;
  a.max_same = max_healthy_same_endpoint;
  a.now_ms = now_ms;
  a.rows = reinterpret_cast<const pm_disc_row*>(e->disc.in.p);
  a.row_endpoint = reinterpret_cast<const uint32_t*>(e->disc.in.p + row_words);
  a.status = e->live.status.p;
  a.pos_of_row = work;
  a.base = work + W;
  a.ev_cnt = a.base + E;
  a.ev_fill = a.ev_cnt + E;
  a.cursor = a.ev_fill + E;
  a.ev_off = a.cursor + 1;
  a.events = e->disc.events.p;
  a.out = e->disc.out.p;
  launch_discovery_sync(a, e->stream);
  HIPCHK(hipGetLastError());
  e->disc.h_out.resize(D);
  HIPCHK(hipMemcpyAsync(e->disc.h_out.data(), e->disc.out.p, size_t(D) * sizeof(pm_disc_result), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  const std::vector<pm_disc_result>& res = e->disc.h_out;
  if (out) std::copy(res.begin(), res.end(), out);
  size_t total = 0;
  for (uint32_t j = 0; j < D; ++j) {
    if (res[j].n_updates > 3u) return set_error(PM_ESTATE, "discovery: a row with more than three updates");
    total += res[j].n_updates;
  }
  if (n_updates_total) *n_updates_total = uint32_t(total);
  if (!apply || !total) return PM_OK;
  // every update in discovery order through pm_on_worker_status_many's body (status_update_impl.rs:8-39), still under the
  // engine mutex; a row that a put-back left Healthy behind an update says so last
  std::vector<uint32_t> workers, flags_new, dead;
  workers.reserve(total);
  flags_new.reserve(total);
  dead.reserve(total);
  for (uint32_t j = 0; j < D; ++j) {
    const pm_disc_result& r = res[j];
    if (!r.n_updates) continue;
    const uint32_t w = rows[j].row;
    for (uint32_t u = 0; u < r.n_updates; ++u) {
      workers.push_back(w);
      flags_new.push_back(e->h_flags[w] & ~uint32_t(PM_W_HEALTHY));
      dead.push_back(r.upd_new[u] == PM_NS_DEAD || r.upd_new[u] == PM_NS_LOWBALANCE ? 1u : 0u);
    }
    if (r.final_status == PM_NS_HEALTHY) {
      workers.push_back(w);
      flags_new.push_back(e->h_flags[w] | PM_W_HEALTHY);
      dead.push_back(0u);
    }
  }
  return worker_status_many_locked(e, workers.data(), flags_new.data(), dead.data(), uint32_t(workers.size()));
}

}  // extern "C"
