// pm_engine_spread.inc — part of pm_engine.cpp (one translation unit; included in place): C ABI: the group geography
// reports (pm_group_spread, pm_config_spread; kernels in pm_spread.inc) and pm_force_regroup (inside extern "C").
//
// The two reports keep the promises of pm_engine_report.inc: they answer from the state every earlier call left (the
// host's flags column and group list, pending changes included), consume no pending delta, compact nothing, clear no flag
// of the tick, and write scratch of their own (d_spr_*, and d_rep_flags for a flags column that has not gone up yet).

// Per-group rows into d_spr_rows, one per live group in list order (= the order pm_get_groups gives).  While the device
// mirror holds the host list slot for slot (see report_groups) sizes, offsets and members are read in place and the row ->
// slot list skips the tombstones; otherwise the live groups' sizes, offsets and members go up to scratch.  `cfg_too`: the
// configuration of every row behind the lists (config_spread_kernel).  *row_cfg = where that column starts.
static int32_t spread_run(pm_engine* e, bool cfg_too, const uint32_t** row_cfg) {
  const size_t G = e->groups.size(), L = G - e->n_dead_groups;
  if (row_cfg) *row_cfg = nullptr;
  if (!L) return PM_OK;
  const bool mirror = (!e->groups_dirty || e->groups_delta_ok) && e->d_n_groups == G && e->d_g_n.p && e->d_g_off.p &&
                      e->d_members.p;
  size_t M = 0;
  if (!mirror)
    for (const Group& gr : e->groups) M += gr.dead ? 0 : gr.members.size();
  // [slot_of_row L][small + big L][cfg L]?[n L, off L, members M]?
  const size_t o_list = L, o_cfg = 2 * L, o_n = o_cfg + (cfg_too ? L : 0), o_off = o_n + L, o_mem = o_off + L;
  std::vector<uint32_t> idx(mirror ? o_n : o_mem + M);
  uint32_t n_small = 0, n_big = 0, k = 0, off = 0;
  for (size_t g = 0; g < G; ++g) {
    const Group& gr = e->groups[g];
    if (gr.dead) continue;
    const uint32_t n = uint32_t(gr.members.size());
    idx[k] = mirror ? uint32_t(g) : k;
    if (n <= 64u) idx[o_list + n_small++] = k;
    else idx[o_list + L - ++n_big] = k;  // (the large groups from the back of the same L words)
    if (cfg_too) idx[o_cfg + k] = gr.cfg;
    if (!mirror) {
      idx[o_n + k] = n, idx[o_off + k] = off;
      std::copy(gr.members.begin(), gr.members.end(), idx.begin() + ptrdiff_t(o_mem + off));
      off += n;
    }
    ++k;
  }
  int32_t rc = upload(e->d_spr_idx, idx.data(), idx.size(), e->stream);
  if (rc) return rc;
  SpreadArgs a{};
  a.slot_of_row = e->d_spr_idx.p;
  a.small = e->d_spr_idx.p + o_list, a.n_small = n_small;
  a.big = e->d_spr_idx.p + o_list + L - n_big, a.n_big = n_big;
  if (mirror) a.g_n = e->d_g_n.p, a.g_off = e->d_g_off.p, a.members = e->d_members.p;
  else a.g_n = e->d_spr_idx.p + o_n, a.g_off = e->d_spr_idx.p + o_off, a.members = e->d_spr_idx.p + o_mem;
  a.W = e->W;
  a.flags = e->d_flags.p;
  if (e->flags_dirty && e->W) {
    if ((rc = upload(e->d_rep_flags, e->h_flags.data(), e->W, e->stream))) return rc;
    a.flags = e->d_rep_flags.p;
  }
  a.addr_rank = e->d_addr_rank.p;
  a.lat = e->d_lat.p, a.lon = e->d_lon.p, a.coslat = e->d_coslat.p;
  HIPCHK(e->d_spr_rows.ensure(L));
  a.out = e->d_spr_rows.p;
  launch_group_spread(a, e->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(e->stream));  // (pageable sources die here)
  if (row_cfg && cfg_too) *row_cfg = e->d_spr_idx.p + o_cfg;
  return PM_OK;
}

int32_t pm_group_spread(pm_engine* e, pm_group_spread_row* out, uint32_t cap, uint32_t* n_groups) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  int32_t rc = report_begin(e, false);
  if (rc) return rc;
  const uint32_t L = uint32_t(e->groups.size() - e->n_dead_groups);
  if (n_groups) *n_groups = L;
  if (cap < L || (L && !out)) return set_error(PM_ERANGE, "spread buffer too small");
  if (!L) return PM_OK;
  if ((rc = spread_run(e, false, nullptr))) return rc;
  HIPCHK(hipMemcpyAsync(out, e->d_spr_rows.p, size_t(L) * sizeof(pm_group_spread_row), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return PM_OK;
}

int32_t pm_config_spread(pm_engine* e, pm_config_spread_row* out, uint32_t cap, uint32_t* n_cfgs) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  int32_t rc = report_begin(e, false);
  if (rc) return rc;
  const uint32_t C = uint32_t(e->cfgs.size()), L = uint32_t(e->groups.size() - e->n_dead_groups);
  if (n_cfgs) *n_cfgs = C;
  if (cap < C || (C && !out)) return set_error(PM_ERANGE, "report buffer too small");
  if (!C) return PM_OK;
  std::vector<SpreadCfgAcc> acc(C);
  if (L) {
    const uint32_t* row_cfg = nullptr;
    if ((rc = spread_run(e, true, &row_cfg))) return rc;
    HIPCHK(e->d_spr_acc.ensure(C));
    HIPCHK(hipMemsetAsync(e->d_spr_acc.p, 0, size_t(C) * sizeof(SpreadCfgAcc), e->stream));
    launch_config_spread(e->d_spr_rows.p, row_cfg, L, C, e->d_spr_acc.p, 4u * e->n_cus, e->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(acc.data(), e->d_spr_acc.p, size_t(C) * sizeof(SpreadCfgAcc), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  for (uint32_t c = 0; c < C; ++c) {
    pm_config_spread_row& r = out[c];
    std::memset(&r, 0, sizeof(r));
    r.groups = acc[c].cnt[SPC_GROUPS];
    r.measured = acc[c].cnt[SPC_MEASURED];
    for (uint32_t j = 0; j < PM_SPREAD_BUCKETS; ++j) r.hist[j] = acc[c].cnt[SPC_HIST + j];
    std::memcpy(&r.max_diameter_km, &acc[c].v[SPV_MAX_DIAMETER], 8);  // (bit patterns of non-negative doubles)
    std::memcpy(&r.max_hop_km, &acc[c].v[SPV_MAX_HOP], 8);
    r.sum_diameter_m = acc[c].v[SPV_SUM_DIAMETER];
    r.sum_ring_m = acc[c].v[SPV_SUM_RING];
  }
  return PM_OK;
}

// "{:x}" of a group id, as get_all_groups sorts them (mod.rs:1040): compared as text, so "10" < "9"
static std::string group_id_hex(uint64_t id) {
  char buf[17];
  std::snprintf(buf, sizeof buf, "%llx", (unsigned long long)id);
  return buf;
}

int32_t pm_force_regroup(pm_engine* e, uint32_t config, uint32_t metric, double threshold_km, uint32_t* dissolved_groups,
                         uint32_t* affected_workers) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  int32_t rc = report_begin(e, false);
  if (rc) return rc;
  if (dissolved_groups) *dissolved_groups = 0;
  if (affected_workers) *affected_workers = 0;
  if (config >= e->cfgs.size()) return set_error(PM_ERANGE, "configuration index out of range");
  if (metric > PM_REGROUP_LONGEST_HOP) return set_error(PM_EINVAL, "unknown regroup metric");
  if (metric != PM_REGROUP_ALL && !(threshold_km >= 0.0)) return set_error(PM_EINVAL, "threshold_km must be a number >= 0");
  const size_t L = e->groups.size() - e->n_dead_groups;
  std::vector<pm_group_spread_row> rows;
  if (metric != PM_REGROUP_ALL && L) {
    if ((rc = spread_run(e, false, nullptr))) return rc;
    rows.resize(L);
    HIPCHK(hipMemcpyAsync(rows.data(), e->d_spr_rows.p, L * sizeof(pm_group_spread_row), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  std::vector<std::pair<std::string, uint32_t>> sel;  // (id text, slot)
  size_t k = 0;
  for (size_t g = 0; g < e->groups.size(); ++g) {
    const Group& gr = e->groups[g];
    if (gr.dead) continue;
    const size_t row = k++;
    if (gr.cfg != config) continue;
    if (metric == PM_REGROUP_DIAMETER && !(rows[row].located >= 2u && rows[row].diameter_km >= threshold_km)) continue;
    if (metric == PM_REGROUP_LONGEST_HOP && !(rows[row].ring_hops >= 1u && rows[row].longest_hop_km >= threshold_km)) continue;
    sel.emplace_back(group_id_hex(gr.id), uint32_t(g));
  }
  if (sel.empty()) return PM_OK;
  std::sort(sel.begin(), sel.end());
  // each as pm_dissolve_group_by_id: the feed entry in this order, the members free at once; the published rows are
  // patched and the list compacted once for all of them (what the calls one by one would leave behind)
  std::vector<uint32_t> freed;
  for (const auto& s : sel) {
    freed.insert(freed.end(), e->groups[s.second].members.begin(), e->groups[s.second].members.end());
    dissolve_locked(e, s.second);
  }
  pub_patch(e, &freed);
  compact_groups(e);
  if (dissolved_groups) *dissolved_groups = uint32_t(sel.size());
  if (affected_workers) *affected_workers = uint32_t(freed.size());
  return PM_OK;
}
