// pm_engine_probe.inc — part of pm_engine.cpp (one translation unit; included in place): C ABI: pm_probe_configs and
// pm_config_overlap (kernel in pm_probe.inc) (inside extern "C").
//
// Both calls keep the promises of pm_engine_report.inc: they answer from the state every earlier call left (the host's flags
// column and group_of, pending changes included, through the reports' scratch uploads), consume no pending delta, compact
// nothing, clear no flag of the tick, leave the installed tables and compat_dirty alone, and write scratch of their own
// (d_probe_*).  The probes' tables go up in one packed copy, one launch, one packed copy back, one synchronisation.

// the sweep both calls share: `a` holds both table views; counters (and the masks, when wanted) come back in e->h_probe_out:
// [W u64 masks, if want_mask][P x PRB_STRIDE u32][P x C u32]
static int32_t probe_run(pm_engine* e, ProbeArgs& a, bool want_mask, const uint32_t** cnt, const uint64_t** mask) {
  const uint32_t P = a.p.n_cfgs, C = a.c.n_cfgs;
  a.group_of = e->d_group_of.p;
  if (e->groups_dirty && e->W) {  // (dissolutions and new rows the device has not seen yet)
    int32_t rc = upload(e->d_rep_gof, e->h_group_of.data(), e->W, e->stream);
    if (rc) return rc;
    a.group_of = e->d_rep_gof.p;
  }
  a.enabled = e->enabled;
  const size_t n_mask = want_mask ? e->W : 0u, n_cnt = size_t(P) * PRB_STRIDE + size_t(P) * C;
  const size_t words = n_mask + (n_cnt + 1u) / 2u;
  HIPCHK(e->d_probe_out.ensure(words));
  a.mask_out = n_mask ? e->d_probe_out.p : nullptr;
  a.out = reinterpret_cast<uint32_t*>(e->d_probe_out.p + n_mask);
  HIPCHK(hipMemsetAsync(a.out, 0, n_cnt * 4u, e->stream));
  launch_probe(a, 4u * e->n_cus, e->stream);
  HIPCHK(hipGetLastError());
  e->h_probe_out.resize(words);
  HIPCHK(hipMemcpyAsync(e->h_probe_out.data(), e->d_probe_out.p, words * 8u, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));  // (the pageable sources of the uploads die here too)
  *mask = e->h_probe_out.data();
  *cnt = reinterpret_cast<const uint32_t*>(e->h_probe_out.data() + n_mask);
  return PM_OK;
}

int32_t pm_probe_configs(pm_engine* e, const pm_config_row* probes, uint32_t n_probes, const pm_gpu_alt_row* alts,
                         uint32_t n_alts, const uint32_t* model_bits, uint32_t n_model_rows, uint32_t n_classes,
                         pm_probe_row* rows, uint32_t* overlap, uint64_t* mask_out) {
  if (!e || (n_probes && (!probes || !rows)) || (n_alts && !alts)) return set_error(PM_EINVAL, "null argument");
  if (n_probes > PM_MAX_CONFIGS) return set_error(PM_EINVAL, "more than PM_MAX_CONFIGS probes");
  const size_t model_words = (size_t(n_classes) + 31u) / 32u;
  if (n_model_rows && model_words && !model_bits) return set_error(PM_EINVAL, "null argument");
  bool model_alt = false;
  for (uint32_t i = 0; i < n_probes; ++i) {  // (the rules of pm_set_configs)
    if (probes[i].max_group_size < probes[i].min_group_size)
      return set_error(PM_EINVAL, "probe is invalid (max_group_size < min_group_size)");
    if (probes[i].min_group_size == 0) return set_error(PM_EINVAL, "min_group_size == 0 is rejected");
    if (uint64_t(probes[i].alt_begin) + probes[i].alt_count > n_alts)
      return set_error(PM_ERANGE, "alternative range outside the alt table");
  }
  for (uint32_t k = 0; k < n_alts; ++k) {
    if (!(alts[k].flags & PM_G_MODEL)) continue;
    model_alt = true;
    if (n_classes == 0) return set_error(PM_EINVAL, "a GPU alternative names a model row but n_classes is 0");
    if (alts[k].model_row >= n_model_rows) return set_error(PM_EINVAL, "a GPU alternative names a model row outside the table");
  }
  std::lock_guard<std::mutex> lk(e->mu);
  int32_t rc = report_begin(e, false);
  if (rc) return rc;
  if (!n_probes) return PM_OK;
  if (n_classes != e->model_classes)
    return set_error(PM_EINVAL, "n_classes differs from the engine's class count (a table built before a model was interned?)");
  if (model_alt && !e->model_rows)  // (report_begin checks the column only against an installed table with rows)
    for (uint32_t w = 0; w < e->W; ++w)
      if ((e->h_flags[w] & PM_W_GPU_MODEL) && e->h_gpu_cls[w] >= n_classes)
        return set_error(PM_ERANGE, "worker gpu_model_class outside the model table");
  ProbeArgs a{};
  if ((rc = report_compat_args(e, &a.c))) return rc;
  // [probe rows][alternatives][model bits], in u32 words (both row types are 32 bytes)
  const size_t o_alt = size_t(n_probes) * 8u, o_bits = o_alt + size_t(n_alts) * 8u;
  const size_t n_bits = model_alt ? size_t(n_model_rows) * model_words : 0u;
  e->h_probe_in.resize(o_bits + n_bits);
  std::memcpy(e->h_probe_in.data(), probes, size_t(n_probes) * sizeof(pm_config_row));
  if (n_alts) std::memcpy(e->h_probe_in.data() + o_alt, alts, size_t(n_alts) * sizeof(pm_gpu_alt_row));
  if (n_bits) std::memcpy(e->h_probe_in.data() + o_bits, model_bits, n_bits * 4u);
  if ((rc = upload(e->d_probe_in, e->h_probe_in.data(), e->h_probe_in.size(), e->stream))) return rc;
  a.p = a.c;
  a.p.n_cfgs = n_probes;
  a.p.model_words = uint32_t(model_words);
  a.p.cfgs = reinterpret_cast<const pm_config_row*>(e->d_probe_in.p);
  a.p.alts = reinterpret_cast<const pm_gpu_alt_row*>(e->d_probe_in.p + o_alt);
  a.p.model_bits = e->d_probe_in.p + o_bits;
  const uint32_t* cnt;
  const uint64_t* mask;
  if ((rc = probe_run(e, a, mask_out != nullptr, &cnt, &mask))) return rc;
  const uint32_t C = a.c.n_cfgs;
  for (uint32_t p = 0; p < n_probes; ++p) {
    const uint32_t* k = cnt + size_t(p) * PRB_STRIDE;
    pm_probe_row& r = rows[p];
    for (uint32_t j = 0; j < PM_WHY_N; ++j) r.why[j] = k[PRB_WHY + j];
    r.eligible_meets = k[PRB_WHY + PM_WHY_OK];
    r.idle_meets = k[PRB_IDLE];
    r.idle_located = k[PRB_LOCATED];
    r.idle_exclusive = k[PRB_EXCL];
    r.groups_max = r.idle_meets / probes[p].min_group_size;
    r.groups_exclusive = r.idle_exclusive / probes[p].min_group_size;
  }
  if (overlap && C) std::memcpy(overlap, cnt + size_t(n_probes) * PRB_STRIDE, size_t(n_probes) * C * 4u);
  if (mask_out && e->W) std::memcpy(mask_out, mask, size_t(e->W) * 8u);
  return PM_OK;
}

int32_t pm_config_overlap(pm_engine* e, uint32_t* overlap, uint32_t cap, uint32_t* n_cfgs) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  int32_t rc = report_begin(e, false);
  if (rc) return rc;
  const uint32_t C = uint32_t(e->cfgs.size());
  if (n_cfgs) *n_cfgs = C;
  if (cap < C * C || (C && !overlap)) return set_error(PM_ERANGE, "overlap buffer too small");
  if (!C) return PM_OK;
  ProbeArgs a{};
  if ((rc = report_compat_args(e, &a.c))) return rc;
  a.p = a.c;  // the installed table on both sides
  const uint32_t* cnt;
  const uint64_t* mask;
  if ((rc = probe_run(e, a, false, &cnt, &mask))) return rc;
  std::memcpy(overlap, cnt + size_t(C) * PRB_STRIDE, size_t(C) * C * 4u);
  return PM_OK;
}
