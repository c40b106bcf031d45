// pm_taskdir.inc — the task directory's kernels (included by pm_kernels.hip inside namespace pm, behind pm_groupdir.inc):
// pm_task_directory of include/pm_engine.h, with their launchers.  They read the task index space, the host's groups and what
// the rollout ledger's reads left behind, and write scratch of their own: a pure read.  Integers only: every result is a count
// or a copy, so nothing depends on the grid or on which wave meets which row.  A SLOT r is handle t_lo + r (pm_device.h).
//
// GROUPS.  One pass over the list, tombstones included: a live group adds one to the live groups of its configuration (LDS, one
// global atomic a non-zero bin and workgroup) and, where the row it holds is live, one to the slot's TD_RUNNING, its size to
// TD_WORKERS and — its every member converged, the rollout ledger's own counter against its size, ro_emit_kernel's rule — one to
// TD_HOLD_CONV.  This is task_report_groups_kernel's job with the converged groups beside it.  The lanes of a wave that hit one
// word send one atomic (wave_add_words); the sizes go as they are.  Integer sums: the same whatever order the atomics land in.
//
// JOIN (rollout on).  The rollout ledger's per-task table is one row a reported id.  The live (id, slot) pairs stand sorted by
// id, equal ids in slot order (eight stable passes from ascending slots): a lower-bound search finds the FIRST live row that
// carries the id, the header's rule for duplicates, with nothing written for it.  One thread a run copies the run's reported
// columns to that slot — no two runs share an id, so no two threads share a slot — or counts an orphan.
//
// TASKS.  One pass over the slots behind both: groups_allowed from the per-configuration counts in LDS (task_report_tasks_kernel's
// sum), the two classes, the filter, the census — per configuration and class by ballots, the sums by wave reductions, one
// global atomic a non-zero bin and workgroup — and the listing flag.  ONE exclusive scan over the flags gives every listed slot
// its place in list order.
//
// ORDER.  BY_LIST: the scan is the order.  BY_OLDEST: place total - 1 - scan (list_place; list_window_kernel of pm_directory.inc).  The _DESC orders: the listed slots compacted in
// list order, four stable radix passes over UINT32_MAX - value (launch_ro_radix_pass: ties keep list order).
//
// EMIT.  One thread per window slot: the position from the live prefix, the columns, the classes, one 88-byte row written whole.

__device__ __forceinline__ bool tdir_live(const TdirArgs& a, uint32_t u) { return (a.tlive[u >> 6] >> (u & 63u)) & 1ull; }

__global__ __launch_bounds__(256) void tdir_group_kernel(TdirArgs a) {
  __shared__ uint32_t s_g[PM_MAX_CONFIGS];
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  if (tid < PM_MAX_CONFIGS) s_g[tid] = 0u;
  __syncthreads();
  const uint32_t k = blockIdx.x * 256u + tid;
  uint32_t w_run = PM_NONE, w_conv = PM_NONE;  // (PM_NONE: this lane counts nothing)
  if (k < a.G) {
    const TdirGroup gr = a.g[k];
    if (gr.live && gr.cfg < a.n_cfgs) {
      atomicAdd(&s_g[gr.cfg], 1u);
      const uint32_t u = gr.handle;
      if (u != PM_NONE && u >= a.t_lo && u < a.t_cap && tdir_live(a, u)) {
        const uint32_t base = (u - a.t_lo) * PM_TD_CNT;
        w_run = base + TD_RUNNING;
        if (gr.size) atomicAdd(&a.cnt[base + TD_WORKERS], gr.size);
        if (a.ro_gcnt && a.ro_gcnt[(size_t)k * PM_RO_GCNT + PM_TS_RUNNING] == gr.size) w_conv = base + TD_HOLD_CONV;
      }
    }
  }
  wave_add_words(a.cnt, w_run, lane);
  wave_add_words(a.cnt, w_conv, lane);
  __syncthreads();
  if (tid < PM_MAX_CONFIGS && s_g[tid]) atomicAdd(&a.g_per_cfg[tid], s_g[tid]);
}

__global__ __launch_bounds__(256) void tdir_join_kernel(TdirArgs a, const pm_ro_task_row* __restrict__ runs, uint32_t D,
                                                        const uint64_t* __restrict__ key, const uint32_t* __restrict__ val,
                                                        uint32_t n_pairs) {
  const uint32_t d = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
  uint32_t orphan_rep = 0u;
  bool orphan = false;
  if (d < D) {
    const pm_ro_task_row r = runs[d];
    uint32_t lo = 0u, hi = n_pairs;  // the first pair whose id is not below the run's
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (key[mid] < r.uid) lo = mid + 1u; else hi = mid;
    }
    uint32_t rep = 0u;
#pragma unroll
    for (uint32_t s = 0; s < PM_TS_N; ++s) rep += r.reporters[s];
    if (r.uid != ~0ull && lo < n_pairs && key[lo] == r.uid) {  // (an id of all ones names no task)
      uint32_t* c = a.cnt + (size_t)val[lo] * PM_TD_CNT;
      c[TD_G_CONV] = r.groups_converged;
      c[TD_CONV] = r.converged;
#pragma unroll
      for (uint32_t s = 0; s < PM_TS_N; ++s) c[TD_REP + s] = r.reporters[s];
    } else {
      orphan = true;
      orphan_rep = rep;
    }
  }
  const uint64_t m = __ballot(orphan);
#pragma unroll
  for (uint32_t x = 32u; x; x >>= 1) orphan_rep += (uint32_t)__shfl_xor((int)orphan_rep, (int)x);
  if (lane == 0u && m) {
    atomicAdd(&a.census[TD_C_ORPHAN_UIDS], (uint32_t)__popcll(m));
    if (orphan_rep) atomicAdd(&a.census[TD_C_ORPHAN_REPORTERS], orphan_rep);
  }
}

__global__ __launch_bounds__(256) void tdir_task_kernel(TdirArgs a) {
  __shared__ uint32_t s_g[PM_MAX_CONFIGS];
  __shared__ uint32_t s_bin[PM_TD_CENSUS];
  __shared__ uint32_t s_all;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, C = a.n_cfgs;
  if (tid < PM_MAX_CONFIGS) s_g[tid] = tid < C ? a.g_per_cfg[tid] : 0u;
  if (tid < PM_TD_CENSUS) s_bin[tid] = 0u;
  __syncthreads();
  if (tid == 0u) {
    uint32_t t = 0;
    for (uint32_t c = 0; c < C; ++c) t += s_g[c];
    s_all = t;
  }
  __syncthreads();
  const uint64_t valid = C >= 64u ? ~0ull : (1ull << C) - 1ull;
  const uint32_t R = a.t_cap - a.t_lo, r = blockIdx.x * 256u + tid;
  uint32_t s_bin_of = PM_NONE, r_bin_of = PM_NONE, workers = 0u, reporters = 0u;  // (PM_NONE: this lane counts nothing)
  uint64_t m_pass = 0ull;
  bool unrestricted = false;
  if (r < R) {
    const uint32_t u = a.t_lo + r;
    bool pass = false;
    uint32_t serve = PM_TKS_STARVED, rollout = PM_TKR_NONE;
    if (tdir_live(a, u)) {
      const uint64_t mask = a.tmask[u], m = mask & valid;
      uint32_t* c = a.cnt + (size_t)r * PM_TD_CNT;
      uint32_t allowed = 0u;
      if (m == valid) {
        allowed = s_all;  // (unrestricted tasks: every configuration)
      } else {
        for (uint64_t b = m; b; b &= b - 1ull) allowed += s_g[__builtin_ctzll(b)];
      }
      c[TD_ALLOWED] = allowed;
      const uint32_t running = c[TD_RUNNING], w = c[TD_WORKERS];
      uint32_t rep = 0u;
#pragma unroll
      for (uint32_t s = 0; s < PM_TS_N; ++s) rep += c[TD_REP + s];
      serve = running ? (uint32_t)PM_TKS_RUNNING : allowed ? (uint32_t)PM_TKS_WAITING : (uint32_t)PM_TKS_STARVED;
      if (a.rollout_on)
        rollout = !running ? (uint32_t)PM_TKR_UNHELD
                : c[TD_HOLD_CONV] == running ? (uint32_t)PM_TKR_CONVERGED : (uint32_t)PM_TKR_ROLLING;
      pass = a.config_mask == ~0ull || (m & a.config_mask) != 0ull;
      pass = pass && ((a.serve_mask >> serve) & 1u) != 0u;
      pass = pass && (!a.rollout_on || ((a.rollout_mask >> rollout) & 1u) != 0u);
      pass = pass && w >= a.workers_min && w <= a.workers_max;
      if (pass) {
        m_pass = m;
        s_bin_of = serve;
        if (a.rollout_on) r_bin_of = rollout;
        unrestricted = mask == ~0ull;
        workers = w;
        reporters = rep;
      }
    }
    a.cls[2u * r] = (uint8_t)serve;
    a.cls[2u * r + 1u] = (uint8_t)rollout;
    a.flag[r] = pass ? 1u : 0u;
  }
  if (__ballot(m_pass != 0ull)) {  // (wave-uniform)
    for (uint32_t c = 0; c < C; ++c) {
      const uint64_t b = __ballot((m_pass >> c) & 1ull);
      if (lane == 0u && b) atomicAdd(&s_bin[c], (uint32_t)__popcll(b));
    }
  }
  for (uint32_t k = 0; k < PM_TKS_N; ++k) {
    const uint64_t b = __ballot(s_bin_of == k);
    if (lane == 0u && b) atomicAdd(&s_bin[TD_C_SERVE + k], (uint32_t)__popcll(b));
  }
  for (uint32_t k = 0; k < PM_TKR_N; ++k) {
    const uint64_t b = __ballot(r_bin_of == k);
    if (lane == 0u && b) atomicAdd(&s_bin[TD_C_ROLLOUT + k], (uint32_t)__popcll(b));
  }
  const uint64_t bu = __ballot(unrestricted);
  if (lane == 0u && bu) atomicAdd(&s_bin[TD_C_UNRESTRICTED], (uint32_t)__popcll(bu));
#pragma unroll
  for (uint32_t x = 32u; x; x >>= 1) {
    workers += (uint32_t)__shfl_xor((int)workers, (int)x);
    reporters += (uint32_t)__shfl_xor((int)reporters, (int)x);
  }
  if (lane == 0u && workers) atomicAdd(&s_bin[TD_C_WORKERS], workers);
  if (lane == 0u && reporters) atomicAdd(&s_bin[TD_C_REPORTERS], reporters);
  __syncthreads();
  if (tid < TD_C_ORPHAN_UIDS && s_bin[tid]) atomicAdd(&a.census[tid], s_bin[tid]);  // (the orphans are the join's)
}

__device__ __forceinline__ uint32_t list_place(const TdirArgs& a, uint32_t r) {
  if (r >= a.t_cap - a.t_lo || !a.flag[r]) return PM_NONE;
  return a.order == PM_TDIR_BY_OLDEST ? a.total - 1u - a.off[r] : a.off[r];
}

__global__ __launch_bounds__(256) void tdir_keys_kernel(TdirArgs a) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  const uint32_t at = list_place(a, r);
  if (at >= a.total) return;  // (PM_NONE too)
  const uint32_t* c = a.cnt + (size_t)r * PM_TD_CNT;
  uint32_t v = c[TD_WORKERS];
  if (a.order == PM_TDIR_BY_REPORTERS_DESC) {
    v = 0u;
#pragma unroll
    for (uint32_t s = 0; s < PM_TS_N; ++s) v += c[TD_REP + s];
  }
  a.key[at] = (uint64_t)(0xFFFFFFFFu - v);  // largest first
  a.val[at] = r;
}

__global__ __launch_bounds__(256) void tdir_emit_kernel(TdirArgs a, const uint32_t* __restrict__ list, uint32_t n,
                                                        pm_tdir_row* __restrict__ rows, uint32_t* __restrict__ handles) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  uint32_t r = list[i];
  if (r >= a.t_cap - a.t_lo) r = 0u;  // (never: the window's slots are slots)
  const uint32_t u = a.t_lo + r;
  const uint64_t w = a.tlive[u >> 6];
  const uint32_t* c = a.cnt + (size_t)r * PM_TD_CNT;
  pm_tdir_row o;
  o.uid = 0ull;  // (the host's, by the handle)
  o.created_at = a.created[u];
  o.topo_mask = a.tmask[u];
  o.task = a.tprefix[u >> 6] + (uint32_t)__popcll(w & ((1ull << (u & 63u)) - 1ull));
  o.groups_allowed = c[TD_ALLOWED];
  o.groups_running = c[TD_RUNNING];
  o.workers_running = c[TD_WORKERS];
  o.groups_converged = c[TD_G_CONV];
  o.converged = c[TD_CONV];
#pragma unroll
  for (uint32_t s = 0; s < PM_TS_N; ++s) o.reporters[s] = c[TD_REP + s];
  o.serve = a.cls[2u * r];
  o.rollout = a.cls[2u * r + 1u];
  o._pad = 0;
  o._pad2 = 0u;
  rows[i] = o;
  handles[i] = u;
}

void launch_tdir_groups(const TdirArgs& a, hipStream_t s) {
  if (!a.G) return;
  hipLaunchKernelGGL(tdir_group_kernel, dim3((a.G + 255u) / 256u), dim3(256), 0, s, a);
}

void launch_tdir_join(const TdirArgs& a, const pm_ro_task_row* runs, uint32_t D, const uint64_t* key, const uint32_t* val,
                      uint32_t n_pairs, hipStream_t s) {
  if (!D) return;
  hipLaunchKernelGGL(tdir_join_kernel, dim3((D + 255u) / 256u), dim3(256), 0, s, a, runs, D, key, val, n_pairs);
}

void launch_tdir_tasks(const TdirArgs& a, hipStream_t s) {
  if (a.t_cap <= a.t_lo) return;
  hipLaunchKernelGGL(tdir_task_kernel, dim3((a.t_cap - a.t_lo + 255u) / 256u), dim3(256), 0, s, a);
}

// (the template stands in pm_directory.inc, included in front of this file; it finds list_place above by its argument's type)
template void launch_list_window<TdirArgs>(const TdirArgs&, uint32_t, hipStream_t);

void launch_tdir_keys(const TdirArgs& a, hipStream_t s) {
  if (a.t_cap <= a.t_lo || !a.total) return;
  hipLaunchKernelGGL(tdir_keys_kernel, dim3((a.t_cap - a.t_lo + 255u) / 256u), dim3(256), 0, s, a);
}

void launch_tdir_emit(const TdirArgs& a, const uint32_t* list, uint32_t n, pm_tdir_row* rows, uint32_t* handles, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(tdir_emit_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, a, list, n, rows, handles);
}
