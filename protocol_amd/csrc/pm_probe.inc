// pm_probe.inc — the probe kernel (included by pm_kernels.hip inside namespace pm): pm_probe_configs and pm_config_overlap of
// include/pm_engine.h, with its launcher.  Read-only: it reads the worker columns, the host-truth group_of, the installed
// configuration tables and the probes' own tables, and writes the call's own output scratch alone.
//
// One launch.  Every wave takes 64 worker rows per step, grid-stride, a worker per lane.  The rows of both configuration
// tables are wave-uniform (scalar loads), as in config_report_kernel; the probes come as a second CompatArgs view (their own
// rows, alternatives and model bits over the same worker columns), so that the clause code is why_code, not a restatement.
//
//   reason histograms   one ballot per distinct code in the wave (config_report_kernel's scheme)
//   the P x C matrix    not P x C ballots: the step's idle lanes are transposed once — lane c keeps the ballot of "idle and
//                       meets installed c" — and for every probe p the wave-uniform ballot of "idle and meets p" is ANDed
//                       with it and popcounted in every lane: one LDS add per (p, lane c) with a non-zero count
//   counters            in LDS (PRB_STRIDE words a probe + P x C words: 20 KiB at 64 x 64, eight workgroups a CU), added
//                       with LDS atomics; each non-zero one goes to global memory once per workgroup.  All of them are u32
//                       sums: the result does not depend on the order.
//   mask_out            a plain coalesced store of every row's probe bits, whatever the row's state

__global__ __launch_bounds__(256) void probe_kernel(ProbeArgs a) {
  __shared__ uint32_t s_cnt[PM_MAX_CONFIGS * PRB_STRIDE + PM_MAX_CONFIGS * PM_MAX_CONFIGS];
  const uint32_t P = a.p.n_cfgs, C = a.c.n_cfgs, W = a.c.W, lane = threadIdx.x & 63u;
  const uint32_t n_cnt = P * PRB_STRIDE + P * C;  // (the matrix is counted into LDS whether it is asked for or not)
  uint32_t* const s_ov = s_cnt + P * PRB_STRIDE;
  for (uint32_t k = threadIdx.x; k < n_cnt; k += 256u) s_cnt[k] = 0u;
  __syncthreads();
  for (uint32_t base = blockIdx.x * 256u + (threadIdx.x & ~63u); base < W; base += gridDim.x * 256u) {
    const uint32_t w = base + lane;
    const bool in = w < W;
    const WhyRow r = why_row(a.c, in ? w : 0u);
    const bool elig = in && (r.wf & PM_W_HEALTHY) && (r.wf & PM_W_HAS_P2P);
    const bool idle = elig && a.group_of[w] < 0;
    const uint64_t any_elig = __ballot(elig), any_idle = __ballot(idle);
    if (!any_elig && !a.mask_out) continue;  // (wave-uniform)
    // ---- installed side, for the idle lanes: the bits, then the transpose (lane c: who is idle and meets c)
    uint64_t cbits = 0ull, tc = 0ull;
    if (any_idle) {
      for (uint32_t c = 0; c < C; ++c) {
        const bool ok = idle && why_code(r, a.c.cfgs[c], a.c) == PM_WHY_OK;
        const uint64_t m = __ballot(ok);
        cbits |= (uint64_t)ok << c;
        if (lane == c) tc = m;
      }
    }
    const bool excl_lane = (cbits & a.enabled) == 0ull;
    // ---- probe side
    uint64_t pbits = 0ull;
    for (uint32_t p = 0; p < P; ++p) {
      const uint32_t code = in ? why_code(r, a.p.cfgs[p], a.p) : PM_WHY_N;
      const bool ok = code == PM_WHY_OK;
      pbits |= (uint64_t)ok << p;
      uint32_t* const row = s_cnt + p * PRB_STRIDE;
      uint64_t left = any_elig;
      while (left) {  // (wave-uniform)
        const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)code, (int)__builtin_ctzll(left));
        const uint64_t m = __ballot(elig && code == k);
        if (lane == 0u) atomicAdd(&row[PRB_WHY + k], (uint32_t)__popcll(m));
        left &= ~m;
      }
      const uint64_t mi = __ballot(idle && ok);
      if (!mi) continue;
      const uint64_t ml = __ballot(idle && ok && (r.wf & PM_W_HAS_LOC)), mx = __ballot(idle && ok && excl_lane);
      if (lane == 0u) {
        atomicAdd(&row[PRB_IDLE], (uint32_t)__popcll(mi));
        if (ml) atomicAdd(&row[PRB_LOCATED], (uint32_t)__popcll(ml));
        if (mx) atomicAdd(&row[PRB_EXCL], (uint32_t)__popcll(mx));
      }
      const uint32_t both = (uint32_t)__popcll(mi & tc);  // (lanes >= C hold tc == 0)
      if (both) atomicAdd(&s_ov[p * C + lane], both);
    }
    if (a.mask_out && in) a.mask_out[w] = pbits;
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < n_cnt; k += 256u)
    if (s_cnt[k]) atomicAdd(&a.out[k], s_cnt[k]);
}

void launch_probe(const ProbeArgs& a, uint32_t max_blocks, hipStream_t s) {
  if (a.p.n_cfgs == 0) return;
  hipLaunchKernelGGL(probe_kernel, dim3(report_blocks(a.c.W, max_blocks)), dim3(256), 0, s, a);
}
