// pm_report.inc — the diagnostics kernels (included by pm_kernels.hip inside namespace pm): the reason code of a (worker,
// configuration) pair, and the three read-only reports of include/pm_engine.h (pm_explain_workers, pm_config_report,
// pm_task_report) with their launchers.  compat_body stays the hot path's own code; why_code restates it clause by clause
// and returns the first clause that fails instead of a bit (code == PM_WHY_OK <=> the compat bit).

// GpuSpecs::meets (shared/src/models/node.rs:445-526) for one alternative: its first failing clause
__device__ __forceinline__ uint32_t gpu_alt_why(uint32_t wf, uint32_t wcount, uint32_t wmem, uint32_t wcls,
                                                const pm_gpu_alt_row& a, const uint32_t* __restrict__ model_bits,
                                                uint32_t words) {
  if (a.flags & PM_G_COUNT) {  // :447-461
    if (!(wf & PM_W_GPU_COUNT)) {
      if (a.count > 0) return PM_WHY_GPU_COUNT;
    } else if (wcount != a.count) {
      return PM_WHY_GPU_COUNT;
    }
  }
  if (a.flags & PM_G_MODEL) {  // :463-484
    if (!(wf & PM_W_GPU_MODEL)) return PM_WHY_GPU_MODEL;
    const uint32_t word = model_bits[a.model_row * words + (wcls >> 5)];
    if (!((word >> (wcls & 31)) & 1u)) return PM_WHY_GPU_MODEL;
  }
  const bool mem_some = (wf & PM_W_GPU_MEM) != 0;  // :487-503
  if ((a.flags & PM_G_MEM) && (!mem_some || wmem < a.memory_mb)) return PM_WHY_GPU_MEM;
  if ((a.flags & PM_G_MEM_MIN) && (!mem_some || wmem < a.memory_mb_min)) return PM_WHY_GPU_MEM;
  if ((a.flags & PM_G_MEM_MAX) && (!mem_some || wmem > a.memory_mb_max)) return PM_WHY_GPU_MEM;
  if ((wf & PM_W_GPU_COUNT) && mem_some) {  // :506-522
    const uint32_t total = wcount * wmem;   // u32 wrapping multiply, as in compat_body
    if ((a.flags & PM_G_TOT_MIN) && total < a.total_memory_min) return PM_WHY_GPU_TOTAL;
    if ((a.flags & PM_G_TOT_MAX) && total > a.total_memory_max) return PM_WHY_GPU_TOTAL;
  }
  return PM_WHY_OK;
}

struct WhyRow {
  uint32_t wf, wcount, wmem, wcls, wcores, wram, wsto;
};
__device__ __forceinline__ WhyRow why_row(const CompatArgs& p, uint32_t w) {
  return WhyRow{p.flags[w], p.gpu_count[w], p.gpu_mem[w], p.gpu_cls[w], p.cpu_cores[w], p.ram[w], p.storage[w]};
}

// is_node_compatible_with_config (mod.rs:206-215) x ComputeSpecs::meets (node.rs:377-441), first failing clause; the
// configuration row is wave-uniform (scalar loads), as in the compat sweep
__device__ __forceinline__ uint32_t why_code(const WhyRow& r, const pm_config_row& cfg, const CompatArgs& p) {
  if (!(cfg.flags & PM_R_HAS_REQ)) return PM_WHY_OK;   // (None, _) => true
  if (!(r.wf & PM_W_HAS_SPECS)) return PM_WHY_NO_SPECS;  // (Some, None) => false
  if (cfg.flags & PM_R_CPU) {
    if (!(r.wf & PM_W_HAS_CPU)) return PM_WHY_CPU;
    if ((cfg.flags & PM_R_CPU_CORES) && (!(r.wf & PM_W_CPU_CORES) || r.wcores < cfg.cpu_cores)) return PM_WHY_CPU;
  }
  if ((cfg.flags & PM_R_RAM) && (!(r.wf & PM_W_RAM) || r.wram < cfg.ram_mb)) return PM_WHY_RAM;
  if ((cfg.flags & PM_R_STORAGE) && (!(r.wf & PM_W_STORAGE) || r.wsto < cfg.storage_gb)) return PM_WHY_STORAGE;
  if (cfg.alt_count) {
    if (!(r.wf & PM_W_HAS_GPU)) return PM_WHY_GPU_NONE;
    uint32_t worst = 0;  // the largest first-failing code: the alternative that got furthest
    for (uint32_t k = 0; k < cfg.alt_count; ++k) {
      const uint32_t c = gpu_alt_why(r.wf, r.wcount, r.wmem, r.wcls, p.alts[cfg.alt_begin + k], p.model_bits, p.model_words);
      if (c == PM_WHY_OK) return PM_WHY_OK;
      worst = c > worst ? c : worst;
    }
    return worst;
  }
  return PM_WHY_OK;
}

// pm_explain_workers: one listed worker per lane, the configurations in turn; four byte codes go out as one dword, rows of
// `stride` dwords (n_cfgs rounded up to four bytes; the host drops the padding in its copy)
__global__ __launch_bounds__(256) void explain_kernel(CompatArgs p, const uint32_t* __restrict__ rows, uint32_t n,
                                                      uint32_t stride, uint32_t* __restrict__ why_out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const WhyRow r = why_row(p, rows[i]);
  for (uint32_t c0 = 0; c0 < p.n_cfgs; c0 += 4u) {
    uint32_t word = 0;
    for (uint32_t j = 0; j < 4u && c0 + j < p.n_cfgs; ++j) word |= why_code(r, p.cfgs[c0 + j], p) << (8u * j);
    why_out[size_t(i) * stride + c0 / 4u] = word;
  }
}

__device__ __forceinline__ bool group_live(const ReportArgs& a, uint32_t g) {
  return !a.live_bits || ((a.live_bits[g >> 5] >> (g & 31u)) & 1u);
}
__device__ __forceinline__ uint32_t task_pos(const ReportArgs& a, uint32_t u, bool* live) {
  const uint64_t w = a.tlive[u >> 6];
  *live = (w >> (u & 63u)) & 1ull;
  return a.tprefix[u >> 6] + (uint32_t)__popcll(w & ((1ull << (u & 63u)) - 1ull));
}

// pm_config_report in one launch: every workgroup takes a grid-stride share of the worker rows, of the group slots and of
// the task index space, counts into LDS, and adds each non-zero counter to the global row once.  Worker x configuration
// counts go through ballots: one per distinct code in the wave (mostly one or two), not one LDS atomic per pair.
__global__ __launch_bounds__(256) void config_report_kernel(ReportArgs a) {
  __shared__ uint32_t s_cnt[PM_MAX_CONFIGS * REP_STRIDE];
  const uint32_t C = a.c.n_cfgs, lane = threadIdx.x & 63u;
  for (uint32_t k = threadIdx.x; k < C * REP_STRIDE; k += 256u) s_cnt[k] = 0u;
  __syncthreads();
  const uint32_t step = gridDim.x * 256u;
  // ---- workers: Healthy with a p2p id, by reason code; idle ones that meet it
  for (uint32_t base = blockIdx.x * 256u + (threadIdx.x & ~63u); base < a.c.W; base += step) {
    const uint32_t w = base + lane;
    const bool in = w < a.c.W;
    const WhyRow r = why_row(a.c, in ? w : 0u);
    const bool elig = in && (r.wf & PM_W_HEALTHY) && (r.wf & PM_W_HAS_P2P);
    if (!__ballot(elig)) continue;
    const bool idle = elig && a.group_of[w] < 0;
    for (uint32_t c = 0; c < C; ++c) {
      const uint32_t code = elig ? why_code(r, a.c.cfgs[c], a.c) : PM_WHY_N;
      uint64_t left = __ballot(elig);
      while (left) {  // (wave-uniform)
        const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)code, (int)__builtin_ctzll(left));
        const uint64_t m = __ballot(code == k);
        if (lane == 0u) atomicAdd(&s_cnt[c * REP_STRIDE + REP_WHY + k], (uint32_t)__popcll(m));
        left &= ~m;
      }
      const uint64_t mi = __ballot(idle && code == PM_WHY_OK);
      if (lane == 0u && mi) atomicAdd(&s_cnt[c * REP_STRIDE + REP_IDLE], (uint32_t)__popcll(mi));
    }
  }
  // ---- live groups by configuration
  for (uint32_t g = blockIdx.x * 256u + threadIdx.x; g < a.G; g += step) {
    const uint32_t c = a.g_cfg[g];
    if (!group_live(a, g) || c >= C) continue;
    atomicAdd(&s_cnt[c * REP_STRIDE + REP_GROUPS], 1u);
    atomicAdd(&s_cnt[c * REP_STRIDE + REP_MEMBERS], a.g_n[g]);
    if (a.g_task[g] == PM_NONE) atomicAdd(&s_cnt[c * REP_STRIDE + REP_NO_TASK], 1u);
  }
  // ---- live tasks whose mask has the bit
  if (a.tmask) {
    for (uint32_t base = a.t_lo + blockIdx.x * 256u + (threadIdx.x & ~63u); base < a.t_cap; base += step) {
      const uint32_t u = base + lane;
      const uint64_t mask = (u < a.t_cap && ((a.tlive[u >> 6] >> (u & 63u)) & 1ull)) ? a.tmask[u] : 0ull;
      if (!__ballot(mask != 0ull)) continue;
      for (uint32_t c = 0; c < C; ++c) {
        const uint64_t m = __ballot((mask >> c) & 1ull);
        if (lane == 0u && m) atomicAdd(&s_cnt[c * REP_STRIDE + REP_TASKS], (uint32_t)__popcll(m));
      }
    }
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < C * REP_STRIDE; k += 256u)
    if (s_cnt[k]) atomicAdd(&a.out[k], s_cnt[k]);
}

// pm_task_report, first the groups: every live group adds itself to its task's running counts (scattered by the task's
// list position) and to the live-group count of its configuration (a.out, zeroed beforehand)
__global__ __launch_bounds__(256) void task_report_groups_kernel(ReportArgs a) {
  __shared__ uint32_t s_g[PM_MAX_CONFIGS];
  const uint32_t C = a.c.n_cfgs;
  if (threadIdx.x < PM_MAX_CONFIGS) s_g[threadIdx.x] = 0u;
  __syncthreads();
  for (uint32_t g = blockIdx.x * 256u + threadIdx.x; g < a.G; g += gridDim.x * 256u) {
    const uint32_t c = a.g_cfg[g];
    if (!group_live(a, g) || c >= C) continue;
    atomicAdd(&s_g[c], 1u);
    const uint32_t u = a.g_task[g];
    if (u == PM_NONE || u < a.t_lo || u >= a.t_cap) continue;
    bool live;
    const uint32_t pos = task_pos(a, u, &live);
    if (!live) continue;
    if (a.running) atomicAdd(&a.running[pos], 1u);
    if (a.workers) atomicAdd(&a.workers[pos], a.g_n[g]);
  }
  __syncthreads();
  if (threadIdx.x < C && s_g[threadIdx.x]) atomicAdd(&a.out[threadIdx.x], s_g[threadIdx.x]);
}

// ... then one pass over the task index space: the per-configuration group counts sit in LDS and every live task sums them
// over its mask's bits into its position
__global__ __launch_bounds__(256) void task_report_tasks_kernel(ReportArgs a) {
  __shared__ uint32_t s_g[PM_MAX_CONFIGS];
  __shared__ uint32_t s_all;
  const uint32_t C = a.c.n_cfgs;
  if (threadIdx.x < PM_MAX_CONFIGS) s_g[threadIdx.x] = threadIdx.x < C ? a.out[threadIdx.x] : 0u;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (uint32_t c = 0; c < C; ++c) t += s_g[c];
    s_all = t;
  }
  __syncthreads();
  const uint64_t valid = C >= 64u ? ~0ull : (1ull << C) - 1ull;
  for (uint32_t u = a.t_lo + blockIdx.x * 256u + threadIdx.x; u < a.t_cap; u += gridDim.x * 256u) {
    bool live;
    const uint32_t pos = task_pos(a, u, &live);
    if (!live) continue;
    uint64_t m = a.tmask[u] & valid;
    uint32_t sum = 0;
    if (m == valid) {
      sum = s_all;  // (unrestricted tasks: every configuration)
    } else {
      for (; m; m &= m - 1ull) sum += s_g[__builtin_ctzll(m)];
    }
    a.allowed[pos] = sum;
  }
}

static uint32_t report_blocks(uint32_t rows, uint32_t cap) {
  const uint32_t b = (rows + 255u) / 256u;
  return b < 1u ? 1u : (b > cap ? cap : b);
}

void launch_explain(const CompatArgs& p, const uint32_t* rows, uint32_t n, uint32_t stride, uint32_t* why_out, hipStream_t s) {
  if (n == 0 || p.n_cfgs == 0) return;
  hipLaunchKernelGGL(explain_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, p, rows, n, stride, why_out);
}
void launch_config_report(const ReportArgs& a, uint32_t max_blocks, hipStream_t s) {
  if (a.c.n_cfgs == 0) return;
  uint32_t rows = a.c.W > a.G ? a.c.W : a.G;
  if (a.t_cap - a.t_lo > rows) rows = a.t_cap - a.t_lo;
  hipLaunchKernelGGL(config_report_kernel, dim3(report_blocks(rows, max_blocks)), dim3(256), 0, s, a);
}
void launch_task_report(const ReportArgs& a, uint32_t max_blocks, hipStream_t s) {
  if (a.G) hipLaunchKernelGGL(task_report_groups_kernel, dim3(report_blocks(a.G, max_blocks)), dim3(256), 0, s, a);
  if (a.allowed && a.t_cap > a.t_lo)
    hipLaunchKernelGGL(task_report_tasks_kernel, dim3(report_blocks(a.t_cap - a.t_lo, 4096u)), dim3(256), 0, s, a);
}
