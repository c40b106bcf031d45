// pm_liveness.inc — the liveness sweep's kernels (included by pm_kernels.hip inside namespace pm): pm_liveness_* of
// include/pm_engine.h, with their launchers.  They read and write the ledger (a status byte and an unhealthy counter per worker
// row) and the last sweep's list; nothing of the tick reads either.
//
// liveness_sweep_kernel is NodeStatusUpdater's process_node (orchestrator/src/status_update/mod.rs:191-372) for every row at
// once: one thread per row, 256 a workgroup; a wave (64 lanes on gfx950) covers the rows [64 j, 64 j + 64) — exactly word j of
// the transition bitmap, which one lane STORES (the sweep owns the whole bitmap: no read-modify-write, no memset in front).
// The census: eight ballots and popcounts per wave, added up in LDS per workgroup, then at most eight atomicAdds a workgroup.
//
// The list: change_scan_kernel (pm_changes.inc) as it is, then liveness_expand_kernel.  The expansion is liveness' own and not
// a template of change_expand_kernel: it gathers three columns (old status, status, counter) where the feed's gathers one, so a
// shared body would need a functor per row type for twelve lines of code.

// rows [first, W): Healthy where the host's flags say so, else NodeStatus::default() (Discovered); counter 0
__global__ __launch_bounds__(256) void liveness_init_kernel(const uint32_t* __restrict__ flags, uint32_t first, uint32_t W,
                                                            uint8_t* __restrict__ status, uint32_t* __restrict__ counter) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= W - first) return;
  status[first + k] = (flags[k] & PM_W_HEALTHY) ? (uint8_t)PM_NS_HEALTHY : (uint8_t)PM_NS_DISCOVERED;
  counter[first + k] = 0u;
}

__global__ __launch_bounds__(256) void liveness_sweep_kernel(LiveSweepArgs a) {
  __shared__ uint32_t s_census[PM_NS_N];
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t w = blockIdx.x * 256u + tid;
  const bool in = w < a.W;
  if (tid < (uint32_t)PM_NS_N) s_census[tid] = 0u;
  __syncthreads();
  uint32_t ns = PM_NS_N;  // (rows at or above W: in no census)
  bool listed = false;
  if (in) {
    const uint64_t beat = a.beat[w];
    const bool present = beat != 0ull && (beat > a.now_ms || a.now_ms - beat <= (uint64_t)PM_LIVE_TTL_MS);
    const bool in_pool = a.pool ? ((a.pool[w >> 6] >> (w & 63u)) & 1ull) != 0ull : true;  // (mod.rs:211)
    const uint32_t s = a.status[w], c = a.counter[w];
    uint32_t nc;
    ns = s;
    if (present) {
      // :233-252 — Unhealthy, WaitingForHeartbeat, Discovered, Dead: status_changed = true whatever the new status is
      if (s == PM_NS_UNHEALTHY || s == PM_NS_WAITING || s == PM_NS_DISCOVERED || s == PM_NS_DEAD) {
        ns = in_pool ? PM_NS_HEALTHY : PM_NS_DISCOVERED;
        listed = true;
      }
      nc = 0u;  // :255-261
    } else {
      nc = c == 0xFFFFFFFFu ? c : c + 1u;  // :265-271 (DEVIATION: saturating)
      if (s == PM_NS_HEALTHY) {  // :274-277
        ns = PM_NS_UNHEALTHY;
      } else if (s == PM_NS_UNHEALTHY) {  // :278-283
        if (nc >= a.m) ns = PM_NS_DEAD;
      } else if (s == PM_NS_DISCOVERED) {  // :284-300
        if (in_pool) ns = PM_NS_UNHEALTHY;
        else if (nc > PM_LIVE_GIVE_UP) ns = PM_NS_DEAD;
      } else if (s == PM_NS_WAITING) {  // :301-308
        if (nc >= a.m) ns = PM_NS_UNHEALTHY;
      }
      listed = ns != s;
    }
    if (ns != s) a.status[w] = (uint8_t)ns;
    if (nc != c) a.counter[w] = nc;
    if (listed) a.old_status[w] = (uint8_t)s;
  }
  // (every lane of every wave gets here)
  const uint64_t mask = __ballot(listed);
  if (lane == 0u && in) a.bitmap[w >> 6] = mask;  // (lane 0's row below W: word w / 64 < ceil(W / 64))
#pragma unroll
  for (uint32_t k = 0; k < (uint32_t)PM_NS_N; ++k) {
    const uint32_t cnt = (uint32_t)__popcll(__ballot(ns == k));
    if (lane == 0u && cnt) atomicAdd(&s_census[k], cnt);
  }
  __syncthreads();
  if (tid < (uint32_t)PM_NS_N && s_census[tid]) atomicAdd(&a.census[tid], s_census[tid]);
}

// out[prefix[j] + rank of bit b in word j] = {64 j + b, old, new, counter} for every set bit
__global__ __launch_bounds__(256) void liveness_expand_kernel(const uint64_t* __restrict__ bitmap, uint32_t n_words,
                                                              const uint32_t* __restrict__ prefix,
                                                              const uint8_t* __restrict__ old_status,
                                                              const uint8_t* __restrict__ status,
                                                              const uint32_t* __restrict__ counter, pm_live_row* __restrict__ out) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t j = blockIdx.x * 4u + (threadIdx.x >> 6);  // (wave-uniform)
  if (j >= n_words) return;
  const uint64_t word = bitmap[j];
  if (!((word >> lane) & 1ull)) return;
  const uint32_t w = j * 64u + lane;  // (< W: the sweep sets no bit at or above W)
  const uint32_t at = prefix[j] + (uint32_t)__popcll(word & ((1ull << lane) - 1ull));
  out[at] = pm_live_row{w, old_status[w], status[w], (uint16_t)0, counter[w]};
}

// stage: n indices (every one below W, no two equal), n counters, n status bytes
__global__ __launch_bounds__(256) void liveness_set_kernel(const uint32_t* __restrict__ stage, uint32_t n,
                                                           uint8_t* __restrict__ status, uint32_t* __restrict__ counter) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n) return;
  const uint32_t w = stage[k];
  status[w] = reinterpret_cast<const uint8_t*>(stage + 2u * size_t(n))[k];
  counter[w] = stage[n + k];
}

// out: n counters, n status bytes, of the rows idx[0, n) (every one below W)
__global__ __launch_bounds__(256) void liveness_get_kernel(const uint32_t* __restrict__ idx, uint32_t n,
                                                           const uint8_t* __restrict__ status, const uint32_t* __restrict__ counter,
                                                           uint32_t* __restrict__ out) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n) return;
  const uint32_t w = idx[k];
  out[k] = counter[w];
  reinterpret_cast<uint8_t*>(out + n)[k] = status[w];
}

void launch_liveness_init(const uint32_t* flags, uint32_t first, uint32_t W, uint8_t* status, uint32_t* counter, hipStream_t s) {
  if (first >= W) return;
  hipLaunchKernelGGL(liveness_init_kernel, dim3((W - first + 255u) / 256u), dim3(256), 0, s, flags, first, W, status, counter);
}

void launch_liveness_sweep(const LiveSweepArgs& a, hipStream_t s) {
  if (!a.W) return;
  hipLaunchKernelGGL(liveness_sweep_kernel, dim3((a.W + 255u) / 256u), dim3(256), 0, s, a);
}

// the listed rows of the bitmap's first n_words words -> out (room for every set bit), ascending; their number -> *total_host
// (pinned); prefix: n_words words of scratch
void launch_liveness_list(const uint64_t* bitmap, uint32_t n_words, const uint8_t* old_status, const uint8_t* status,
                          const uint32_t* counter, uint32_t* prefix, uint32_t* total_host, pm_live_row* out, hipStream_t s) {
  hipLaunchKernelGGL(change_scan_kernel, dim3(1), dim3(256), 0, s, bitmap, n_words, prefix, total_host);
  if (n_words)
    hipLaunchKernelGGL(liveness_expand_kernel, dim3((n_words + 3u) / 4u), dim3(256), 0, s, bitmap, n_words, prefix, old_status,
                       status, counter, out);
}

void launch_liveness_set(const uint32_t* stage, uint32_t n, uint8_t* status, uint32_t* counter, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(liveness_set_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, stage, n, status, counter);
}

void launch_liveness_get(const uint32_t* idx, uint32_t n, const uint8_t* status, const uint32_t* counter, uint32_t* out,
                         hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(liveness_get_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, idx, n, status, counter, out);
}
