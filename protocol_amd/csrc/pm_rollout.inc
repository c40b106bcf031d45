// pm_rollout.inc — the rollout ledger's kernels (included by pm_kernels.hip inside namespace pm): pm_rollout_* of
// include/pm_engine.h, with their launchers.  They read and write the ledger (an id and a state byte per worker row) and
// scratch of their own; nothing of the tick reads either.  Integers only: every result is a count or a copy, so nothing
// depends on the grid or on which wave meets which row.
//
// INGEST.  A worker named more than once ends with its last report.  ro_mark_kernel leaves in last[w] the highest report
// index (+ 1) that names w: an integer maximum is commutative and associative, so the word is the same whatever order the
// atomics land in.  ro_apply_kernel runs behind it on the stream (every mark has landed), and report i writes row w iff
// last[w] == i + 1: exactly one report per named worker does, so no two threads write one row.  The writer puts the word back
// to zero; a loser that reads it afterwards sees 0, which is no report's index + 1 either.
//
// CLASSIFY.  One pass over [0, W): the class byte, the group's same / other / silent counters, the census.  The census is
// reduced per wave by ballots, per workgroup in LDS, and reaches HBM as one atomic a bin and workgroup; a group's counters are
// reduced across the lanes of a wave that add to the same word (one atomic per distinct word and wave).
//
// PER-TASK TABLE.  The ids of the reporting rows and of the listed groups' claims are compacted into one key array (the scan
// of the metrics ledger), sorted by a least-significant-digit radix sort, eight bits a pass, EIGHT passes: every byte of the
// 64-bit id takes part.  Chunks are PM_RO_CHUNK keys whatever the grid is and a chunk is ranked by one wave in entry order,
// as in the metrics ledger's regroup.  Then one wave per run of equal keys counts what the run holds.

__global__ __launch_bounds__(256) void ro_fill_kernel(uint64_t* __restrict__ uid, uint8_t* __restrict__ state,
                                                      uint32_t* __restrict__ last, uint32_t first, uint32_t end) {
  const uint32_t w = first + blockIdx.x * 256u + threadIdx.x;
  if (w >= end) return;
  uid[w] = 0ull;
  state[w] = (uint8_t)PM_TS_NONE;
  last[w] = 0u;
}

__global__ __launch_bounds__(256) void ro_mark_kernel(const pm_ro_report* __restrict__ r, uint32_t n, uint32_t* __restrict__ last) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) atomicMax(&last[r[i].worker], i + 1u);
}

__global__ __launch_bounds__(256) void ro_apply_kernel(const pm_ro_report* __restrict__ r, uint32_t n, uint32_t* __restrict__ last,
                                                       uint64_t* __restrict__ uid, uint8_t* __restrict__ state) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const pm_ro_report rep = r[i];
  if (last[rep.worker] != i + 1u) return;
  const bool clear = rep.state == PM_TS_NONE;
  uid[rep.worker] = clear ? 0ull : rep.uid;
  state[rep.worker] = (uint8_t)rep.state;
  last[rep.worker] = 0u;
}

__global__ __launch_bounds__(256) void ro_get_kernel(const uint32_t* __restrict__ idx, uint32_t n, const uint64_t* __restrict__ uid,
                                                     const uint8_t* __restrict__ state, uint64_t* __restrict__ out_uid,
                                                     uint8_t* __restrict__ out_state) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n) return;
  out_uid[k] = uid[idx[k]];
  out_state[k] = state[idx[k]];
}

// a live group that holds a task: what the group list shows and what its members are measured against
__device__ __forceinline__ bool ro_listed(const RoGroup& gr) { return gr.slot != PM_NONE && gr.task != PM_NONE; }

// THE RULE (stated once; the group directory's member pass asks it too): a member (reported id, state) of a group that holds
// the task `claimed` is PM_RO_SILENT / _OTHER / _BEHIND / _CONVERGED
__device__ __forceinline__ uint32_t ro_member_class(uint32_t st, uint64_t id, uint64_t claimed) {
  const bool reports = st < PM_TS_N;
  const bool same = reports && id == claimed && id != ~0ull;  // (an id of all ones never matches an assignment)
  return !reports ? (uint32_t)PM_RO_SILENT : !same ? (uint32_t)PM_RO_OTHER
       : st == PM_TS_RUNNING ? (uint32_t)PM_RO_CONVERGED : (uint32_t)PM_RO_BEHIND;
}

// counters by word: the lanes of this wave that add to one word send one atomic (`todo` is wave-uniform); PM_NONE: the lane
// adds nothing.  Every lane of the wave must call it.
__device__ __forceinline__ void wave_add_words(uint32_t* __restrict__ cnt, uint32_t word, uint32_t lane) {
  uint64_t todo = __ballot(word != PM_NONE);
  while (todo) {
    const uint32_t lead = (uint32_t)__builtin_ctzll(todo);
    const uint32_t k = (uint32_t)__shfl((int)word, (int)lead);
    const uint64_t m = __ballot(word == k);
    if (lane == lead) atomicAdd(&cnt[k], (uint32_t)__popcll(m));
    todo &= ~m;
  }
}

// threads [0, W): a worker each; threads [W, W + G): whether the list entry is listed
__global__ __launch_bounds__(256) void ro_classify_kernel(RoPrepArgs a) {
  __shared__ uint32_t s_bin[PM_RO_CENSUS];
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  if (tid < PM_RO_CENSUS) s_bin[tid] = 0u;
  __syncthreads();
  const uint32_t i = blockIdx.x * 256u + tid;
  uint32_t cls = PM_NONE, st_bin = PM_NONE, word = PM_NONE;  // (PM_NONE: this lane counts nothing)
  if (i < a.W) {
    const int32_t g = a.group_of[i];
    const uint32_t st = a.state[i];
    const uint64_t id = a.uid[i];
    const bool reports = st < PM_TS_N;
    bool held = false;
    uint64_t claimed = 0;
    if (g >= 0 && (uint32_t)g < a.G) {
      const RoGroup gr = a.g[g];
      held = ro_listed(gr);
      claimed = gr.uid;
    }
    st_bin = reports ? st : (uint32_t)PM_TS_N;
    if (!held) {
      cls = reports ? PM_RO_STRAY : PM_RO_IDLE;
    } else {
      cls = ro_member_class(st, id, claimed);
      word = (uint32_t)g * PM_RO_GCNT + (cls == PM_RO_SILENT ? PM_TS_N + 1u : cls == PM_RO_OTHER ? (uint32_t)PM_TS_N : st);
    }
    a.cls[i] = (uint8_t)cls;
    a.flag[i] = reports ? 1u : 0u;
  } else if (i < a.W + a.G) {
    a.flag[i] = ro_listed(a.g[i - a.W]) ? 1u : 0u;
  }
  // the census: a ballot a bin, one LDS atomic a bin and wave
  for (uint32_t c = 0; c < PM_RO_N; ++c) {
    const uint64_t m = __ballot(cls == c);
    if (lane == 0u && m) atomicAdd(&s_bin[c], (uint32_t)__popcll(m));
  }
  for (uint32_t s = 0; s <= PM_TS_N; ++s) {
    const uint64_t m = __ballot(st_bin == s);
    if (lane == 0u && m) atomicAdd(&s_bin[PM_RO_N + s], (uint32_t)__popcll(m));
  }
  wave_add_words(a.g_cnt, word, lane);  // the groups' counters
  __syncthreads();
  if (tid < PM_RO_N + PM_TS_N + 1u && s_bin[tid]) atomicAdd(&a.census[tid], s_bin[tid]);
}

// behind the flags' scan and the complete group counters: the key array, and the groups whose every member is converged
__global__ __launch_bounds__(256) void ro_emit_kernel(RoPrepArgs a) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
  bool conv = false;
  if (i < a.W) {
    if (a.flag[i]) {
      a.key[a.off[i]] = a.uid[i];
      a.val[a.off[i]] = a.state[i];
    }
  } else if (i < a.W + a.G) {
    const uint32_t g = i - a.W;
    if (a.flag[i]) {
      const RoGroup gr = a.g[g];
      a.key[a.off[i]] = gr.uid;
      a.val[a.off[i]] = PM_RO_CLAIM | g;
      conv = a.g_cnt[g * PM_RO_GCNT + PM_TS_RUNNING] == gr.size;
    }
  }
  const uint64_t m = __ballot(conv);
  if (lane == 0u && m) atomicAdd(&a.census[PM_RO_CENSUS - 1u], (uint32_t)__popcll(m));
}

__global__ __launch_bounds__(64) void ro_radix_hist_kernel(const uint64_t* __restrict__ key, uint32_t N, uint32_t shift,
                                                           uint32_t chunks, uint32_t* __restrict__ hist) {
  __shared__ uint32_t s_h[256];
  const uint32_t lane = threadIdx.x, c = blockIdx.x;
  for (uint32_t d = lane; d < 256u; d += 64u) s_h[d] = 0u;
  __syncthreads();
  const uint32_t end = min(N, (c + 1u) * PM_RO_CHUNK);
  for (uint32_t i = c * PM_RO_CHUNK + lane; i < end; i += 64u) atomicAdd(&s_h[(uint32_t)(key[i] >> shift) & 255u], 1u);
  __syncthreads();
  for (uint32_t d = lane; d < 256u; d += 64u) hist[d * chunks + c] = s_h[d];
}

// one wave a chunk, 64 keys a round in entry order: a key's place is its digit's cursor plus the lanes in front of it that
// hold the same digit (stable)
__global__ __launch_bounds__(64) void ro_radix_scatter_kernel(const uint64_t* __restrict__ key_in, const uint32_t* __restrict__ val_in,
                                                              uint32_t N, uint32_t shift, uint32_t chunks,
                                                              const uint32_t* __restrict__ hist_scan, uint64_t* __restrict__ key_out,
                                                              uint32_t* __restrict__ val_out) {
  __shared__ uint32_t s_cur[256];
  const uint32_t lane = threadIdx.x, c = blockIdx.x;
  for (uint32_t d = lane; d < 256u; d += 64u) s_cur[d] = hist_scan[d * chunks + c];
  __syncthreads();
  for (uint32_t round = 0; round < PM_RO_CHUNK / 64u; ++round) {
    const uint32_t i = c * PM_RO_CHUNK + round * 64u + lane;
    const bool in = i < N;
    const uint64_t k = in ? key_in[i] : 0ull;
    const uint32_t d = (uint32_t)(k >> shift) & 255u;
    uint64_t peers = __ballot(in);
#pragma unroll
    for (uint32_t bit = 0; bit < 8u; ++bit) {
      const bool b = ((d >> bit) & 1u) != 0u;
      const uint64_t m = __ballot(in && b);
      peers &= b ? m : ~m;
    }
    const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
    const uint32_t at = in ? s_cur[d] + rank : 0u;
    __syncthreads();
    if (in && at < N) {
      key_out[at] = k;
      val_out[at] = val_in[i];
    }
    if (in && rank == 0u) s_cur[d] += (uint32_t)__popcll(peers);
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void ro_heads_kernel(const uint64_t* __restrict__ key, uint32_t N, uint32_t* __restrict__ head) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < N) head[i] = (i == 0u || key[i] != key[i - 1u]) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void ro_starts_kernel(const uint32_t* __restrict__ head, const uint32_t* __restrict__ head_off,
                                                        uint32_t N, uint32_t* __restrict__ start) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < N && head[i]) start[head_off[i]] = i;
}

// one wave a run: the lanes stride over it, count in registers, and the wave adds up
__global__ __launch_bounds__(256) void ro_reduce_kernel(const uint64_t* __restrict__ key, const uint32_t* __restrict__ val, uint32_t N,
                                                        const uint32_t* __restrict__ start, uint32_t D, const RoGroup* __restrict__ g,
                                                        const uint32_t* __restrict__ g_cnt, pm_ro_task_row* __restrict__ rows) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t d = blockIdx.x * 4u + (threadIdx.x >> 6);  // (wave-uniform)
  if (d >= D) return;
  const uint32_t first = start[d], end = d + 1u < D ? start[d + 1u] : N;
  uint32_t c[PM_TS_N + 4];  // reporters, groups, groups_converged, assigned, converged
#pragma unroll
  for (uint32_t q = 0; q < PM_TS_N + 4u; ++q) c[q] = 0u;
  for (uint32_t i = first + lane; i < end; i += 64u) {
    const uint32_t v = val[i];
    if (v & PM_RO_CLAIM) {
      const uint32_t slot = v & ~PM_RO_CLAIM;
      const uint32_t size = g[slot].size, conv = g_cnt[slot * PM_RO_GCNT + PM_TS_RUNNING];
      c[PM_TS_N] += 1u;
      c[PM_TS_N + 1u] += conv == size ? 1u : 0u;
      c[PM_TS_N + 2u] += size;
      c[PM_TS_N + 3u] += conv;
    } else {
#pragma unroll
      for (uint32_t s = 0; s < PM_TS_N; ++s) c[s] += v == s ? 1u : 0u;
    }
  }
#pragma unroll
  for (uint32_t q = 0; q < PM_TS_N + 4u; ++q)
#pragma unroll
    for (uint32_t m = 32u; m; m >>= 1) c[q] += (uint32_t)__shfl_xor((int)c[q], (int)m);
  if (lane != 0u) return;
  pm_ro_task_row o;
  o.uid = key[first];
  o.task = PM_NONE;  // (the host resolves it, for the rows it hands out)
  o.groups = c[PM_TS_N];
  o.groups_converged = c[PM_TS_N + 1u];
  o.assigned = c[PM_TS_N + 2u];
  o.converged = c[PM_TS_N + 3u];
#pragma unroll
  for (uint32_t s = 0; s < PM_TS_N; ++s) o.reporters[s] = c[s];
  o._pad = 0u;
  rows[d] = o;
}

__global__ __launch_bounds__(256) void ro_group_rows_kernel(const RoGroup* __restrict__ g, uint32_t G, const uint32_t* __restrict__ listed,
                                                            const uint32_t* __restrict__ off, const uint32_t* __restrict__ g_cnt,
                                                            pm_ro_group_row* __restrict__ rows) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= G || !listed[k]) return;
  const RoGroup gr = g[k];
  pm_ro_group_row o;
  o.group_id = gr.id;
  o.slot = gr.slot;
  o.config = gr.cfg;
  o.task = gr.task;
  o.size = gr.size;
#pragma unroll
  for (uint32_t s = 0; s < PM_TS_N; ++s) o.same[s] = g_cnt[k * PM_RO_GCNT + s];
  o.other = g_cnt[k * PM_RO_GCNT + PM_TS_N];
  o.silent = g_cnt[k * PM_RO_GCNT + PM_TS_N + 1u];
  rows[off[k]] = o;
}

__global__ __launch_bounds__(256) void ro_worker_flags_kernel(const uint8_t* __restrict__ cls, uint32_t W, uint32_t class_mask,
                                                              uint32_t* __restrict__ flag) {
  const uint32_t w = blockIdx.x * 256u + threadIdx.x;
  if (w < W) flag[w] = (class_mask >> cls[w]) & 1u;
}

__global__ __launch_bounds__(256) void ro_worker_rows_kernel(RoPrepArgs a, const uint32_t* __restrict__ flag,
                                                             const uint32_t* __restrict__ off, pm_ro_worker_row* __restrict__ rows) {
  const uint32_t w = blockIdx.x * 256u + threadIdx.x;
  if (w >= a.W || !flag[w]) return;
  const int32_t g = a.group_of[w];
  pm_ro_worker_row o;
  o.worker = w;
  o.group_slot = g >= 0 && (uint32_t)g < a.G ? a.g[g].slot : (uint32_t)PM_NONE;
  o.uid = a.uid[w];
  o.cls = a.cls[w];
  o.state = a.state[w];
  o._pad = 0;
  o._pad2 = 0u;
  rows[off[w]] = o;
}

void launch_ro_fill(uint64_t* uid, uint8_t* state, uint32_t* last, uint32_t first, uint32_t end, hipStream_t s) {
  if (first >= end) return;
  hipLaunchKernelGGL(ro_fill_kernel, dim3((end - first + 255u) / 256u), dim3(256), 0, s, uid, state, last, first, end);
}

void launch_ro_ingest(const pm_ro_report* r, uint32_t n, uint32_t* last, uint64_t* uid, uint8_t* state, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(ro_mark_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, r, n, last);
  hipLaunchKernelGGL(ro_apply_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, r, n, last, uid, state);
}

void launch_ro_get(const uint32_t* idx, uint32_t n, const uint64_t* uid, const uint8_t* state, uint64_t* out_uid, uint8_t* out_state,
                   hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(ro_get_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, idx, n, uid, state, out_uid, out_state);
}

void launch_ro_classify(const RoPrepArgs& a, hipStream_t s) {
  if (!(a.W + a.G)) return;
  hipLaunchKernelGGL(ro_classify_kernel, dim3((a.W + a.G + 255u) / 256u), dim3(256), 0, s, a);
}

void launch_ro_emit(const RoPrepArgs& a, hipStream_t s) {
  if (!(a.W + a.G)) return;
  hipLaunchKernelGGL(ro_emit_kernel, dim3((a.W + a.G + 255u) / 256u), dim3(256), 0, s, a);
}

void launch_ro_radix_pass(const uint64_t* key_in, const uint32_t* val_in, uint32_t N, uint32_t shift, uint32_t* hist,
                          uint32_t* hist_scan, uint64_t* key_out, uint32_t* val_out, hipStream_t s) {
  if (!N) return;
  const uint32_t chunks = (N + PM_RO_CHUNK - 1u) / PM_RO_CHUNK;
  hipLaunchKernelGGL(ro_radix_hist_kernel, dim3(chunks), dim3(64), 0, s, key_in, N, shift, chunks, hist);
  launch_mx_scan(hist, 256u * chunks, hist_scan, nullptr, s);  // (counts: never near the scan's mark bit)
  hipLaunchKernelGGL(ro_radix_scatter_kernel, dim3(chunks), dim3(64), 0, s, key_in, val_in, N, shift, chunks, hist_scan, key_out,
                     val_out);
}

uint32_t launch_ro_radix_sort(const RoSortBufs& b, uint32_t N, uint32_t passes, uint32_t cur, hipStream_t s) {
  for (uint32_t p = 0; p < passes; ++p, cur ^= 1u)
    launch_ro_radix_pass(b.key[cur], b.val[cur], N, 8u * p, b.hist, b.hist_scan, b.key[cur ^ 1u], b.val[cur ^ 1u], s);
  return cur;
}

void launch_ro_heads(const uint64_t* key, uint32_t N, uint32_t* head, hipStream_t s) {
  if (!N) return;
  hipLaunchKernelGGL(ro_heads_kernel, dim3((N + 255u) / 256u), dim3(256), 0, s, key, N, head);
}

void launch_ro_starts(const uint32_t* head, const uint32_t* head_off, uint32_t N, uint32_t* start, hipStream_t s) {
  if (!N) return;
  hipLaunchKernelGGL(ro_starts_kernel, dim3((N + 255u) / 256u), dim3(256), 0, s, head, head_off, N, start);
}

void launch_ro_reduce(const uint64_t* key, const uint32_t* val, uint32_t N, const uint32_t* start, uint32_t D, const RoGroup* g,
                      const uint32_t* g_cnt, pm_ro_task_row* rows, hipStream_t s) {
  if (!D) return;
  hipLaunchKernelGGL(ro_reduce_kernel, dim3((D + 3u) / 4u), dim3(256), 0, s, key, val, N, start, D, g, g_cnt, rows);
}

void launch_ro_group_rows(const RoGroup* g, uint32_t G, const uint32_t* listed, const uint32_t* off, const uint32_t* g_cnt,
                          pm_ro_group_row* rows, hipStream_t s) {
  if (!G) return;
  hipLaunchKernelGGL(ro_group_rows_kernel, dim3((G + 255u) / 256u), dim3(256), 0, s, g, G, listed, off, g_cnt, rows);
}

void launch_ro_worker_flags(const uint8_t* cls, uint32_t W, uint32_t class_mask, uint32_t* flag, hipStream_t s) {
  if (!W) return;
  hipLaunchKernelGGL(ro_worker_flags_kernel, dim3((W + 255u) / 256u), dim3(256), 0, s, cls, W, class_mask, flag);
}

void launch_ro_worker_rows(const RoPrepArgs& a, const uint32_t* flag, const uint32_t* off, pm_ro_worker_row* rows, hipStream_t s) {
  if (!a.W) return;
  hipLaunchKernelGGL(ro_worker_rows_kernel, dim3((a.W + 255u) / 256u), dim3(256), 0, s, a, flag, off, rows);
}
