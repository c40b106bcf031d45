// pm_metrics.inc — the metrics ledger's kernels (included by pm_kernels.hip inside namespace pm): pm_metrics_* of
// include/pm_engine.h, with their launchers.  They read and write the ledger (a CSR of (series, value) entries, the manual row
// in front, rows sorted by series) and scratch of their own; nothing of the tick reads either.
//
// INGEST.  mx_fold_kernel is store_metrics / delete_metric / the heartbeat route's stale-key deletion (metrics_store.rs:25-109,
// heartbeat.rs:94-151) for one touched row per workgroup of ONE wave: the row sits in LDS, unsorted, and the row's beats are
// applied to it in batch order, entry by entry; what runs in parallel inside a step is the search for a series (64 slots a
// look) and the compaction, never two entries.  So the result does not depend on which wave gets which row.  The kernel runs
// twice: the count pass leaves the row's new length (and says whether a row would pass PM_MX_ROW_MAX), then, behind the scan
// of the lengths and only if no row did, the write pass folds again and stores the row sorted by series.  Rows no beat names
// are copied by mx_copy_kernel, one thread per old entry.
//
// TOTALS.  A least-significant-digit radix sort of the entries by series, eight bits a pass, as many passes as n_series
// needs.  It is stable, and the entries start in row order, so every series ends with its values in ascending row order.  The
// chunks are PM_MX_CHUNK entries whatever the grid is, the histograms are integer counts, and a chunk is ranked by one wave in
// entry order (peers by ballots): the output position of every entry is a function of the ledger alone.  mx_sum_kernel then
// adds every series' values one by one, one wave a series.

// p[first, end) = v
__global__ __launch_bounds__(256) void mx_fill_kernel(uint32_t* __restrict__ p, uint32_t first, uint32_t end, uint32_t v) {
  const uint32_t i = first + blockIdx.x * 256u + threadIdx.x;
  if (i < end) p[i] = v;
}

__global__ __launch_bounds__(256) void mx_lengths_kernel(const uint32_t* __restrict__ off, uint32_t R, uint32_t* __restrict__ new_n) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r < R) new_n[r] = off[r + 1] - off[r];
}

// slot of `series` among the row's n entries, or PM_NONE (wave-uniform: every lane gets the same answer)
__device__ __forceinline__ uint32_t mx_find(const uint32_t* s_ser, uint32_t n, uint32_t series, uint32_t lane) {
  for (uint32_t base = 0; base < n; base += 64u) {
    const uint32_t i = base + lane;
    const uint64_t m = __ballot(i < n && s_ser[i] == series);
    if (m) return base + (uint32_t)__builtin_ctzll(m);
  }
  return PM_NONE;
}

template <bool WRITE>
__global__ __launch_bounds__(64) void mx_fold_kernel(MxFoldArgs a) {
  __shared__ double s_val[PM_MX_ROW_MAX];
  __shared__ uint32_t s_ser[PM_MX_ROW_MAX];
  __shared__ uint8_t s_keep[PM_MX_ROW_MAX];
  const uint32_t lane = threadIdx.x, k = blockIdx.x;
  if (k >= a.n_touched) return;
  const uint32_t row = a.t_row[k], b0 = a.t_first[k], nb = a.t_nb[k];
  const uint32_t o0 = a.off_old[row];
  uint32_t n = min(a.off_old[row + 1] - o0, (uint32_t)PM_MX_ROW_MAX);  // (a row is never longer: the bound refuses the batch)
  for (uint32_t i = lane; i < n; i += 64u) {
    s_ser[i] = a.ser_old[o0 + i];
    s_val[i] = a.val_old[o0 + i];
  }
  __syncthreads();
  bool over = false;
  // (everything below is wave-uniform but the slot a lane looks at: n, the hits and the branches are the same in all lanes)
  for (uint32_t b = b0; b < b0 + nb; ++b) {
    const pm_mx_beat beat = a.beats[b];
    const pm_mx_entry* const ent = a.entries + beat.first;
    if (beat.kind == PM_MXB_REPLACE) {
      // heartbeat.rs:109-140 — the stale keys go first: every series the beat does not name
      for (uint32_t i = lane; i < n; i += 64u) s_keep[i] = 0;
      __syncthreads();
      for (uint32_t j = 0; j < beat.n; ++j) {
        const uint32_t at = mx_find(s_ser, n, ent[j].series, lane);
        if (at != PM_NONE && lane == 0u) s_keep[at] = 1;
      }
      __syncthreads();
      uint32_t m = 0;
      for (uint32_t base = 0; base < n; base += 64u) {
        const uint32_t i = base + lane;
        const bool keep = i < n && s_keep[i] != 0;
        const uint32_t sv = keep ? s_ser[i] : 0u;
        const double vv = keep ? s_val[i] : 0.0;
        const uint64_t mask = __ballot(keep);
        const uint32_t at = m + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        __syncthreads();  // (the slots this round fills lie at or below the ones it has just read)
        if (keep) {
          s_ser[at] = sv;
          s_val[at] = vv;
        }
        __syncthreads();
        m += (uint32_t)__popcll(mask);
      }
      n = m;
    }
    if (beat.kind == PM_MXB_DELETE) {  // metrics_store.rs:91-109 (HDEL: an absent field is no error)
      for (uint32_t j = 0; j < beat.n; ++j) {
        const uint32_t at = mx_find(s_ser, n, ent[j].series, lane);
        if (at == PM_NONE) continue;
        if (lane == 0u) {
          s_ser[at] = s_ser[n - 1u];
          s_val[at] = s_val[n - 1u];
        }
        --n;
        __syncthreads();
      }
    } else {  // metrics_store.rs:42-73, in the beat's order
      for (uint32_t j = 0; j < beat.n; ++j) {
        const pm_mx_entry en = ent[j];
        const uint32_t at = mx_find(s_ser, n, en.series, lane);
        if (at == PM_NONE) {
          if (n >= PM_MX_ROW_MAX) {
            over = true;
            continue;
          }
          if (lane == 0u) {
            s_ser[n] = en.series;
            s_val[n] = en.value;
          }
          ++n;
        } else if (!(en.flags & PM_MXF_MAX) || en.value > s_val[at]) {  // :52-63 (a NaN on either side: not greater)
          if (lane == 0u) s_val[at] = en.value;
        }
        __syncthreads();
      }
    }
  }
  if (!WRITE) {
    if (lane == 0u) {
      a.new_n[row] = n | PM_MX_TOUCHED;
      if (over) atomicOr(a.over, 1u);
    }
    return;
  }
  // sorted by series: an entry's place is the number of smaller series (no two are equal)
  const uint32_t o1 = a.off_new[row];
  for (uint32_t i = lane; i < n; i += 64u) {
    const uint32_t si = s_ser[i];
    uint32_t r = 0;
    for (uint32_t j = 0; j < n; ++j) r += s_ser[j] < si ? 1u : 0u;
    a.ser_new[o1 + r] = si;
    a.val_new[o1 + r] = s_val[i];
  }
}

// one workgroup: tiles of 4096 words, four a thread, a running total across the tiles
__global__ __launch_bounds__(1024) void mx_scan_kernel(const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ out,
                                                       uint32_t* __restrict__ total_host) {
  __shared__ uint32_t s_wave[16];
  __shared__ uint32_t s_carry;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  if (tid == 0u) s_carry = 0u;
  __syncthreads();
  for (uint32_t base = 0; base < n; base += 4096u) {
    const uint32_t i0 = base + tid * 4u;
    uint32_t v[4], t = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q) {
      v[q] = i0 + q < n ? (in[i0 + q] & ~PM_MX_TOUCHED) : 0u;
      t += v[q];
    }
    uint32_t x = t;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
      const uint32_t y = __shfl_up(x, d);
      if (lane >= d) x += y;
    }
    if (lane == 63u) s_wave[wave] = x;
    __syncthreads();
    uint32_t before = s_carry, tile = 0;
#pragma unroll
    for (uint32_t w = 0; w < 16u; ++w) {
      if (w < wave) before += s_wave[w];
      tile += s_wave[w];
    }
    uint32_t excl = before + x - t;
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q) {
      if (i0 + q < n) out[i0 + q] = excl;
      excl += v[q];
    }
    __syncthreads();
    if (tid == 0u) s_carry += tile;
    __syncthreads();
  }
  if (tid == 0u) {
    out[n] = s_carry;
    if (total_host) *total_host = s_carry;
  }
}

// the entries of the rows the fold did not write, one thread per OLD entry
__global__ __launch_bounds__(256) void mx_copy_kernel(const uint32_t* __restrict__ off_old, const uint32_t* __restrict__ new_n,
                                                      const uint32_t* __restrict__ off_new, uint32_t R, uint32_t N_old,
                                                      const uint32_t* __restrict__ ser_old, const double* __restrict__ val_old,
                                                      uint32_t* __restrict__ ser_new, double* __restrict__ val_new) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= N_old) return;
  uint32_t lo = 0, hi = R;  // the last row r with off_old[r] <= i (rows in front of it may be empty)
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (off_old[mid] <= i) lo = mid; else hi = mid;
  }
  if (new_n[lo] & PM_MX_TOUCHED) return;
  const uint32_t at = off_new[lo] + (i - off_old[lo]);
  ser_new[at] = ser_old[i];
  val_new[at] = val_old[i];
}

// the liveness hook: the rows of the sweep's list that became Dead are emptied (status_update/mod.rs:314-343)
__global__ __launch_bounds__(256) void mx_mark_dead_kernel(const pm_live_row* __restrict__ list, uint32_t n, uint32_t R,
                                                           const uint32_t* __restrict__ off, uint32_t* __restrict__ new_n,
                                                           uint32_t* __restrict__ hit_host) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n) return;
  const pm_live_row r = list[k];
  const uint32_t row = r.worker + 1u;
  if (r.new_status != PM_NS_DEAD || row >= R) return;
  if (off[row + 1u] == off[row]) return;  // (empty already)
  new_n[row] = PM_MX_TOUCHED;             // (length 0, and the copy leaves the row out)
  *hit_host = 1u;                         // (a flag: every writer stores the same word)
}

__global__ __launch_bounds__(256) void mx_row_lengths_kernel(const uint32_t* __restrict__ rows, uint32_t n,
                                                             const uint32_t* __restrict__ off, uint32_t* __restrict__ len) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n) return;
  const uint32_t r = rows[k];
  len[k] = off[r + 1u] - off[r];
}

// the listing with its join, one thread per output entry
__global__ __launch_bounds__(256) void mx_rows_kernel(MxRowsArgs a) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.total) return;
  uint32_t lo = 0, hi = a.n;  // the last listed row k with out_off[k] <= i
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (a.out_off[mid] <= i) lo = mid; else hi = mid;
  }
  const uint32_t row = a.rows ? a.rows[lo] : lo;
  const uint32_t src = a.off[row] + (i - a.out_off[lo]);
  pm_mx_row o;
  o.row = row ? row - 1u : (uint32_t)PM_MX_MANUAL;
  o.series = a.ser[src];
  o.value = a.val[src];
  o.group_id = (uint64_t)PM_NONE;
  o.config = 0u;
  o._pad = 0u;
  if (row) {
    const int32_t g = a.group_of[row - 1u];
    if (g >= 0) {
      o.group_id = a.g_id[g];
      o.config = a.g_cfg[g];
    }
  }
  a.out[i] = o;
}

__global__ __launch_bounds__(64) void mx_radix_hist_kernel(const uint32_t* __restrict__ ser, uint32_t N, uint32_t shift,
                                                           uint32_t chunks, uint32_t* __restrict__ hist) {
  __shared__ uint32_t s_h[256];
  const uint32_t lane = threadIdx.x, c = blockIdx.x;
  for (uint32_t d = lane; d < 256u; d += 64u) s_h[d] = 0u;
  __syncthreads();
  const uint32_t end = min(N, (c + 1u) * PM_MX_CHUNK);
  for (uint32_t i = c * PM_MX_CHUNK + lane; i < end; i += 64u) atomicAdd(&s_h[(ser[i] >> shift) & 255u], 1u);
  __syncthreads();
  for (uint32_t d = lane; d < 256u; d += 64u) hist[d * chunks + c] = s_h[d];
}

// one wave a chunk, 64 entries a round in entry order: an entry's place is its digit's cursor plus the lanes in front of it
// that hold the same digit
__global__ __launch_bounds__(64) void mx_radix_scatter_kernel(const uint32_t* __restrict__ ser_in, const double* __restrict__ val_in,
                                                              uint32_t N, uint32_t shift, uint32_t chunks,
                                                              const uint32_t* __restrict__ hist_scan, uint32_t* __restrict__ ser_out,
                                                              double* __restrict__ val_out) {
  __shared__ uint32_t s_cur[256];
  const uint32_t lane = threadIdx.x, c = blockIdx.x;
  for (uint32_t d = lane; d < 256u; d += 64u) s_cur[d] = hist_scan[d * chunks + c];
  __syncthreads();
  for (uint32_t round = 0; round < PM_MX_CHUNK / 64u; ++round) {
    const uint32_t i = c * PM_MX_CHUNK + round * 64u + lane;
    const bool in = i < N;
    const uint32_t s = in ? ser_in[i] : 0u;
    const uint32_t d = (s >> shift) & 255u;
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
      ser_out[at] = s;
      val_out[at] = val_in[i];
    }
    if (in && rank == 0u) s_cur[d] += (uint32_t)__popcll(peers);
    __syncthreads();
  }
}

// one wave a series: the segment of the sorted entries that holds it, added up front to back from +0.0
__global__ __launch_bounds__(256) void mx_sum_kernel(const uint32_t* __restrict__ ser, const double* __restrict__ val, uint32_t N,
                                                     uint32_t n_series, double* __restrict__ sum, uint32_t* __restrict__ count) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t s = blockIdx.x * 4u + (threadIdx.x >> 6);  // (wave-uniform)
  if (s >= n_series) return;
  uint32_t lo = 0, hi = N;  // the first entry with a series >= s
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (ser[mid] < s) lo = mid + 1u; else hi = mid;
  }
  const uint32_t first = lo;
  hi = N;                   // the first entry with a series > s
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (ser[mid] <= s) lo = mid + 1u; else hi = mid;
  }
  const uint32_t end = lo;
  double acc = 0.0;
  uint32_t base = first;
  // (every lane adds the same values in the same order.)  Whole tiles: lane j's value comes over the scalar side, 64 dependent
  // adds with nothing but two lane reads between them — a popular series is one long chain, and its length is the cold call's time
  for (; base + 64u <= end; base += 64u) {
    const double v = val[base + lane];
    const int lo = __double2loint(v), hi = __double2hiint(v);
#pragma unroll
    for (int j = 0; j < 64; ++j) acc += __hiloint2double(__builtin_amdgcn_readlane(hi, j), __builtin_amdgcn_readlane(lo, j));
  }
  if (base < end) {
    const uint32_t m = end - base;
    const double v = lane < m ? val[base + lane] : 0.0;
    for (uint32_t j = 0; j < m; ++j) acc += __shfl(v, (int)j);
  }
  if (lane == 0u) {
    sum[s] = acc;
    count[s] = end - first;
  }
}

void launch_mx_fill(uint32_t* p, uint32_t first, uint32_t end, uint32_t v, hipStream_t s) {
  if (first >= end) return;
  hipLaunchKernelGGL(mx_fill_kernel, dim3((end - first + 255u) / 256u), dim3(256), 0, s, p, first, end, v);
}

void launch_mx_lengths(const uint32_t* off, uint32_t R, uint32_t* new_n, hipStream_t s) {
  hipLaunchKernelGGL(mx_lengths_kernel, dim3((R + 255u) / 256u), dim3(256), 0, s, off, R, new_n);
}

void launch_mx_fold(const MxFoldArgs& a, bool write, hipStream_t s) {
  if (!a.n_touched) return;
  if (write) hipLaunchKernelGGL(mx_fold_kernel<true>, dim3(a.n_touched), dim3(64), 0, s, a);
  else hipLaunchKernelGGL(mx_fold_kernel<false>, dim3(a.n_touched), dim3(64), 0, s, a);
}

void launch_mx_scan(const uint32_t* in, uint32_t n, uint32_t* out, uint32_t* total_host, hipStream_t s) {
  hipLaunchKernelGGL(mx_scan_kernel, dim3(1), dim3(1024), 0, s, in, n, out, total_host);
}

void launch_mx_copy(const uint32_t* off_old, const uint32_t* new_n, const uint32_t* off_new, uint32_t R, uint32_t N_old,
                    const uint32_t* ser_old, const double* val_old, uint32_t* ser_new, double* val_new, hipStream_t s) {
  if (!N_old) return;
  hipLaunchKernelGGL(mx_copy_kernel, dim3((N_old + 255u) / 256u), dim3(256), 0, s, off_old, new_n, off_new, R, N_old, ser_old,
                     val_old, ser_new, val_new);
}

void launch_mx_mark_dead(const pm_live_row* list, uint32_t n, uint32_t R, const uint32_t* off, uint32_t* new_n, uint32_t* hit_host,
                         hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(mx_mark_dead_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, list, n, R, off, new_n, hit_host);
}

void launch_mx_row_lengths(const uint32_t* rows, uint32_t n, const uint32_t* off, uint32_t* len, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(mx_row_lengths_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, rows, n, off, len);
}

void launch_mx_rows(const MxRowsArgs& a, hipStream_t s) {
  if (!a.total) return;
  hipLaunchKernelGGL(mx_rows_kernel, dim3((a.total + 255u) / 256u), dim3(256), 0, s, a);
}

void launch_mx_radix_pass(const uint32_t* ser_in, const double* val_in, uint32_t N, uint32_t shift, uint32_t* hist,
                          uint32_t* hist_scan, uint32_t* ser_out, double* val_out, hipStream_t s) {
  if (!N) return;
  const uint32_t chunks = (N + PM_MX_CHUNK - 1u) / PM_MX_CHUNK;
  hipLaunchKernelGGL(mx_radix_hist_kernel, dim3(chunks), dim3(64), 0, s, ser_in, N, shift, chunks, hist);
  hipLaunchKernelGGL(mx_scan_kernel, dim3(1), dim3(1024), 0, s, hist, 256u * chunks, hist_scan, (uint32_t*)nullptr);
  hipLaunchKernelGGL(mx_radix_scatter_kernel, dim3(chunks), dim3(64), 0, s, ser_in, val_in, N, shift, chunks, hist_scan, ser_out,
                     val_out);
}

void launch_mx_sums(const uint32_t* ser_sorted, const double* val_sorted, uint32_t N, uint32_t n_series, double* sum,
                    uint32_t* count, hipStream_t s) {
  if (!n_series) return;
  hipLaunchKernelGGL(mx_sum_kernel, dim3((n_series + 3u) / 4u), dim3(256), 0, s, ser_sorted, val_sorted, N, n_series, sum, count);
}
