// pm_near.inc — the nearest-candidates kernel (included by pm_kernels.hip inside namespace pm): pm_nearest_workers of
// include/pm_engine.h, with its launcher.  Read-only: it reads the worker columns, the host-truth group_of and the
// configuration tables, and writes the call's own output scratch alone.
//
// One workgroup of four waves per query.  The order asked for is sort_nodes_by_proximity's (mod.rs:234-255) over the
// candidates in index order — a stable sort, unlocated nodes at f64::MAX — which is the ascending order of the 96-bit key
// (a_bits, w): a_bits the bit pattern of the pair's hav_a (non-negative doubles order like their bits; a > 1 taken as 1, as
// in pm_spread.inc), the bits of f64::MAX for an unlocated candidate, and 0 for every candidate when the origin is unlocated
// (the reference does not sort then).  The worker index makes the keys distinct, so "the first k" is one definite set.
//
// Selection: each wave takes a stride of the worker rows and keeps a buffer of max(2 k, k + 64) keys in LDS.  Lanes whose
// WHOLE key is below the wave's k-th key so far (with all a equal, a threshold on a alone would let nothing or everything
// in) are compacted behind the buffer's end by ballot and prefix count; a buffer that cannot take the next 64 is sorted by
// its wave (a bitonic network over LDS, wave-local: no barrier) and cut to k, which gives the next threshold.  At the end
// every wave sorts what it holds, and the workgroup merges the four lists by rank: an entry's place is its index plus the
// number of smaller keys in the other three lists (binary searches), and the places below k are stored.
//
// PM_NEAR_SEED is resolved by the same workgroup first: the minimum over the IDLE pool's candidates of (unlocated, w).

__device__ __forceinline__ bool near_less(uint64_t a1, uint32_t w1, uint64_t a2, uint32_t w2) {
  return a1 < a2 || (a1 == a2 && w1 < w2);
}
__device__ __forceinline__ void near_wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // (the lanes read what other lanes of the wave wrote to LDS)
}

// is worker w (flags wf) a candidate of (pool, cfg)?  The pool predicate of mod.rs:492-497 first: most rows of a swarm with
// standing groups fail it and never load their spec columns.
__device__ __forceinline__ bool near_candidate(const NearArgs& a, uint32_t w, uint32_t wf, uint32_t pool,
                                               const pm_config_row& cfg) {
  if (!(wf & PM_W_HEALTHY) || !(wf & PM_W_HAS_P2P)) return false;
  if (pool == PM_NEAR_IDLE && a.group_of[w] >= 0) return false;
  const WhyRow r{wf, a.c.gpu_count[w], a.c.gpu_mem[w], a.c.gpu_cls[w], a.c.cpu_cores[w], a.c.ram[w], a.c.storage[w]};
  return why_code(r, cfg, a.c) == PM_WHY_OK;
}

// the wave sorts sa/sw[0, cnt) ascending by (a, w), through a bitonic network over the next power of two (padded with the
// largest key); cnt is wave-uniform and at most PM_NEAR_CAP
__device__ __forceinline__ void near_wave_sort(uint64_t* sa, uint32_t* sw, uint32_t cnt, uint32_t lane) {
  uint32_t P = 2u;
  while (P < cnt) P <<= 1;
  for (uint32_t i = cnt + lane; i < P; i += 64u) sa[i] = ~0ull, sw[i] = 0xFFFFFFFFu;
  near_wave_fence();
  for (uint32_t size = 2u; size <= P; size <<= 1) {
    for (uint32_t stride = size >> 1; stride; stride >>= 1) {
      for (uint32_t t = lane; t < P / 2u; t += 64u) {
        const uint32_t i = ((t & ~(stride - 1u)) << 1) | (t & (stride - 1u)), j = i + stride;
        const bool up = !(i & size);  // (size == P: every pair ascending)
        const uint64_t ai = sa[i], aj = sa[j];
        const uint32_t wi = sw[i], wj = sw[j];
        if (near_less(aj, wj, ai, wi) == up) sa[i] = aj, sw[i] = wj, sa[j] = ai, sw[j] = wi;
      }
      near_wave_fence();
    }
  }
}

// entries of the sorted list sa/sw[0, n) below the key (a, w)
__device__ __forceinline__ uint32_t near_lower_bound(const uint64_t* sa, const uint32_t* sw, uint32_t n, uint64_t a,
                                                     uint32_t w) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (near_less(sa[mid], sw[mid], a, w)) lo = mid + 1u;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void nearest_kernel(NearArgs a) {
  __shared__ uint64_t s_a[4][PM_NEAR_CAP];
  __shared__ uint32_t s_w[4][PM_NEAR_CAP];
  __shared__ uint64_t s_seed[4];
  __shared__ uint32_t s_n[4], s_cand[4], s_loc[4];
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
  const uint32_t qi = blockIdx.y, W = a.c.W, k = a.k;
  const pm_near_query q = a.q[qi];                // (uniform -> scalar loads)
  const pm_config_row cfg = a.c.cfgs[q.config];   // (the host checked config < n_cfgs)
  uint32_t* const out_w = a.workers + size_t(qi) * k;
  double* const out_km = a.km + size_t(qi) * k;
  const double km_none = __longlong_as_double((long long)PM_KEY_NOLOC);

  // ---- the origin
  uint32_t origin = q.origin;
  if (origin == PM_NEAR_SEED) {
    uint64_t best = ~0ull;  // (unlocated << 32) | w
    for (uint32_t base = wave * 64u; base < W; base += 256u) {  // (wave-uniform)
      const uint32_t w = base + lane;
      const bool in = w < W;
      const uint32_t wf = in ? a.c.flags[w] : 0u;
      const bool cand = in && near_candidate(a, w, wf, PM_NEAR_IDLE, cfg);
      if (cand) {
        const uint64_t key = ((wf & PM_W_HAS_LOC) ? 0ull : 1ull << 32) | w;
        best = key < best ? key : best;
      }
      if (__ballot(cand && (wf & PM_W_HAS_LOC))) break;  // (no later row of this wave can be in front of a located one)
    }
    best = wave_min_u64(best);
    if (lane == 0u) s_seed[wave] = best;
    __syncthreads();
    uint64_t m = s_seed[0];
    for (uint32_t j = 1; j < 4u; ++j) m = s_seed[j] < m ? s_seed[j] : m;
    origin = m == ~0ull ? PM_NONE : (uint32_t)m;
    if (origin == PM_NONE) {  // (uniform) no candidate in the IDLE pool: an empty row
      for (uint32_t j = tid; j < k; j += 256u) out_w[j] = PM_NONE, out_km[j] = km_none;
      if (tid == 0u) a.rows[qi] = pm_near_row{PM_NONE, 0u, 0u, 0u};
      return;
    }
  }
  const bool o_loc = (a.c.flags[origin] & PM_W_HAS_LOC) != 0u;
  const double olat = a.lat[origin], olon = a.lon[origin], ocos = a.coslat[origin];

  // ---- selection: this wave's rows
  uint64_t* const sa = s_a[wave];
  uint32_t* const sw = s_w[wave];
  const uint32_t cap = 2u * k > k + 64u ? 2u * k : k + 64u;  // <= PM_NEAR_CAP
  uint32_t cnt = 0, n_cand = 0, n_loc = 0;
  uint64_t thr_a = ~0ull;
  uint32_t thr_w = 0xFFFFFFFFu;
  for (uint32_t base = wave * 64u; base < W; base += 256u) {  // (wave-uniform)
    const uint32_t w = base + lane;
    const bool in = w < W && w != origin;
    const uint32_t wf = in ? a.c.flags[w] : 0u;
    const bool cand = in && near_candidate(a, w, wf, a.pool, cfg);
    const bool loc = cand && (wf & PM_W_HAS_LOC);
    const uint64_t mc = __ballot(cand);
    if (!mc) continue;
    n_cand += (uint32_t)__popcll(mc);
    n_loc += (uint32_t)__popcll(__ballot(loc));
    uint64_t bits = 0ull;
    if (cand && o_loc) {
      bits = PM_KEY_NOLOC;
      if (loc) {
        const double h = hav_a(olat, olon, ocos, a.lat[w], a.lon[w], a.coslat[w]);
        bits = (uint64_t)__double_as_longlong(h > 1.0 ? 1.0 : h);
      }
    }
    bool pass = cand && near_less(bits, w, thr_a, thr_w);
    uint64_t mp = __ballot(pass);
    uint32_t np = (uint32_t)__popcll(mp);
    if (!np) continue;
    if (cnt + np > cap) {  // (uniform; cnt > k here) cut to the k smallest: the next threshold
      near_wave_sort(sa, sw, cnt, lane);
      cnt = k;
      thr_a = sa[k - 1u], thr_w = sw[k - 1u];
      pass = pass && near_less(bits, w, thr_a, thr_w);
      mp = __ballot(pass);
      np = (uint32_t)__popcll(mp);
      near_wave_fence();  // (the threshold is read before anything lands behind it)
    }
    if (pass) {
      const uint32_t at = cnt + __builtin_amdgcn_mbcnt_hi((uint32_t)(mp >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mp, 0u));
      sa[at] = bits, sw[at] = w;  // (at < k + 64 <= cap after a cut, < cnt + np <= cap otherwise)
    }
    cnt += np;
  }
  near_wave_fence();
  if (cnt > 1u) near_wave_sort(sa, sw, cnt, lane);
  if (lane == 0u) s_n[wave] = cnt < k ? cnt : k, s_cand[wave] = n_cand, s_loc[wave] = n_loc;
  __syncthreads();

  // ---- merge by rank
  const uint32_t total = s_cand[0] + s_cand[1] + s_cand[2] + s_cand[3];
  const uint32_t n_out = total < k ? total : k;
  for (uint32_t j = 0; j < 4u; ++j) {
    const uint32_t n = s_n[j];
    for (uint32_t i = tid; i < n; i += 256u) {
      const uint64_t ka = s_a[j][i];
      const uint32_t kw = s_w[j][i];
      uint32_t rank = i;
      for (uint32_t o = 0; o < 4u; ++o)
        if (o != j) rank += near_lower_bound(s_a[o], s_w[o], s_n[o], ka, kw);
      if (rank < n_out) {
        out_w[rank] = kw;
        out_km[rank] = (o_loc && ka != PM_KEY_NOLOC) ? spread_km(__longlong_as_double((long long)ka)) : km_none;
      }
    }
  }
  for (uint32_t j = n_out + tid; j < k; j += 256u) out_w[j] = PM_NONE, out_km[j] = km_none;
  if (tid == 0u) a.rows[qi] = pm_near_row{origin, n_out, total, s_loc[0] + s_loc[1] + s_loc[2] + s_loc[3]};
}

void launch_nearest(const NearArgs& a, hipStream_t s) {
  if (!a.n_q || !a.k || a.k > PM_NEAR_MAX_K || a.n_q > PM_NEAR_MAX_QUERIES) return;
  hipLaunchKernelGGL(nearest_kernel, dim3(1, a.n_q), dim3(256), 0, s, a);
}
