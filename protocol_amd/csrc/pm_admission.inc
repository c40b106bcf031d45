// pm_admission.inc — part of pm_kernels.hip (included in place, namespace pm, behind pm_secp256k1.inc): what the middleware does
// behind ADDRESS_NOT_AUTHORIZED (auth_signature_middleware.rs:424-483) for a batch of requests, as if they were handled one after
// another in batch order, all at now_ms — the rate window per row, the request's age, the nonce's format and the replay set —
// and the beat column the liveness sweep reads.
//
// Nothing here depends on which thread comes first: order comes from the ledgers' stable radix sort (launch_ro_radix_sort: fixed
// chunks, ties keep entry order), ranks from lower bounds and launch_mx_scan, and every ledger word has one writer.
//
// Rate: the requests that pass the gate, sorted by row.  A request's rank in its row's run is the number of requests of the row
// in front of it in batch order; the first `room` of them pass, and the run's head writes the row's window (a kernel of its own,
// behind the one that reads the windows).
//
// Nonce set: entries sorted by the first k bits of the digest (k = 64 but for the test hook), equal keys in the order they came:
// standing entries before new ones, new ones in batch order.  The batch's entries are sorted by the same key; a new entry looks
// its key up in the standing array (lower bound) and walks the run of equal keys comparing all 256 bits, then walks back over
// the batch's own run for an earlier copy.  The next standing array is a merge by cross ranks: a kept new entry goes to (kept new
// entries in front of it) + (kept standing entries with a key <= its own), a kept standing entry to (kept standing entries in
// front of it) + (kept new entries with a smaller key).  Standing entries that are no longer live are not kept.  The standing
// array is read by one flag pass and one copy pass and scanned once; it is never sorted again.
static constexpr uint32_t PM_AD_GATE = 0xFFu;   // stage: the gate refused the request (or gave it no row): nothing touches it
static constexpr uint32_t PM_AD_NONCE = 0xFEu;  // stage: the request reaches the nonce set
static constexpr uint64_t PM_AD_WINDOW_MS = 60000ull;
static constexpr uint32_t PM_AD_MAX_REQUESTS = 100u;
static constexpr uint64_t PM_AD_MAX_AGE_S = 300ull;

__device__ __forceinline__ uint64_t ad_key(uint64_t d0, uint32_t kbits) { return __builtin_bswap64(d0) >> (64u - kbits); }

// an entry is live: the liveness ledger's convention for Redis' edge millisecond
__device__ __forceinline__ bool ad_live(uint64_t now_ms, uint64_t stored_ms) {
  return now_ms < stored_ms || now_ms - stored_ms <= (uint64_t)PM_RQ_NONCE_TTL_MS;
}

// what a row's window gives at now_ms: base = the count the batch's requests add to (0: the window starts over)
__device__ __forceinline__ bool ad_window(uint64_t now_ms, uint64_t w, uint32_t c, uint32_t* base) {
  const bool fresh = (w == 0ull && c == 0u) || (now_ms >= w && now_ms - w >= PM_AD_WINDOW_MS);
  *base = fresh ? 0u : c;
  return fresh;
}

// the first position of key[0, n) that holds a key >= k (upper: > k)
template <bool UPPER>
__device__ __forceinline__ uint32_t ad_bound(const uint64_t* __restrict__ key, uint32_t n, uint64_t k) {
  uint32_t lo = 0u, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    const uint64_t x = key[mid];
    if (UPPER ? x <= k : x < k) lo = mid + 1u; else hi = mid;
  }
  return lo;
}

// the same over the standing digests: entry q's key is made from its first word
template <bool UPPER>
__device__ __forceinline__ uint32_t ad_bound_dig(const uint64_t* __restrict__ dig, uint32_t N, uint32_t kbits, uint64_t k) {
  uint32_t lo = 0u, hi = N;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    const uint64_t x = ad_key(dig[4u * (size_t)mid], kbits);
    if (UPPER ? x <= k : x < k) lo = mid + 1u; else hi = mid;
  }
  return lo;
}

// key[i] = the request's row where it passed the gate (BANNED passes the middleware), else W: behind every row
__global__ __launch_bounds__(256) void ad_row_key_kernel(const uint32_t* __restrict__ verdict, uint32_t n, uint32_t W,
                                                         uint64_t* __restrict__ key, uint32_t* __restrict__ val) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t code = verdict[8u * (size_t)i], row = verdict[8u * (size_t)i + 1u];
  key[i] = ((code == PM_RQ_BANNED || code == PM_RQ_OK) && row < W) ? row : W;
  val[i] = i;
}

// one lane a sorted position: rate limit, age and the nonce's format, the first that applies
__global__ __launch_bounds__(256) void ad_rate_kernel(const AdRateArgs a) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= a.n) return;
  const uint64_t k = a.key[j];
  const uint32_t i = a.val[j];
  if (i >= a.n) return;
  if (k >= a.W) {
    a.stage[i] = PM_AD_GATE;
    return;
  }
  const uint32_t rank = j - ad_bound<false>(a.key, a.n, k);
  uint32_t base;
  ad_window(a.now_ms, a.win[k], a.cnt[k], &base);
  const uint32_t room = base >= PM_AD_MAX_REQUESTS ? 0u : PM_AD_MAX_REQUESTS - base;
  const uint32_t f = a.flags ? a.flags[i] : 0u;
  uint32_t st = PM_AD_NONCE;
  if (rank >= room) {
    st = PM_RQ_RATE_LIMITED;
  } else if (!(f & PM_RQ_FLAG_NO_TIMESTAMP) && a.ts && a.now_ms / 1000ull - a.ts[i] > PM_AD_MAX_AGE_S) {  // (wrapping: a future timestamp expires)
    st = PM_RQ_EXPIRED;
  } else if ((f & PM_RQ_FLAG_NO_NONCE) || !a.noff) {
    st = PM_RQ_NO_NONCE;
  } else {
    const uint32_t first = a.noff[i], len = a.noff[i + 1u] - first;
    bool good = len >= 16u && len <= 64u;
    if (good)
      for (uint32_t q = 0; q < len; ++q) {
        const uint32_t c = a.nonce[(size_t)first + q];
        good = good && ((c >= '0' && c <= '9') || (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z') || c == '-');
      }
    if (!good) st = PM_RQ_BAD_NONCE;
  }
  a.stage[i] = st;
}

// the head of a row's run writes the row's window: the run's first min(m, room) requests were counted
__global__ __launch_bounds__(256) void ad_rate_commit_kernel(const uint64_t* __restrict__ key, uint32_t n, uint32_t W, uint64_t now_ms,
                                                             uint64_t* __restrict__ win, uint32_t* __restrict__ cnt) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= n) return;
  const uint64_t k = key[j];
  if (k >= W || (j > 0u && key[j - 1u] == k)) return;
  const uint32_t m = ad_bound<true>(key, n, k) - j;
  uint32_t base;
  const bool fresh = ad_window(now_ms, win[k], cnt[k], &base);
  const uint32_t room = base >= PM_AD_MAX_REQUESTS ? 0u : PM_AD_MAX_REQUESTS - base;
  const uint32_t took = m < room ? m : room;
  if (fresh) win[k] = now_ms;
  if (took) cnt[k] = base + took;
}

__global__ __launch_bounds__(256) void ad_nonce_key_kernel(const uint64_t* __restrict__ dig, uint32_t n, uint32_t kbits,
                                                           uint64_t* __restrict__ key, uint32_t* __restrict__ val) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  key[i] = ad_key(dig[4u * (size_t)i], kbits);
  val[i] = i;
}

__device__ __forceinline__ bool ad_same(const uint64_t* __restrict__ a, const uint64_t* __restrict__ b) {
  return a[0] == b[0] && a[1] == b[1] && a[2] == b[2] && a[3] == b[3];
}

// one lane a sorted position: a live standing entry with the same 256 bits, or an earlier request of the batch with them that
// reached this step, is a replay; anything else is stored
__global__ __launch_bounds__(256) void ad_nonce_kernel(const AdNonceArgs a) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= a.n) return;
  const uint32_t i = a.val[j];
  a.keep_new[j] = 0u;
  if (i >= a.n) return;
  a.replay[i] = 0u;
  if (a.stage[i] != PM_AD_NONCE) return;
  const uint64_t k = a.key[j];
  const uint64_t* d = a.dig + 4u * (size_t)i;
  bool rep = false, found = false;
  for (uint32_t q = ad_bound_dig<false>(a.old_dig, a.N, a.kbits, k); q < a.N && !found; ++q) {
    const uint64_t* o = a.old_dig + 4u * (size_t)q;
    if (ad_key(o[0], a.kbits) != k) break;
    if (ad_same(o, d)) found = true, rep = ad_live(a.now_ms, a.old_ms[q]);  // (the set holds a digest once)
  }
  for (uint32_t p = j; !rep && p > 0u && a.key[p - 1u] == k; --p) {
    const uint32_t i2 = a.val[p - 1u];
    if (i2 < a.n && a.stage[i2] == PM_AD_NONCE && ad_same(a.dig + 4u * (size_t)i2, d)) rep = true;
  }
  a.replay[i] = rep ? 1u : 0u;
  a.keep_new[j] = rep ? 0u : 1u;
}

__global__ __launch_bounds__(256) void ad_old_live_kernel(const uint64_t* __restrict__ old_ms, uint32_t N, uint64_t now_ms,
                                                          uint32_t* __restrict__ keep_old) {
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  if (q < N) keep_old[q] = ad_live(now_ms, old_ms[q]) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void ad_merge_new_kernel(const AdMergeArgs a) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= a.n || !a.keep_new[j]) return;
  const uint32_t i = a.val[j];
  const uint32_t at = a.rank_new[j] + a.rank_old[ad_bound_dig<true>(a.old_dig, a.N, a.kbits, a.key[j])];
  if (i >= a.n || at >= a.cap) return;
#pragma unroll
  for (uint32_t q = 0; q < 4u; ++q) a.out_dig[4u * (size_t)at + q] = a.dig[4u * (size_t)i + q];
  a.out_ms[at] = a.now_ms;
}

__global__ __launch_bounds__(256) void ad_merge_old_kernel(const AdMergeArgs a) {
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  if (q >= a.N || !a.keep_old[q]) return;
  const uint64_t* o = a.old_dig + 4u * (size_t)q;
  const uint32_t at = a.rank_old[q] + a.rank_new[ad_bound<false>(a.key, a.n, ad_key(o[0], a.kbits))];
  if (at >= a.cap) return;
#pragma unroll
  for (uint32_t w = 0; w < 4u; ++w) a.out_dig[4u * (size_t)at + w] = o[w];
  a.out_ms[at] = a.old_ms[q];
}

// one lane a request: the verdict's code is the gate's, the stage's, REPLAY, or the gate's BANNED / OK behind all of them; an OK
// that is a beat stamps its row (every beat of a call stamps now_ms: the maximum does not depend on who is first); the census by
// ballots
__global__ __launch_bounds__(256) void ad_final_kernel(uint32_t* __restrict__ verdict, uint32_t n, uint32_t W,
                                                       const uint32_t* __restrict__ stage, const uint32_t* __restrict__ replay,
                                                       const uint8_t* __restrict__ flags, uint64_t now_ms, uint64_t* __restrict__ beat,
                                                       uint32_t* __restrict__ counts) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
  uint32_t code = PM_AD_N_CODES;
  if (i < n) {
    code = verdict[8u * (size_t)i];
    const uint32_t st = stage[i];
    if (st == PM_AD_NONCE)
      code = replay[i] ? (uint32_t)PM_RQ_REPLAY : code;
    else if (st != PM_AD_GATE)
      code = st;
    verdict[8u * (size_t)i] = code;
    const uint32_t row = verdict[8u * (size_t)i + 1u];
    if (code == PM_RQ_OK && flags && (flags[i] & PM_RQ_FLAG_BEAT) && row < W)
      atomicMax((unsigned long long*)(beat + row), (unsigned long long)now_ms);
  }
#pragma unroll
  for (uint32_t c = 0; c < (uint32_t)PM_AD_N_CODES; ++c) {
    const uint64_t m = __ballot(code == c);
    if (lane == 0u && m) atomicAdd(counts + c, (uint32_t)__popcll(m));
  }
}

// the hand-over calls: rows idx[0, n), distinct for the writers
__global__ __launch_bounds__(256) void ad_gather_kernel(const uint32_t* __restrict__ idx, uint32_t n, const uint64_t* __restrict__ a64,
                                                        const uint32_t* __restrict__ a32, uint64_t* __restrict__ out64,
                                                        uint32_t* __restrict__ out32) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n) return;
  out64[k] = a64[idx[k]];
  if (a32) out32[k] = a32[idx[k]];
}

__global__ __launch_bounds__(256) void ad_scatter_kernel(const uint32_t* __restrict__ idx, uint32_t n, uint32_t W,
                                                         const uint64_t* __restrict__ in64, const uint32_t* __restrict__ in32,
                                                         uint64_t* __restrict__ a64, uint32_t* __restrict__ a32) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n || idx[k] >= W) return;
  a64[idx[k]] = in64[k];
  if (a32) a32[idx[k]] = in32[k];
}

// out[w] = the later of the two columns
__global__ __launch_bounds__(256) void ad_beat_max_kernel(const uint64_t* __restrict__ col, uint32_t W, uint64_t* __restrict__ out) {
  const uint32_t w = blockIdx.x * 256u + threadIdx.x;
  if (w < W) out[w] = out[w] > col[w] ? out[w] : col[w];
}

static inline dim3 ad_grid(uint32_t n) { return dim3((n + 255u) / 256u); }

static inline uint32_t ad_passes(uint64_t top) {  // radix passes that cover every value <= top
  uint32_t p = 1u;
  while (p < 8u && (top >> (8u * p))) ++p;
  return p;
}

// the requests sorted by row into b (the buffer returned), then the stages
uint32_t launch_ad_rate(AdRateArgs a, const uint32_t* verdict, const RoSortBufs& b, hipStream_t s) {
  if (!a.n) return 0u;
  hipLaunchKernelGGL(ad_row_key_kernel, ad_grid(a.n), dim3(256), 0, s, verdict, a.n, a.W, b.key[0], b.val[0]);
  const uint32_t cur = launch_ro_radix_sort(b, a.n, ad_passes(a.W), 0u, s);
  a.key = b.key[cur], a.val = b.val[cur];
  hipLaunchKernelGGL(ad_rate_kernel, ad_grid(a.n), dim3(256), 0, s, a);
  return cur;
}

void launch_ad_rate_commit(const uint64_t* key, uint32_t n, uint32_t W, uint64_t now_ms, uint64_t* win, uint32_t* cnt, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(ad_rate_commit_kernel, ad_grid(n), dim3(256), 0, s, key, n, W, now_ms, win, cnt);
}

// the batch's nonces sorted by key into b, the replays, the flags of what is kept on both sides
uint32_t launch_ad_nonces(AdNonceArgs a, const RoSortBufs& b, uint32_t* keep_old, hipStream_t s) {
  uint32_t cur = 0u;
  if (a.n) {
    hipLaunchKernelGGL(ad_nonce_key_kernel, ad_grid(a.n), dim3(256), 0, s, a.dig, a.n, a.kbits, b.key[0], b.val[0]);
    cur = launch_ro_radix_sort(b, a.n, (a.kbits + 7u) / 8u, 0u, s);
    a.key = b.key[cur], a.val = b.val[cur];
    hipLaunchKernelGGL(ad_nonce_kernel, ad_grid(a.n), dim3(256), 0, s, a);
  }
  if (a.N) hipLaunchKernelGGL(ad_old_live_kernel, ad_grid(a.N), dim3(256), 0, s, a.old_ms, a.N, a.now_ms, keep_old);
  return cur;
}

void launch_ad_old_live(const uint64_t* old_ms, uint32_t N, uint64_t now_ms, uint32_t* keep_old, hipStream_t s) {
  if (N) hipLaunchKernelGGL(ad_old_live_kernel, ad_grid(N), dim3(256), 0, s, old_ms, N, now_ms, keep_old);
}

void launch_ad_merge(const AdMergeArgs& a, hipStream_t s) {
  if (a.n) hipLaunchKernelGGL(ad_merge_new_kernel, ad_grid(a.n), dim3(256), 0, s, a);
  if (a.N) hipLaunchKernelGGL(ad_merge_old_kernel, ad_grid(a.N), dim3(256), 0, s, a);
}

void launch_ad_final(uint32_t* verdict, uint32_t n, uint32_t W, const uint32_t* stage, const uint32_t* replay, const uint8_t* flags,
                     uint64_t now_ms, uint64_t* beat, uint32_t* counts, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(ad_final_kernel, ad_grid(n), dim3(256), 0, s, verdict, n, W, stage, replay, flags, now_ms, beat, counts);
}

void launch_ad_gather(const uint32_t* idx, uint32_t n, const uint64_t* a64, const uint32_t* a32, uint64_t* out64, uint32_t* out32,
                      hipStream_t s) {
  if (n) hipLaunchKernelGGL(ad_gather_kernel, ad_grid(n), dim3(256), 0, s, idx, n, a64, a32, out64, out32);
}

void launch_ad_scatter(const uint32_t* idx, uint32_t n, uint32_t W, const uint64_t* in64, const uint32_t* in32, uint64_t* a64,
                       uint32_t* a32, hipStream_t s) {
  if (n) hipLaunchKernelGGL(ad_scatter_kernel, ad_grid(n), dim3(256), 0, s, idx, n, W, in64, in32, a64, a32);
}

void launch_ad_beat_max(const uint64_t* col, uint32_t W, uint64_t* out, hipStream_t s) {
  if (W) hipLaunchKernelGGL(ad_beat_max_kernel, ad_grid(W), dim3(256), 0, s, col, W, out);
}
