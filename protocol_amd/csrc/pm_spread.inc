// pm_spread.inc — the group geography kernels (included by pm_kernels.hip inside namespace pm): how far apart the members of
// every live group are (pm_group_spread), the same per configuration (pm_config_spread), with their launchers.  Read-only:
// the kernels read the worker columns and the group list and write report scratch alone.
//
// Distance: hav_a of the pair (the sine form, the key the carve certifies; symmetric in its arguments bit for bit), a > 1
// taken as 1, then d = 6371 * 2 * atan2(sqrt(a), sqrt(1 - a)) as calculate_distance has it (mod.rs:218-231).  The maximum
// over pairs is taken on a — d is a non-decreasing function of it — so the n^2 loop holds no sqrt and no atan2.
//
// Dispatch: TWO launches over two row lists the host builds from the sizes it holds anyway (n <= 64: one wave a group, four
// groups a workgroup, no barrier; n > 64: one workgroup a group).  One launch with a per-workgroup branch would give a
// workgroup of four small groups and one of a 300-member group the same resources and make every wave carry the tile
// loop's LDS; the lists cost 4 bytes a group on a copy that goes up anyway.

__device__ __forceinline__ double spread_km(double a) {
  a = a > 1.0 ? 1.0 : a;  // (the reference: NaN)
  return 6371.0 * (2.0 * atan2(sqrt(a), sqrt(1.0 - a)));
}

// ---- wave-wide unsigned max via DPP, in the style of wave_min_u32 (identity 0 for lanes a step does not reach)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_max32_step(uint32_t v) {
  const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xF, false);
  return o > v ? o : v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
  v = dpp_max32_step<0x111, 0xF>(v);  // row_shr:1
  v = dpp_max32_step<0x112, 0xF>(v);  // row_shr:2
  v = dpp_max32_step<0x114, 0xF>(v);  // row_shr:4
  v = dpp_max32_step<0x118, 0xF>(v);  // row_shr:8
  v = dpp_max32_step<0x142, 0xA>(v);  // row_bcast:15 -> rows 1,3
  v = dpp_max32_step<0x143, 0xC>(v);  // row_bcast:31 -> rows 2,3
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
  const uint32_t hi = (uint32_t)(v >> 32);
  const uint32_t mh = wave_max_u32(hi);
  const uint32_t ml = wave_max_u32(hi == mh ? (uint32_t)v : 0u);
  return ((uint64_t)mh << 32) | ml;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// one member as a lane (or an LDS slot) holds it
struct SpreadMember {
  double lat, lon, cs;
  uint32_t w, rk, loc;
};
__device__ __forceinline__ SpreadMember spread_member(const SpreadArgs& a, uint32_t at, bool in) {
  SpreadMember m{0.0, 0.0, 0.0, PM_NONE, 0xFFFFFFFFu, 0u};
  if (!in) return m;
  m.w = a.members[at];
  if (m.w >= a.W) return m;  // (never in a list the engine holds: such a member reads "not located")
  m.rk = a.addr_rank[m.w];
  m.loc = (a.flags[m.w] & PM_W_HAS_LOC) ? 1u : 0u;
  m.lat = a.lat[m.w], m.lon = a.lon[m.w], m.cs = a.coslat[m.w];
  return m;
}
// a lane's best pair so far: the larger a, then the lexicographically smaller (lo, hi)
struct SpreadBest {
  uint64_t a_bits;  // bit pattern of a >= 0: orders like the value
  uint64_t pair;    // (lo << 32) | hi, worker indices; ~0 = none yet
};
__device__ __forceinline__ void spread_take(SpreadBest& b, double a, uint32_t w1, uint32_t w2) {
  const uint64_t bits = (uint64_t)__double_as_longlong(a > 1.0 ? 1.0 : a);
  const uint64_t pair = w1 < w2 ? ((uint64_t)w1 << 32) | w2 : ((uint64_t)w2 << 32) | w1;
  if (b.pair == ~0ull || bits > b.a_bits || (bits == b.a_bits && pair < b.pair)) b.a_bits = bits, b.pair = pair;
}
__device__ __forceinline__ void spread_store(pm_group_spread_row* out, uint32_t located, uint32_t hops, SpreadBest best,
                                             double ring, uint64_t hop_bits, uint32_t hop_w) {
  pm_group_spread_row r;
  const bool measured = located >= 2u && best.pair != ~0ull;
  r.located = located;
  r.ring_hops = hops;
  r.far_a = measured ? (uint32_t)(best.pair >> 32) : PM_NONE;
  r.far_b = measured ? (uint32_t)best.pair : PM_NONE;
  r.hop_from = hops ? hop_w : PM_NONE;
  r._pad = 0u;
  r.diameter_km = measured ? spread_km(__longlong_as_double((long long)best.a_bits)) : 0.0;
  r.ring_km = hops ? ring : 0.0;
  r.longest_hop_km = hops ? __longlong_as_double((long long)hop_bits) : 0.0;
  *out = r;
}

// ---- n <= 64: one wave per group.  Lane i holds member i; member j goes round by readlane, and from the one comparison a
// lane takes its maximum (with the partner) and its rank in (addr_rank, worker) order.  The ranks are a permutation of
// [0, n): every lane pushes its number to lane `rank` and pulls the one at rank + 1 — the scatter and the gather go through
// the LDS crossbar (ds_permute / ds_bpermute) without an LDS allocation or a barrier.
__global__ __launch_bounds__(256) void group_spread_wave_kernel(SpreadArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (i >= a.n_small) return;  // (wave-uniform)
  const uint32_t row = a.small[i], slot = a.slot_of_row[row];
  const uint32_t n = a.g_n[slot], off = a.g_off[slot];
  if (n > 64u) return;  // (the host sorted the lists by the sizes it holds: never)
  const bool in = lane < n;
  const SpreadMember m = spread_member(a, off + lane, in);
  const uint64_t latb = (uint64_t)__double_as_longlong(m.lat), lonb = (uint64_t)__double_as_longlong(m.lon),
                 csb = (uint64_t)__double_as_longlong(m.cs);
  SpreadBest best{0ull, ~0ull};
  uint32_t rank = 0;
  for (uint32_t j = 0; j < n; ++j) {  // (wave-uniform)
    const uint32_t wj = (uint32_t)__builtin_amdgcn_readlane((int)m.w, (int)j);
    const uint32_t rkj = (uint32_t)__builtin_amdgcn_readlane((int)m.rk, (int)j);
    const uint32_t locj = (uint32_t)__builtin_amdgcn_readlane((int)m.loc, (int)j);
    rank += (in && (rkj < m.rk || (rkj == m.rk && wj < m.w))) ? 1u : 0u;
    if (!locj) continue;  // (uniform)
    const double latj = __longlong_as_double((long long)readlane_u64(latb, j));
    const double lonj = __longlong_as_double((long long)readlane_u64(lonb, j));
    const double csj = __longlong_as_double((long long)readlane_u64(csb, j));
    if (m.loc && j != lane) spread_take(best, hav_a(m.lat, m.lon, m.cs, latj, lonj, csj), m.w, wj);
  }
  const uint32_t located = (uint32_t)__popcll(__ballot(m.loc != 0u));
  // the group's maximum, then the smallest pair among the lanes that hold it
  const bool has = best.pair != ~0ull;
  const uint64_t amax = wave_max_u64(has ? best.a_bits : 0ull);
  SpreadBest top{amax, wave_min_u64(has && best.a_bits == amax ? best.pair : ~0ull)};
  // the ring: lane of the member after this one (lanes outside the group keep to themselves)
  const uint32_t dst = in ? rank : lane;
  const uint32_t by_rank = (uint32_t)__builtin_amdgcn_ds_permute((int)(dst << 2), (int)lane);
  const uint32_t nxt_rank = in ? (rank + 1u == n ? 0u : rank + 1u) : lane;
  const uint32_t nxt = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(nxt_rank << 2), (int)by_rank);
  const uint32_t loc2 = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(nxt << 2), (int)m.loc);
  const double lat2 = __shfl(m.lat, (int)nxt, 64), lon2 = __shfl(m.lon, (int)nxt, 64), cs2 = __shfl(m.cs, (int)nxt, 64);
  const bool hop = in && m.loc && loc2 && nxt != lane;
  const double d = hop ? spread_km(hav_a(m.lat, m.lon, m.cs, lat2, lon2, cs2)) : 0.0;
  const uint32_t hops = (uint32_t)__popcll(__ballot(hop));
  const double ring = wave_sum_f64(d);
  const uint64_t dbits = (uint64_t)__double_as_longlong(d);
  const uint64_t dmax = wave_max_u64(dbits);
  const uint32_t hop_w = wave_min_u32(hop && dbits == dmax ? m.w : 0xFFFFFFFFu);
  if (lane == 0u) spread_store(&a.out[row], located, hops, top, ring, dmax, hop_w);
}

// ---- n > 64: one workgroup per group, for any n (the reference bounds max_group_size nowhere).  A thread owns the members
// tid, tid + 256, ... in turn; for each round of owners the whole group passes through LDS in tiles of 256.  A member's
// place in the ring needs no rank here: its successor is the member with the smallest (addr_rank, worker) key above its
// own, or the group's smallest when there is none — two running minima of the same pass, whatever n is.
constexpr uint32_t SPREAD_TILE = 256;
struct SpreadTile {
  double lat[SPREAD_TILE], lon[SPREAD_TILE], cs[SPREAD_TILE];
  uint32_t w[SPREAD_TILE], rk[SPREAD_TILE], loc[SPREAD_TILE];
};
__global__ __launch_bounds__(256) void group_spread_block_kernel(SpreadArgs a) {
  __shared__ SpreadTile t;
  __shared__ uint64_t s_a[4], s_pair[4], s_hop[4];
  __shared__ double s_ring[4];
  __shared__ uint32_t s_cnt[4][3];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  if (blockIdx.x >= a.n_big) return;  // (uniform)
  const uint32_t row = a.big[blockIdx.x], slot = a.slot_of_row[row];
  const uint32_t n = a.g_n[slot], off = a.g_off[slot];
  SpreadBest best{0ull, ~0ull};
  double ring = 0.0;
  uint64_t hop_bits = 0ull;
  uint32_t hop_w = 0xFFFFFFFFu, located = 0, hops = 0;
  for (uint32_t base = 0; base < n; base += SPREAD_TILE) {  // (uniform: every thread runs every round, owner or not)
    const bool in = base + tid < n;
    const SpreadMember m = spread_member(a, off + base + tid, in);
    const uint64_t key = ((uint64_t)m.rk << 32) | m.w;
    uint64_t succ = ~0ull, first = ~0ull;
    for (uint32_t t0 = 0; t0 < n; t0 += SPREAD_TILE) {
      __syncthreads();  // (the tile's readers of the round before are through)
      const SpreadMember s = spread_member(a, off + t0 + tid, t0 + tid < n);
      t.lat[tid] = s.lat, t.lon[tid] = s.lon, t.cs[tid] = s.cs, t.w[tid] = s.w, t.rk[tid] = s.rk, t.loc[tid] = s.loc;
      __syncthreads();
      const uint32_t cnt = n - t0 < SPREAD_TILE ? n - t0 : SPREAD_TILE;
      if (!in) continue;
      for (uint32_t j = 0; j < cnt; ++j) {  // (every lane reads the same slot: an LDS broadcast)
        const uint32_t wj = t.w[j];
        const uint64_t kj = ((uint64_t)t.rk[j] << 32) | wj;
        first = kj < first ? kj : first;
        succ = (kj > key && kj < succ) ? kj : succ;
        if (m.loc && t.loc[j] && wj != m.w) spread_take(best, hav_a(m.lat, m.lon, m.cs, t.lat[j], t.lon[j], t.cs[j]), m.w, wj);
      }
    }
    if (in && m.loc) {
      ++located;
      const uint32_t nx = (uint32_t)(succ != ~0ull ? succ : first);  // the worker after this one (first: the ring closes)
      if (nx != m.w && nx < a.W && (a.flags[nx] & PM_W_HAS_LOC)) {
        const double d = spread_km(hav_a(m.lat, m.lon, m.cs, a.lat[nx], a.lon[nx], a.coslat[nx]));
        const uint64_t db = (uint64_t)__double_as_longlong(d);
        ++hops;
        ring += d;
        if (db > hop_bits || (db == hop_bits && m.w < hop_w)) hop_bits = db, hop_w = m.w;
      }
    }
  }
  // the waves' results, then the four of them by thread 0 under the same rules
  const bool has = best.pair != ~0ull;
  const uint64_t amax = wave_max_u64(has ? best.a_bits : 0ull);
  const uint64_t pmin = wave_min_u64(has && best.a_bits == amax ? best.pair : ~0ull);
  const uint64_t dmax = wave_max_u64(hops ? hop_bits : 0ull);
  const uint32_t wmin = wave_min_u32(hops && hop_bits == dmax ? hop_w : 0xFFFFFFFFu);
  const double rsum = wave_sum_f64(ring);
  const uint32_t nloc = wave_sum(located), nhop = wave_sum(hops);
  if (lane == 0u) {
    s_a[wave] = amax, s_pair[wave] = pmin, s_hop[wave] = dmax, s_ring[wave] = rsum;
    s_cnt[wave][0] = nloc, s_cnt[wave][1] = nhop, s_cnt[wave][2] = wmin;
  }
  __syncthreads();
  if (tid != 0u) return;
  SpreadBest top{0ull, ~0ull};
  double rg = 0.0;
  uint64_t hb = 0ull;
  uint32_t hw = 0xFFFFFFFFu, nl = 0, nh = 0;
  for (uint32_t k = 0; k < 4u; ++k) {
    if (s_pair[k] != ~0ull &&
        (top.pair == ~0ull || s_a[k] > top.a_bits || (s_a[k] == top.a_bits && s_pair[k] < top.pair)))
      top.a_bits = s_a[k], top.pair = s_pair[k];
    if (s_cnt[k][1] && (s_hop[k] > hb || (s_hop[k] == hb && s_cnt[k][2] < hw))) hb = s_hop[k], hw = s_cnt[k][2];
    rg += s_ring[k];
    nl += s_cnt[k][0], nh += s_cnt[k][1];
  }
  spread_store(&a.out[row], nl, nh, top, rg, hb, hw);
}

// ---- pm_config_spread: grid-stride over the per-group rows; counts, histogram and the integer metre sums through LDS
// atomics, the two maxima as the u64 bit patterns of non-negative doubles (they order like the values); one global atomic
// per non-zero counter per workgroup.
__device__ __forceinline__ uint32_t spread_bucket(double km) {
  return (km >= PM_SPREAD_EDGES_KM[0] ? 1u : 0u) + (km >= PM_SPREAD_EDGES_KM[1] ? 1u : 0u) +
         (km >= PM_SPREAD_EDGES_KM[2] ? 1u : 0u) + (km >= PM_SPREAD_EDGES_KM[3] ? 1u : 0u);
}
__global__ __launch_bounds__(256) void config_spread_kernel(const pm_group_spread_row* __restrict__ rows,
                                                            const uint32_t* __restrict__ row_cfg, uint32_t n_rows,
                                                            uint32_t n_cfgs, SpreadCfgAcc* __restrict__ out) {
  __shared__ SpreadCfgAcc s[PM_MAX_CONFIGS];
  for (uint32_t k = threadIdx.x; k < n_cfgs; k += 256u) s[k] = SpreadCfgAcc{};
  __syncthreads();
  for (uint32_t r = blockIdx.x * 256u + threadIdx.x; r < n_rows; r += gridDim.x * 256u) {
    const uint32_t c = row_cfg[r];
    if (c >= n_cfgs) continue;
    const pm_group_spread_row g = rows[r];
    atomicAdd(&s[c].cnt[SPC_GROUPS], 1u);
    if (g.located >= 2u) {
      atomicAdd(&s[c].cnt[SPC_MEASURED], 1u);
      atomicAdd(&s[c].cnt[SPC_HIST + spread_bucket(g.diameter_km)], 1u);
      atomicMax(&s[c].v[SPV_MAX_DIAMETER], (unsigned long long)__double_as_longlong(g.diameter_km));
      atomicAdd(&s[c].v[SPV_SUM_DIAMETER], (unsigned long long)llrint(g.diameter_km * 1000.0));
    }
    if (g.ring_hops) {
      atomicMax(&s[c].v[SPV_MAX_HOP], (unsigned long long)__double_as_longlong(g.longest_hop_km));
      atomicAdd(&s[c].v[SPV_SUM_RING], (unsigned long long)llrint(g.ring_km * 1000.0));
    }
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < n_cfgs; k += 256u) {
    for (uint32_t j = 0; j < SPC_N; ++j)
      if (s[k].cnt[j]) atomicAdd(&out[k].cnt[j], s[k].cnt[j]);
    if (s[k].v[SPV_MAX_DIAMETER]) atomicMax(&out[k].v[SPV_MAX_DIAMETER], s[k].v[SPV_MAX_DIAMETER]);
    if (s[k].v[SPV_MAX_HOP]) atomicMax(&out[k].v[SPV_MAX_HOP], s[k].v[SPV_MAX_HOP]);
    if (s[k].v[SPV_SUM_DIAMETER]) atomicAdd(&out[k].v[SPV_SUM_DIAMETER], s[k].v[SPV_SUM_DIAMETER]);
    if (s[k].v[SPV_SUM_RING]) atomicAdd(&out[k].v[SPV_SUM_RING], s[k].v[SPV_SUM_RING]);
  }
}

void launch_group_spread(const SpreadArgs& a, hipStream_t s) {
  if (a.n_small) hipLaunchKernelGGL(group_spread_wave_kernel, dim3((a.n_small + 3u) / 4u), dim3(256), 0, s, a);
  if (a.n_big) hipLaunchKernelGGL(group_spread_block_kernel, dim3(a.n_big), dim3(256), 0, s, a);
}
void launch_config_spread(const pm_group_spread_row* rows, const uint32_t* row_cfg, uint32_t n_rows, uint32_t n_cfgs,
                          SpreadCfgAcc* out, uint32_t max_blocks, hipStream_t s) {
  if (!n_rows || !n_cfgs) return;
  hipLaunchKernelGGL(config_spread_kernel, dim3(report_blocks(n_rows, max_blocks)), dim3(256), 0, s, rows, row_cfg, n_rows,
                     n_cfgs, out);
}
