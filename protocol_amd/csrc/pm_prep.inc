// pm_prep.inc — full-chip list preparation (included by pm_kernels.hip inside namespace pm): the next candidate list
// of the batch pipeline (carve_prep_*), the ordered eligible list (carve_elig_*), the spatial index of its positions
// (cell_*).  Reference: the filter at node_groups/mod.rs:492-519.
// ------------------------------------------------------------------------------------------------
// Full-chip preparation of the next candidate list (proposal-driven FORM carve).  The validator is one
// workgroup; compacting a 100 k-entry eligible list (and scattering group_of for the groups it just formed) on
// one CU took a third of its time.  Between two validation launches run, on every CU:
//   carve_prep_count_kernel   group_of for the groups of the last launch; per block, per remaining configuration,
//                             the number of live compatible positions (+ global totals); clears the slot loc bitmap
//   carve_prep_place_kernel   every block picks the same next configuration from the totals (mod.rs:505-519: the
//                             first whose loop would be entered), derives its offset from the per-block counts
//                             and places its candidates (stable: slot order = input order); the block that
//                             finishes last computes the proposal batch (prop_limit_scan) and publishes the status
// One 64-position word per wave, four waves per block.

#define PREP_WAVES 4

// The plan of a preparation, decided once (one thread) so that every block of the two kernels works on the same
// configuration: where the search for the next configuration starts — the carve's own state.
__device__ __forceinline__ void plan_batch(const CarveArgs& p) {  // (one thread)
  BatchDesc d = {};
  d.planned = 1u;
  d.ci0 = p.status->cur_ci;
  d.total_available = p.status->total_available;
  *p.desc = d;
}

__global__ __launch_bounds__(256) void carve_prep_count_kernel(const CarveArgs* __restrict__ pa) {
  const CarveArgs& p = *pa;
  const auto st = G(p.status);
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t wave_g = blockIdx.x * PREP_WAVES + wave;
  {
    // group_of for the groups the last validation launch appended (idempotent; also runs after the carve ended)
    const uint32_t g_lo = st->g_lo, g_hi = st->g_hi, n_waves = gridDim.x * PREP_WAVES;
    for (uint32_t g = g_lo + wave_g; g < g_hi; g += n_waves) {
      const uint32_t off = G(p.g_off)[g], gn = G(p.g_n)[g];
      for (uint32_t k = lane; k < gn; k += 64u) G(p.group_of)[G(p.members)[off + k]] = (int32_t)g;
    }
  }
  if (st->state != CARVE_STATE_RUNNING) {
    if (blockIdx.x == 0 && tid == 0) p.desc->planned = 0u;
    return;
  }
  PM_BLOG(if (blockIdx.x == 0 && tid == 0) p.status->prof[5] = ~0ull;)  // (earliest block start of the placement behind this)
  // (one batch at a time: the plan is the carve's own state, the same in every block)
  const uint32_t ci0 = st->cur_ci;
  if (blockIdx.x == 0 && tid == 0) plan_batch(p);
  if (ci0 >= p.n_avail) return;
  __shared__ uint32_t s_cnt[PREP_WAVES][PM_MAX_CONFIGS];
  const uint32_t n = st->n_eligible, n_words = (n + 63u) >> 6;
  const uint32_t j = wave_g;  // this wave's word of the position space
  uint64_t m = 0;
  if (j < n_words) {
    const uint32_t i = j * 64u + lane;
    const uint64_t aw = G(p.alive_g)[j];
    const bool alive = i < n && ((aw >> lane) & 1ull);
    m = alive ? G((const uint64_t*)p.c_compat)[i] : 0ull;
    if (lane == 0) {
      G(p.alive_snap)[j] = aw;
      G(p.bits_scratch)[p.bits_stride + j] = 0ull;  // slot loc bitmap: the placement ORs its bits in
    }
  }
  for (uint32_t ci = ci0; ci < p.n_avail; ++ci) {
    const uint32_t cnt = (uint32_t)__popcll(__ballot((m >> p.avail_cfg[ci]) & 1ull));
    if (lane == 0) s_cnt[wave][ci] = cnt;
  }
  __syncthreads();
  if (tid >= ci0 && tid < p.n_avail) {
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t w = 0; w < PREP_WAVES; ++w) sum += s_cnt[w][tid];
    G(p.prep_block_counts)[(size_t)blockIdx.x * PM_MAX_CONFIGS + tid] = sum;
    if (sum) atomicAdd(&p.prep_counts[tid], sum);
  }
}

__global__ __launch_bounds__(256) void carve_prep_place_kernel(const CarveArgs* __restrict__ pa) {
  const CarveArgs& p = *pa;
  const auto st = G(p.status);
  const auto D = G((const BatchDesc*)p.desc);
  if (st->state != CARVE_STATE_RUNNING || !D->planned) return;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  __shared__ uint32_t s_red[PREP_WAVES + 4];
  __shared__ uint32_t s_bits[PREP_WAVES][64];
  PM_BLOG(const uint64_t pl_t0 = PM_TICKS(); if (tid == 0) atomicMin((unsigned long long*)&p.status->prof[5], (unsigned long long)pl_t0);)
  const uint32_t n = st->n_eligible, n_words = (n + 63u) >> 6;
  const uint32_t total_available = D->total_available;
  // ---- the next configuration whose loop would be entered (mod.rs:505-519), the same in every block.  (Counts and
  // total_available only ever shrink: a configuration that cannot be entered by these numbers cannot be entered by
  // the validator's either, so skipping it is final.)
  uint32_t ci = D->ci0, n_list = 0;
  for (; ci < p.n_avail; ++ci) {
    const uint32_t min_s = p.min_size[ci];
    if (total_available < min_s) continue;             // `while` never entered (:507)
    n_list = G((const uint32_t*)p.prep_counts)[ci];
    if (n_list < min_s || n_list == 0) continue;       // :517-519
    break;
  }
  const bool none = ci >= p.n_avail;
  // proposals for this list?  (the configuration and the list length decide: the same answer in every block) ...
  const bool props = !none && p.proximity && n_list <= PM_CARVE_BIG_SLOTS && p.max_size[ci] - 1u < PM_PROP_KMAX &&
                     !(p.debug_mem_above && n_list > p.debug_mem_above);
  // ... and do they walk the spatial index?  A walk visits the indexed positions around the seed whether they are
  // still candidates or not, the sweep visits the n_list candidates: the walk pays while the list is long and a good
  // part of the index is still in it.
  uint32_t cell_g = props ? st->cell_g : 0u;
  if (cell_g && p.prune_mode == 1u && (uint64_t)n_list * n_list < (uint64_t)p.prune_factor * st->n_indexed) cell_g = 0u;
  if (!none) {
    const uint64_t cbit = 1ull << p.avail_cfg[ci];
    // ---- this block's first slot: candidates of the blocks in front of it
    uint32_t part = 0;
    for (uint32_t b = tid; b < blockIdx.x; b += 256u) part += G((const uint32_t*)p.prep_block_counts)[(size_t)b * PM_MAX_CONFIGS + ci];
    part = wave_sum(part);
    if (lane == 0) s_red[wave] = part;
    // ---- this wave's word: candidates, their ranks
    const uint32_t j = blockIdx.x * PREP_WAVES + wave;
    const uint32_t i = j * 64u + lane;
    const uint32_t ic = i < n ? i : (n ? n - 1u : 0u);
    const uint64_t aw = j < n_words ? G((const uint64_t*)p.alive_snap)[j] : 0ull;
    const uint64_t lg = j < n_words ? G(p.loc_g)[j] : 0ull;
    const uint64_t cm = n ? G((const uint64_t*)p.c_compat)[ic] : 0ull;
    const uint32_t ow = n ? G(p.order)[ic] : 0u;
    const uint32_t os = n ? G(p.c_site)[ic] : 0u;
    const double la = n ? G(p.c_lat)[ic] : 0.0, lo = n ? G(p.c_lon)[ic] : 0.0, co = n ? G(p.c_cos)[ic] : 0.0;
    const double vx = n ? G(p.c_ux)[ic] : 0.0, vy = n ? G(p.c_uy)[ic] : 0.0, vz = n ? G(p.c_uz)[ic] : 0.0;
    const bool c = i < n && ((aw >> lane) & 1ull) && (cm & cbit) != 0ull;
    const uint64_t bal = __ballot(c);
    const uint32_t cnt = (uint32_t)__popcll(bal);
    if (lane == 0) s_red[PREP_WAVES + wave] = cnt;
    __syncthreads();
    PM_BLOG(if (tid == 0) atomicAdd((unsigned long long*)&p.status->prof[14], (unsigned long long)(PM_TICKS() - pl_t0));)  // loads in
    uint32_t off = 0;
#pragma unroll
    for (uint32_t w = 0; w < PREP_WAVES; ++w) off += s_red[w];
    for (uint32_t w = 0; w < wave; ++w) off += s_red[PREP_WAVES + w];
    const uint32_t rank = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
    const uint32_t has_loc = (uint32_t)(lg >> lane) & 1u;
    if (c) {
      const uint32_t s = off + rank;
      G(p.slot_pos)[s] = i | (has_loc << 31);  // bit 31: has a location
      G(p.slot_wid)[s] = ow;
      G(p.cc_lat)[s] = la;
      G(p.cc_lon)[s] = lo;
      G(p.cc_cos)[s] = co;
      G(p.cc_ux)[s] = vx;
      G(p.cc_uy)[s] = vy;
      G(p.cc_uz)[s] = vz;
      G(p.cc_site)[s] = os;
      s_bits[wave][rank] = has_loc;
    }
    if (cell_g && i < n && has_loc) G(p.cs_slot)[G((const uint32_t*)p.cs_of_pos)[i]] = c ? off + rank : 0xFFFFFFFFu;
    // the located bits of this wave's slots [off, off + cnt): compacted by rank, ORed into the slot loc bitmap
    // (cleared by carve_prep_count_kernel); at most two words
    __syncthreads();
    const uint64_t locm = __ballot(lane < cnt && s_bits[wave][lane] != 0u);
    if (lane == 0 && locm) {
      const auto loc = (unsigned long long*)(p.bits_scratch + p.bits_stride);
      const uint32_t sh = off & 63u;
      atomicOr(&loc[off >> 6], (unsigned long long)(locm << sh));
      if (sh && (locm >> (64u - sh))) atomicOr(&loc[(off >> 6) + 1u], (unsigned long long)(locm >> (64u - sh)));
    }
  }
  // ---- the block that finishes last completes the list and publishes it
  PM_BLOG(if (tid == 0) atomicAdd((unsigned long long*)&p.status->prof[15], (unsigned long long)(PM_TICKS() - pl_t0));)  // stores issued
  // What the last block reads of the others is the slot loc bitmap, and that is written with device-scope atomics
  // only: they need no release, just to have been performed before this block's ticket is taken — which a wait for
  // the wave's outstanding memory operations gives (workgroup-scope fence: s_waitcnt, no cache maintenance).  The
  // column stores are for the kernels behind this one; the end of the kernel releases them.  (A device-scope fence
  // here writes the XCD's L2 back once per BLOCK: 25 of the 42 us this kernel took at 100 k positions.)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __syncthreads();
  BLOG_BLOCK_TICKET(pl_t0);  // this block, start to ticket
  if (tid == 0) s_red[0] = atomicAdd(&p.prep_counts[PM_MAX_CONFIGS], 1u);
  __syncthreads();
  if (s_red[0] != gridDim.x - 1u) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // (see what the other blocks' atomics wrote: invalidate, nothing to write back)
  PM_BLOG(const uint64_t pl_t1 = PM_TICKS();)  // every block is through: the tail begins
  if (none) {
    if (tid == 0) {
      p.desc->ci = p.n_avail;
      p.desc->none = 1u;
      BLOG_LINE_NONE();
    }
    return;
  }
  const uint32_t lw = (n_list + 63u) >> 6;
  const auto alive = G(p.bits_scratch);
  for (uint32_t w = tid; w < lw; w += 256u)  // slot alive bitmap: every slot of the fresh list
    alive[w] = (w + 1u < lw || (n_list & 63u) == 0u) ? ~0ull : ((1ull << (n_list & 63u)) - 1ull);
  __syncthreads();  // (the scan below reads them back: same workgroup, the barrier's own fence is enough)
  uint32_t prop_k = 0, limit = 0, n_seeds = 0;
  const uint32_t max_s = p.max_size[ci];
  if (props) {
    const uint32_t k = max_s - 1u + PM_PROP_RESERVE;
    prop_k = k < PM_PROP_KMAX ? k : PM_PROP_KMAX;
    if (wave == 0) {
      prop_limit_scan(p, n_list, lane, &limit, &n_seeds, cell_g != 0u);
      if (lane == 0) {
        s_red[1] = limit;
        s_red[2] = n_seeds;
      }
    }
    __syncthreads();  // (uniform: prop_k depends on the configuration only)
    limit = s_red[1];
    n_seeds = s_red[2];
    prop_seed_slots(p, limit, tid, 256u);
  }
  if (tid == 0) {
    BatchDesc* d = p.desc;
    d->ci = ci;
    d->n_list = n_list;
    d->prop_k = prop_k;
    d->prop_limit = limit;
    d->n_seeds = n_seeds;
    d->cell_g = cell_g;
    d->valid = 1u;
    if (cell_g) p.status->pruned_batches += 1u;
    BLOG_PLACED(pl_t1);
    BLOG_LINE(n_list, n_seeds, cell_g);
  }
}

// ------------------------------------------------------------------------------------------------
// Full-chip construction of the ordered eligible list at the start of a proposal-driven FORM carve (the INIT launch
// of the validator did this on one CU: 0.5 ms at 100 k rows, and a tenth of an incremental tick that adds a few
// hundred workers to a standing swarm).  Same two-step shape as the list preparation above:
//   carve_elig_count_kernel   eligible rows (Healthy & p2p & unassigned, mod.rs:492-497) per block; clears loc_g
//   carve_elig_place_kernel   stable placement (position order = row order), the position-indexed columns, the
//                             loc bitmap; the block that finishes last writes the alive bitmap and the status
// One 64-row word per wave, four waves per block.

__device__ __forceinline__ bool row_eligible(const CarveArgs& p, uint32_t w) {
  if (w >= p.W) return false;
  const uint32_t f = G(p.wflags)[w];
  return (f & PM_W_HEALTHY) && (f & PM_W_HAS_P2P) && G(p.group_of)[w] < 0;
}

__device__ __forceinline__ void carve_elig_count_body(const CarveArgs& p, uint32_t fresh, uint32_t n_groups0, uint32_t n_members0) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  // A fresh carve: this launch IS the initialisation of the status block (no other block of it reads the block; the
  // kernels behind it do) — a host-to-device copy and a fill in front of every carve otherwise, 4 us of queue each.
  // The streaming carve's control words likewise (every launch of the sequence, fresh or re-armed, starts them at zero).
  if (blockIdx.x == 0) {
    if (fresh) {
      uint32_t* w = (uint32_t*)p.status;
      for (uint32_t k = tid; k < (uint32_t)(sizeof(CarveStatus) / 4u); k += 256u) w[k] = 0u;
    }
    if (p.stream && tid < PM_STREAM_CTL_WORDS) p.stream_ctl[tid] = 0u;
    __syncthreads();
    if (fresh && tid == 0) {
      p.status->state = CARVE_STATE_RUNNING;
      p.status->n_groups = n_groups0;
      p.status->n_members = n_members0;
    }
  }
  if (!fresh && G(p.status)->state != CARVE_STATE_RUNNING) return;
  __shared__ uint32_t s_c[PREP_WAVES];
  const uint32_t j = blockIdx.x * PREP_WAVES + wave;
  const uint64_t bal = __ballot(row_eligible(p, j * 64u + lane));
  if (lane == 0) {
    s_c[wave] = (uint32_t)__popcll(bal);
    if (j < ((p.W + 63u) >> 6)) G(p.loc_g)[j] = 0ull;  // (the positions are a subset of the rows)
  }
  // (streaming carve: the per-configuration bitmaps of compatible positions, ORed in by the placement)
  if (p.stream && lane < p.n_avail && j < ((p.W + 63u) >> 6)) G(p.cfgbits)[(size_t)lane * p.bits_stride + j] = 0ull;
  if (blockIdx.x == 0 && tid <= PM_MAX_CONFIGS + 1u) p.prep_counts[tid] = 0u;  // totals and both tickets
  __syncthreads();
  if (tid == 0) {
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t w = 0; w < PREP_WAVES; ++w) sum += s_c[w];
    G(p.prep_block_counts)[(size_t)blockIdx.x * PM_MAX_CONFIGS] = sum;
  }
}
__global__ __launch_bounds__(256) void carve_elig_count_kernel(const CarveArgs* __restrict__ pa, uint32_t fresh, uint32_t n_groups0,
                                                               uint32_t n_members0) {
  carve_elig_count_body(*pa, fresh, n_groups0, n_members0);
}
// The same with the carve's argument block as its OWN argument: the first kernel of a launch sequence reads the block from
// the launch packet's kernarg segment and its first workgroup stores it where the kernels behind it read it — no
// host-to-device copy (a launch of the runtime's copy kernel with 17 us of an idle GPU in front and 7 behind, profiles/
// r06_timeline.txt) and no launch of its own for the block.
struct CarveArgWords {
  uint32_t w[(sizeof(CarveArgs) + 3u) / 4u];
};
static_assert(sizeof(CarveArgWords) + 32u <= 4096u, "the argument block fits a kernarg segment");
static_assert(sizeof(CarveArgWords) == sizeof(CarveArgs), "the block is whole words");
__global__ __launch_bounds__(256) void carve_elig_count_put_kernel(CarveArgWords a, uint32_t* __restrict__ dst, uint32_t fresh,
                                                                   uint32_t n_groups0, uint32_t n_members0) {
  if (blockIdx.x == 0)
    for (uint32_t i = threadIdx.x; i < sizeof(CarveArgWords) / 4u; i += 256u) dst[i] = a.w[i];
  carve_elig_count_body(reinterpret_cast<const CarveArgs&>(a), fresh, n_groups0, n_members0);
}

__global__ __launch_bounds__(256) void carve_elig_place_kernel(const CarveArgs* __restrict__ pa, uint32_t start_ci) {
  const CarveArgs& p = *pa;
  const auto st = G(p.status);
  if (st->state != CARVE_STATE_RUNNING) return;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  __shared__ uint32_t s_red[2 * PREP_WAVES + 2];
  __shared__ uint32_t s_bits[PREP_WAVES][64];
  __shared__ uint64_t s_cm[PREP_WAVES][64];
  // ---- this block's first position: eligible rows of the blocks in front of it
  uint32_t part = 0;
  for (uint32_t b = tid; b < blockIdx.x; b += 256u) part += G((const uint32_t*)p.prep_block_counts)[(size_t)b * PM_MAX_CONFIGS];
  part = wave_sum(part);
  if (lane == 0) s_red[wave] = part;
  const uint32_t w = (blockIdx.x * PREP_WAVES + wave) * 64u + lane;
  const bool e = row_eligible(p, w);
  const uint64_t bal = __ballot(e);
  const uint32_t cnt = (uint32_t)__popcll(bal);
  if (lane == 0) s_red[PREP_WAVES + wave] = cnt;
  __syncthreads();
  uint32_t off = 0;
#pragma unroll
  for (uint32_t k = 0; k < PREP_WAVES; ++k) off += s_red[k];
  for (uint32_t k = 0; k < wave; ++k) off += s_red[PREP_WAVES + k];
  const uint32_t rank = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
  if (e) {
    const uint32_t i = off + rank;
    const uint32_t has_loc = (G(p.wflags)[w] & PM_W_HAS_LOC) ? 1u : 0u;
    G(p.order)[i] = w;
    G(p.c_lat)[i] = G(p.lat)[w];
    G(p.c_lon)[i] = G(p.lon)[w];
    G(p.c_cos)[i] = G(p.coslat)[w];
    G(p.c_ux)[i] = G(p.ux)[w];
    G(p.c_uy)[i] = G(p.uy)[w];
    G(p.c_uz)[i] = G(p.uz)[w];
    G(p.c_site)[i] = G(p.site)[w];
    if (p.stream) pack_store(p.c_pack, i, G(p.ux)[w], G(p.uy)[w], G(p.uz)[w], G(p.site)[w], has_loc);
    const uint64_t cmw = G(p.compat)[w];
    G(p.c_compat)[i] = cmw;
    s_bits[wave][rank] = has_loc;
    s_cm[wave][rank] = cmw;
  }
  // the located bits of this wave's positions [off, off + cnt): compacted by rank, ORed into loc_g (at most two words)
  __syncthreads();
  const uint64_t locm = __ballot(lane < cnt && s_bits[wave][lane] != 0u);
  if (lane == 0 && locm) {
    const auto loc = (unsigned long long*)p.loc_g;
    const uint32_t sh = off & 63u;
    atomicOr(&loc[off >> 6], (unsigned long long)(locm << sh));
    if (sh && (locm >> (64u - sh))) atomicOr(&loc[(off >> 6) + 1u], (unsigned long long)(locm >> (64u - sh)));
  }
  if (p.stream) {  // the same for every configuration of the carve order: which of these positions are compatible
    const uint64_t cmr = lane < cnt ? s_cm[wave][lane] : 0ull;
    const uint32_t sh = off & 63u;
    for (uint32_t ci = 0; ci < p.n_avail; ++ci) {
      const uint64_t bits = __ballot((cmr >> p.avail_cfg[ci]) & 1ull);
      if (lane == 0 && bits) {
        const auto cb = (unsigned long long*)(p.cfgbits + (size_t)ci * p.bits_stride);
        atomicOr(&cb[off >> 6], (unsigned long long)(bits << sh));
        if (sh && (bits >> (64u - sh))) atomicOr(&cb[(off >> 6) + 1u], (unsigned long long)(bits >> (64u - sh)));
      }
    }
  }
  // ---- the block that finishes last completes the list and publishes it (it reads nothing the other blocks wrote
  // but the ticket: see carve_prep_place_kernel for why this is not a device-scope fence)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __syncthreads();
  if (tid == 0) s_red[0] = atomicAdd(&p.prep_counts[PM_MAX_CONFIGS + 1u], 1u);
  __syncthreads();
  if (s_red[0] != gridDim.x - 1u) return;
  __threadfence();
  uint32_t total = 0;
  for (uint32_t b = tid; b < gridDim.x; b += 256u) total += G((const uint32_t*)p.prep_block_counts)[(size_t)b * PM_MAX_CONFIGS];
  total = wave_sum(total);
  __syncthreads();
  if (lane == 0) s_red[1u + wave] = total;
  __syncthreads();
  const uint32_t n = s_red[1] + s_red[2] + s_red[3] + s_red[4];
  const uint32_t n_words = (n + 63u) >> 6;
  for (uint32_t j = tid; j < n_words; j += 256u) {
    const uint64_t all = (j + 1u < n_words || (n & 63u) == 0u) ? ~0ull : ((1ull << (n & 63u)) - 1ull);
    G(p.alive_g)[j] = all;
    if (p.stream) G(p.bits_scratch)[j] = all;  // (streaming carve: the published copy of "what no group holds yet")
  }
  if (tid <= PM_MAX_CONFIGS + 1u) p.prep_counts[tid] = 0u;  // totals + tickets of the first list preparation
  if (tid == 0) {
    st->n_eligible = n;
    st->total_available = n;  // mod.rs:503
    st->cur_ci = start_ci;
    st->g_lo = st->g_hi = st->n_groups;
  }
}

// ------------------------------------------------------------------------------------------------
// Spatial index of the carve's located positions (see cell_walk).  Positions never move during a carve — only the
// candidate lists drawn from them do — so the index is built once, behind the eligible list: a counting sort by grid
// cell of the unit vectors.
//   cell_count_kernel   every located position: its cell, and its rank among the cell's members (one atomic)
//   cell_scan_*_kernel  exclusive scan of the G^3 counts -> cell_start; leaves the counts zero
//   cell_place_kernel   position -> entry; the entry's unit vector and site, in cell order
// Per batch, carve_prep_place_kernel then writes the slot every entry has in the prepared list (cs_slot, ~0 = none).
__global__ __launch_bounds__(256) void cell_count_kernel(const CarveArgs* __restrict__ pa) {
  const CarveArgs& p = *pa;
  const auto st = G(p.status);
  if (st->state != CARVE_STATE_RUNNING) return;
  const uint32_t n = st->n_eligible;
  const bool forced = p.prune_mode >= 2u;  // (modes 2, 3: an index for any swarm; mode 1: where it pays, PM_CELL_AUTO_N)
  const uint32_t g = (p.prune_mode && p.proximity && (forced || n >= PM_CELL_AUTO_N))
                         ? cell_g_for(forced && n >= 64u && n < PM_CELL_MIN_N ? PM_CELL_MIN_N : n) : 0u;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    st->cell_g = g;
    st->n_indexed = 0u;
  }
  if (!g) return;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  if (!bit_at(G((const uint64_t*)p.loc_g), i)) {
    G(p.pos_cell)[i] = 0xFFFFFFFFu;
    return;
  }
  const uint32_t c = (cell_coord(G(p.c_uz)[i], g) * g + cell_coord(G(p.c_uy)[i], g)) * g + cell_coord(G(p.c_ux)[i], g);
  G(p.pos_cell)[i] = c;
  G(p.pos_rank)[i] = atomicAdd(&p.cell_cnt[c], 1u);
}

// the scan, on every CU: 1024 counts per block.  (A single workgroup took 230 us for the 262,144 cells of the 64^3 grid.)
//   cell_scan_sums_kernel   the sum of every block's counts; the block that finishes last turns the sums into offsets
//   cell_scan_apply_kernel  every block scans its own counts from its offset, and leaves the counts zero behind it
#define CELL_SCAN_PER_BLOCK 1024u
static_assert((PM_CELL_TABLE + CELL_SCAN_PER_BLOCK - 1u) / CELL_SCAN_PER_BLOCK <= 320u, "block sums fit one look of 256 + 64 threads");
__global__ __launch_bounds__(256) void cell_scan_sums_kernel(const CarveArgs* __restrict__ pa) {
  const CarveArgs& p = *pa;
  const auto st = G(p.status);
  if (st->state != CARVE_STATE_RUNNING) return;
  const uint32_t g = st->cell_g;
  if (!g) return;
  const uint32_t total = g * g * g, n_blocks = (total + CELL_SCAN_PER_BLOCK - 1u) / CELL_SCAN_PER_BLOCK;
  if (blockIdx.x >= n_blocks) return;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  __shared__ uint32_t s_w[4];
  __shared__ uint32_t s_last;
  const auto cnt = G((const uint32_t*)p.cell_cnt);
  const uint32_t i0 = blockIdx.x * CELL_SCAN_PER_BLOCK + tid * 4u;
  uint32_t v = 0;
#pragma unroll
  for (uint32_t k = 0; k < 4u; ++k) v += i0 + k < total ? cnt[i0 + k] : 0u;
  v = wave_sum(v);
  if (lane == 0) s_w[wave] = v;
  __syncthreads();
  // the sums and the ticket live behind the starts (cell_start has PM_CELL_TABLE words, the table needs total + 1)
  const auto blk = p.cell_start + PM_CELL_TABLE;  // [320] sums -> offsets, [320] ticket
  if (tid == 0) {
    blk[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    __threadfence();
    s_last = atomicAdd(&blk[320], 1u) == n_blocks - 1u ? 1u : 0u;
  }
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  // exclusive scan of up to 320 block sums by wave 0: five strides of 64
  if (wave == 0) {
    uint32_t carry = 0;
    for (uint32_t c0 = 0; c0 < n_blocks; c0 += 64u) {
      const uint32_t c = c0 + lane;
      const uint32_t x = c < n_blocks ? G((const uint32_t*)blk)[c] : 0u;
      const uint32_t incl = wave_incl_scan_u32(x);
      if (c < n_blocks) blk[c] = carry + incl - x;
      carry += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    }
    if (lane == 0) {
      blk[320] = 0u;  // the ticket, for the next carve
      p.cell_start[total] = carry;
      st->n_indexed = carry;
    }
  }
}
__global__ __launch_bounds__(256) void cell_scan_apply_kernel(const CarveArgs* __restrict__ pa) {
  const CarveArgs& p = *pa;
  const auto st = G((const CarveStatus*)p.status);
  if (st->state != CARVE_STATE_RUNNING) return;
  const uint32_t g = st->cell_g;
  if (!g) return;
  const uint32_t total = g * g * g, n_blocks = (total + CELL_SCAN_PER_BLOCK - 1u) / CELL_SCAN_PER_BLOCK;
  if (blockIdx.x >= n_blocks) return;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  __shared__ uint32_t s_w[4];
  const auto cnt = G(p.cell_cnt);
  const auto start = G(p.cell_start);
  const uint32_t i0 = blockIdx.x * CELL_SCAN_PER_BLOCK + tid * 4u;
  uint32_t v[4];
#pragma unroll
  for (uint32_t k = 0; k < 4u; ++k) v[k] = i0 + k < total ? cnt[i0 + k] : 0u;
  const uint32_t mine = v[0] + v[1] + v[2] + v[3];
  const uint32_t incl = wave_incl_scan_u32(mine);
  if (lane == 63u) s_w[wave] = incl;
  __syncthreads();
  uint32_t run = G((const uint32_t*)(p.cell_start + PM_CELL_TABLE))[blockIdx.x] + incl - mine;
  for (uint32_t w = 0; w < wave; ++w) run += s_w[w];
#pragma unroll
  for (uint32_t k = 0; k < 4u; ++k) {
    if (i0 + k < total) {
      start[i0 + k] = run;
      cnt[i0 + k] = 0u;
    }
    run += v[k];
  }
}

__global__ __launch_bounds__(256) void cell_place_kernel(const CarveArgs* __restrict__ pa) {
  const CarveArgs& p = *pa;
  const auto st = G((const CarveStatus*)p.status);
  if (st->state != CARVE_STATE_RUNNING || !st->cell_g) return;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= st->n_eligible) return;
  const uint32_t c = G((const uint32_t*)p.pos_cell)[i];
  if (c == 0xFFFFFFFFu) {
    G(p.cs_of_pos)[i] = 0xFFFFFFFFu;
    return;
  }
  const uint32_t e = G((const uint32_t*)p.cell_start)[c] + G((const uint32_t*)p.pos_rank)[i];
  G(p.cs_of_pos)[i] = e;
  if (p.stream) {
    G(p.cs_slot)[e] = i;  // (streaming carve: slot == position, for the whole carve)
    pack_store(p.cs_pack, e, G((const double*)p.c_ux)[i], G((const double*)p.c_uy)[i], G((const double*)p.c_uz)[i],
               G((const uint32_t*)p.c_site)[i], 1u);
  }
  G(p.cs_ux)[e] = G((const double*)p.c_ux)[i];
  G(p.cs_uy)[e] = G((const double*)p.c_uy)[i];
  G(p.cs_uz)[e] = G((const double*)p.c_uz)[i];
  G(p.cs_site)[e] = G((const uint32_t*)p.c_site)[i];
}


// ------------------------------------------------------------------------------------------------
// The merge pass through the streaming carve (pm_engine.cpp run_merge): the eligible list is SUPPLIED — the nodes of the
// compatible solo groups in group-id order (p.order, n_order entries) — and there is one configuration, which every
// entry is compatible with.  One launch: the position-indexed columns, the gather records, the bitmaps (located, the
// configuration's candidates = every position, the validator's master copy and the published one) and a fresh status
// block; carve_stream_kernel comes right behind it.  One 64-position word per wave.
__global__ __launch_bounds__(256) void merge_place_kernel(const CarveArgs* __restrict__ pa, uint32_t n_groups0, uint32_t n_members0,
                                                          uint32_t steps0) {
  const CarveArgs& p = *pa;
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t n = p.n_order, n_words = (n + 63u) >> 6;
  if (blockIdx.x == 0) {
    uint32_t* w = (uint32_t*)p.status;
    for (uint32_t k = tid; k < (uint32_t)(sizeof(CarveStatus) / 4u); k += 256u) w[k] = 0u;
    if (tid < PM_STREAM_CTL_WORDS) p.stream_ctl[tid] = 0u;
    __syncthreads();
    if (tid == 0) {
      p.status->state = CARVE_STATE_RUNNING;
      p.status->n_groups = n_groups0;
      p.status->n_members = n_members0;
      p.status->steps_total = steps0;
      p.status->n_eligible = n;
      p.status->total_available = n;
      p.status->g_lo = p.status->g_hi = n_groups0;
    }
  }
  const uint32_t i = blockIdx.x * 256u + tid;
  bool has_loc = false;
  if (i < n) {
    const uint32_t w = G(p.order)[i];
    has_loc = (G(p.wflags)[w] & PM_W_HAS_LOC) != 0u;
    G(p.c_lat)[i] = G(p.lat)[w];
    G(p.c_lon)[i] = G(p.lon)[w];
    G(p.c_cos)[i] = G(p.coslat)[w];
    G(p.c_ux)[i] = G(p.ux)[w];
    G(p.c_uy)[i] = G(p.uy)[w];
    G(p.c_uz)[i] = G(p.uz)[w];
    G(p.c_site)[i] = G(p.site)[w];
    G(p.c_compat)[i] = G(p.compat)[w];
    pack_store(p.c_pack, i, G(p.ux)[w], G(p.uy)[w], G(p.uz)[w], G(p.site)[w], has_loc ? 1u : 0u);
  }
  const uint64_t bl = __ballot(has_loc), ba = __ballot(i < n);
  const uint32_t j = i >> 6;
  if (lane == 0 && j < n_words) {
    G(p.loc_g)[j] = bl;
    G(p.cfgbits)[j] = ba;       // (configuration 0 of 1: every position)
    G(p.alive_g)[j] = ba;       // the validator's master bitmap
    G(p.bits_scratch)[j] = ba;  // the published one
  }
}
