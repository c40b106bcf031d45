// pm_validate.inc — the validator's building blocks (included by pm_kernels.hip inside namespace pm): the LDS layout and
// wave helpers of the carve, the three-wave chain through LDS rings (producer, collector, chain), carve_fast_steps,
// carve_exact_step and the all-in-HBM path for lists beyond the LDS scheme.  Reference: node_groups/mod.rs:478-628.
// ------------------------------------------------------------------------------------------------
// Carve kernel: the sequential part of the greedy group formation inside ONE workgroup (8 waves).  The
// greedy is a chain of dependent steps (group g+1's seed depends on what group g removed), so there is no
// cross-workgroup traffic to pay for: candidates are position-compacted, the alive/candidate bitmaps live
// in LDS.  The exact form of a step is
//   seed search (bitmap scan) -> Haversine term for every remaining candidate -> top-(max-1)
//   selection by (key, position) with a wavefront argmin staged through LDS -> commit;
// almost every step is instead served from the neighbour lists carve_propose_kernel computed on the whole
// chip (carve_chain / carve_fast_steps below), which only have to be filtered against the bitmap.
//
// Ordering key.  The reference sorts by d = 6371 * 2 * atan2(sqrt(a), sqrt(1-a)) computed with glibc
// libm (mod.rs:218-231).  d is a monotone function of a, so the kernel orders by a (f64, polynomial sin: sin_band)
// and proves the selection equal to the reference's: if every candidate whose a lies within a
// relative 2^-36 band around the last selected one has bit-identical coordinates (then the
// reference's distances tie exactly and the stable sort falls back to input order, like the
// kernel's (key, position) order), the selected SET is the reference's.  Otherwise the step is
// reported as UNCERTAIN and the engine settles exactly that step on the host with glibc.

// (16 waves compile — the whole kernel then has to fit 128 VGPRs: 103 spilled — and were measured in round 2, with the
// speculative rounds of that round: carve 3.57 ms instead of 2.47 at 100k x 10k, 24.3 instead of 19.2 ms at 1M x 100k)
#ifndef CARVE_WAVES
#define CARVE_WAVES 8
#endif
#define CARVE_THREADS (CARVE_WAVES * 64)
// a value that is the same in every lane, moved to an SGPR
#define UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
// an LDS address as an opaque SGPR value (wave-uniform by construction): the compiler can neither re-derive it nor
// treat it as a vector value
template <typename LP, typename GP>
__device__ __forceinline__ LP lds_pin(GP* g) {
  LP p = (LP)g;
  uint32_t a = (uint32_t)(uintptr_t)p;
  a = (uint32_t)__builtin_amdgcn_readfirstlane((int)a);
  asm volatile("" : "+s"(a));
  return (LP)(uintptr_t)a;
}
// The carve kernels take their argument block through a pointer (see carve_kernel), so the compiler cannot
// see that the pointers inside it are global memory and would emit FLAT accesses — which count against the
// LDS counter as well and serialise every LDS wait behind the outstanding HBM traffic.  G() restores the
// address space at the point of use.
template <typename T>
__device__ __forceinline__ __attribute__((address_space(1))) T* G(T* q) {
  return (__attribute__((address_space(1))) T*)q;
}
// 32-byte gather records {ux, uy, uz, site | located << 32} (CarveArgs::c_pack / cs_pack): one line per candidate
typedef double pm_d4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void pack_store(double* base, uint32_t i, double x, double y, double z, uint32_t site, uint32_t located) {
  pm_d4 v;
  v.x = x;
  v.y = y;
  v.z = z;
  v.w = __longlong_as_double((long long)(((unsigned long long)(located & 1u) << 32) | site));
  G((pm_d4*)base)[i] = v;
}
__device__ __forceinline__ pm_d4 pack_load(const double* base, uint32_t i) { return G((const pm_d4*)base)[i]; }
__device__ __forceinline__ uint32_t pack_site(const pm_d4& v) { return (uint32_t)(unsigned long long)__double_as_longlong(v.w); }
__device__ __forceinline__ bool pack_located(const pm_d4& v) { return (((unsigned long long)__double_as_longlong(v.w)) >> 32) & 1ull; }

// ---- wave-wide unsigned min via DPP (no LDS traffic): row_shr 1,2,4,8 -> row_bcast15 -> row_bcast31,
// result broadcast from lane 63 with readlane.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_min32_step(uint32_t v) {
  const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp((int)0xFFFFFFFF, (int)v, CTRL, ROW_MASK, 0xF, false);
  return o < v ? o : v;  // folds into one v_min_u32 with a DPP operand
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
  v = dpp_min32_step<0x111, 0xF>(v);  // row_shr:1
  v = dpp_min32_step<0x112, 0xF>(v);  // row_shr:2
  v = dpp_min32_step<0x114, 0xF>(v);  // row_shr:4
  v = dpp_min32_step<0x118, 0xF>(v);  // row_shr:8
  v = dpp_min32_step<0x142, 0xA>(v);  // row_bcast:15 -> rows 1,3
  v = dpp_min32_step<0x143, 0xC>(v);  // row_bcast:31 -> rows 2,3
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
// 64-bit minimum as two 32-bit reductions (high words, then the low words of the lanes that hold the minimal
// high word): a 64-bit compare-and-select per DPP step costs about three times as many instructions
__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
  const uint32_t hi = (uint32_t)(v >> 32);
  const uint32_t mh = wave_min_u32(hi);
  const uint32_t ml = wave_min_u32(hi == mh ? (uint32_t)v : 0xFFFFFFFFu);
  return ((uint64_t)mh << 32) | ml;
}

__device__ __forceinline__ uint64_t readlane_u64(uint64_t v, uint32_t l) {
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)l) << 32) |
         (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)l);
}

// barrier for exchanges that go through LDS only (no global-memory drain)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

struct BlockRed {
  uint32_t a[CARVE_WAVES];
  uint32_t b[CARVE_WAVES];
  uint32_t part_n[CARVE_WAVES];
  uint32_t flag[CARVE_WAVES];
  // mailbox: wave 0 -> workgroup after a run of fast (proposal) steps
  uint32_t f_action, f_n_cand, f_total_available, f_n_groups, f_mem_off, f_steps, f_fast, f_pad;
  unsigned long long f_cand_sum;
  unsigned long long _spare0;
  uint32_t _spare1, _spare2;
};

// sin on [-pi/2, pi/2] as an odd Taylor polynomial to x^19 (|rel err| < 1e-15 there).  Half a longitude difference
// beyond 180 degrees lies in (pi/2, pi]: reflected, sin(x) = sin(pi - x) with pi in two pieces (the reflection is
// exact to 1e-32) — those are two of every five pairs of a world-wide swarm, and the OCML path they used to take
// (argument reduction with a table in memory) cost a wave more than everything else in a step of stream_small or a
// sweep of carve_exact_step.  Only what is no difference of two longitudes still goes there.  The certificate band
// (2^-36) is four orders of magnitude wider than this error.
__device__ __forceinline__ double sin_band(double x) {
  double ax = fabs(x);
  if (ax > 1.5707963267948966) {
    if (ax > 3.2) return sin(x);
    ax = (3.141592653589793116 - ax) + 1.2246467991473532e-16;
    x = x < 0.0 ? -ax : ax;
  }
  const double z = x * x;
  double p = -8.2206352466243297e-18;               // -1/19!
  p = fma(p, z, 2.8114572543455206e-15);            //  1/17!
  p = fma(p, z, -7.6471637318198164e-13);           // -1/15!
  p = fma(p, z, 1.6059043836821613e-10);            //  1/13!
  p = fma(p, z, -2.5052108385441720e-08);           // -1/11!
  p = fma(p, z, 2.7557319223985893e-06);            //  1/9!
  p = fma(p, z, -1.9841269841269841e-04);           // -1/7!
  p = fma(p, z, 8.3333333333333332e-03);            //  1/5!
  p = fma(p, z, -1.6666666666666666e-01);           // -1/3!
  return fma(x * z, p, x);
}

__device__ __forceinline__ double hav_a(double lat1, double lon1, double cos1, double lat2, double lon2,
                                        double cos2) {
  const double dlat = (lat2 - lat1) * PM_RAD;
  const double dlon = (lon2 - lon1) * PM_RAD;
  const double s1 = sin_band(dlat * 0.5);
  const double s2 = sin_band(dlon * 0.5);
  return s1 * s1 + cos1 * cos2 * (s2 * s2);
}

// The proposer's Haversine term.  a = sin^2(dphi/2) + cos cos sin^2(dlam/2) is, exactly, a quarter of the squared
// chord between the two unit vectors: a = |u1 - u2|^2 / 4 — three subtractions, a multiply and two fma instead of
// two sine polynomials.  The unit vectors carry an absolute error of ~2e-16 per component, so the chord form has a
// relative error of ~6e-16 / sqrt(a) against the reference's a when the two longitudes lie less than 180 degrees apart.
// The long way round the reference's own fl(fl(lon2 - lon1) * RAD) rounds by up to ~9e-16 radians, which the chord
// never sees, and the error grows to ~1.3e-15 / sqrt(a) (measured; 2e-15 / sqrt(a) is the bound asserted).  That is
// within an eighth of the certificate band (2^-36) for a >= PM_A_CHORD_MIN (about 14.5 km), and that is where it is used;
// nearer candidates (rare: a handful per seed) take the sine form, whose error is independent of the distance.  Every path of the proposer goes through this one
// function, so a candidate's key is the same bit pattern wherever it is computed.
struct SeedGeo {
  double lat, lon, cos, ux, uy, uz;
};
template <typename DP>
__device__ __forceinline__ double prox_a(const SeedGeo& s, double ux, double uy, double uz, DP lat, DP lon, DP cs, uint32_t t) {
  const double dx = ux - s.ux, dy = uy - s.uy, dz = uz - s.uz;
  const double a = 0.25 * fma(dx, dx, fma(dy, dy, dz * dz));
  if (a >= PM_A_CHORD_MIN) return a;
  return hav_a(s.lat, s.lon, s.cos, lat[t], lon[t], cs[t]);
}

template <typename P>
__device__ __forceinline__ bool bit_at(P b, uint32_t i) { return (b[i >> 6] >> (i & 63u)) & 1ull; }

// Ordering key of a candidate: the f64 bits of its Haversine term `a` with the low SLOT_BITS replaced by
// the slot number (slot order == input order), so one u64 compare is the whole (distance, input order)
// comparison.  Dropping SLOT_BITS mantissa bits is covered by the certificate band.
__device__ __forceinline__ uint64_t pack_key(uint64_t key_bits, uint32_t slot, uint32_t slot_bits) {
  return ((key_bits >> slot_bits) << slot_bits) | slot;
}

enum { STEP_CONTINUE = 0, STEP_BREAK = 1, STEP_UNCERTAIN = 2, STEP_OVERFLOW = 3, STEP_ABORT = 4 };

struct StepCtx {
  uint32_t mode, proximity, min_s, max_s, cfg;
  uint32_t n_list;       // slots of the current list
  uint32_t n_cand;       // live slots
  uint32_t n_start;      // live slots when the validation of this batch started
  uint32_t n_groups, mem_off;
  uint32_t total_available;
  uint32_t steps, fast_steps;
  unsigned long long cand_sum;
  // proposals (0 = none)
  uint32_t prop_k, prop_limit;
  uint32_t n_seeds;  // seeds of the batch
  bool use_props;
  // packed-key geometry of the current list: low slot_bits of a key hold the slot; certificate band
  uint32_t slot_bits;
  double band;
  bool big;  // per-slot arrays live in HBM/L2 (list above PM_CARVE_SLOTS), bitmaps + staged rows in LDS
};

__device__ __forceinline__ void ctx_set_geometry(StepCtx& c) {
  c.big = c.n_list > PM_CARVE_SLOTS;
  c.slot_bits = c.big ? PM_CARVE_SLOT_BITS_BIG : PM_CARVE_SLOT_BITS;
  c.band = c.big ? PM_TIE_BAND_BIG : PM_TIE_BAND;
}

enum { FAST_DONE = 0, FAST_SLOW = 1, FAST_OVERFLOW = 2, FAST_AGAIN = 3, FAST_REPROPOSE = 4, FAST_SEQ = 5, FAST_WIDEN = 6,
       FAST_ABORT = 7, FAST_TAIL = 8, FAST_TINY = 9, FAST_RANOUT = 10 };

#define FAST_RETURN(code) do { c_ref = c; seed_cur = cur; return (code); } while (0)  // (SLOW_RETURN(why): FAST_SLOW, counted — pm_measure.inc)

// a proposal batch ends (the list is compacted and re-proposed) once fewer than 1 / PM_THIN_DIV of the slots that were
// alive when its validation started are left; a batch prepared beside the one in front of it is not worth validating
// when less than 1 / PM_STALE_DIV of its list is still alive (the next one is prepared from the state as it is then)
#ifndef PM_THIN_DIV
#define PM_THIN_DIV 3u
#endif
#ifndef PM_STALE_DIV
#define PM_STALE_DIV 3u
#endif

// ---- The step rule: one step of the reference's try_form_new_groups (mod.rs:507-586), said once for every stepper
// of this file and of pm_stream.inc.  A stepper differs in where its keys come from and in how many waves work on it;
// what follows it shares with the others.
//   step_open    a configuration takes another step `while total_available >= min` (mod.rs:507), unless fewer than min
//                are compatible (`compatible < min => break`, :517-519).  The merge pass has no pool to count:
//                `while remaining_groups.len() >= min` (:695).
//   step_want    a seed wants max - 1 neighbours, or everyone that is left: fill to max (:545-551).  A group of fewer
//                than min is none (:564-566; the steppers that can come up short test that themselves).
//   step_room    whether the output arrays hold another group of `total`: if not the launch ends and the host makes room.
//   step_forced  the debug hook (pm_engine_config::debug_uncertain_every): every N-th step of a match goes to the host as if it
//                could not be certified.  step_forced_in: the commits that fit in front of the next such step.
//   cert_band    the certificate: the selection is the reference's if everyone within a relative band — plus an absolute
//                one, for a key of 0 — around the last selected key sits at that candidate's coordinates (see "Ordering
//                key" at the top); and no key near the antipode, where the reference's term can round above 1 and its
//                distance is NaN: unsafe, the host settles it.
//   step_record  what a commit writes, by one lane or thread (create_group_atomically, :299-322): the group's record.
//                The members and the bitmaps (healthy_nodes.retain, :585) are the stepper's own.
//   step_book    what a commit books (total_available -= group.len(), :586).  Steps that were no exact sweep count as
//                fast_steps too: their steppers say so.
//   chain_*      the two in-order chains (carve_chain, stream_chain) commit full groups without a look at the context:
//                what a run starts from, how many commits may follow one another before one of the conditions above
//                (or the re-proposal threshold) can come true, which of them ends the run, and the books of the run.
//   first_live_bit, fill_location_less, ctx_uniform: the seed of a step without a seed list (the first located candidate,
//                :526-530), the location-less candidates that fill a group in input order (:553-561; f64::MAX sorts
//                behind every located one), and a context whose fields are said to be the same in every lane.
__device__ __forceinline__ bool step_open(uint32_t total_available, uint32_t n_cand, uint32_t min_s, bool merge = false) {
  return (merge || total_available >= min_s) && n_cand >= min_s && n_cand > 0u;
}
__device__ __forceinline__ bool step_open(const StepCtx& c, bool merge = false) {
  return step_open(c.total_available, c.n_cand, c.min_s, merge);
}
__device__ __forceinline__ uint32_t step_want(const StepCtx& c) {
  return c.max_s - 1u < c.n_cand - 1u ? c.max_s - 1u : c.n_cand - 1u;
}
__device__ __forceinline__ bool step_room(const StepCtx& c, uint32_t total, uint32_t cap_g, uint32_t cap_m) {
  return c.n_groups < cap_g && c.mem_off + total <= cap_m;
}
__device__ __forceinline__ bool step_forced(uint32_t every, uint32_t steps_done) {
  return every && ((steps_done + 1u) % every) == 0u;
}
__device__ __forceinline__ uint32_t step_forced_in(uint32_t every, uint32_t steps_done) {
  return every ? every - (steps_done + 1u) % every : 0xFFFFFFFFu;
}
__device__ __forceinline__ double cert_band(double a_m, double band_rel, bool& unsafe) {
  unsafe = a_m > PM_A_MAX_SAFE;
  return a_m * band_rel + 1e-300;
}
template <typename P>
__device__ __forceinline__ void step_record(P g_cfg, P g_n, P g_off, uint32_t g, uint32_t cfg, uint32_t n, uint32_t off) {
  g_cfg[g] = cfg;
  g_n[g] = n;
  g_off[g] = off;
}
__device__ __forceinline__ void step_book(StepCtx& c, uint32_t total) {
  c.n_groups += 1u;
  c.mem_off += total;
  c.cand_sum += c.n_cand;
  c.n_cand -= total;
  c.total_available -= total;
  c.steps += 1u;
}

// what a run of a chain starts from (wave-uniform)
struct ChainRun {
  uint32_t group_n, cap_g, cap_m, dbg_every, n_list, n_start;
  uint32_t step0;  // steps of the match in front of the run
  uint32_t base_cand, base_groups, base_mem;
};
__device__ __forceinline__ ChainRun chain_run(const CarveArgs& p, const StepCtx& c, uint32_t steps_before) {
  ChainRun r;
  r.group_n = UNI(c.max_s);
  r.cap_g = UNI(p.cap_groups);
  r.cap_m = UNI(p.cap_members);
  r.dbg_every = UNI(p.debug_uncertain_every);
  r.n_list = UNI(c.n_list);
  r.n_start = UNI(c.n_start);
  r.step0 = UNI(steps_before) + UNI(c.steps);
  r.base_cand = UNI(c.n_cand);
  r.base_groups = UNI(c.n_groups);
  r.base_mem = UNI(c.mem_off);
  return r;
}
// Commits that can follow one another before any of the conditions that end a chain can come true (they are looked at
// again when the budget is used up): candidates for full groups, room in the output arrays, the re-proposal
// threshold, the debug hook.  >= 1 whenever none of those conditions holds.
__device__ __forceinline__ uint32_t chain_budget(const ChainRun& r, uint32_t n_cand, uint32_t commits) {
  uint32_t b = n_cand / r.group_n;
  const uint32_t room_g = r.cap_g - (r.base_groups + commits), room_m = (r.cap_m - r.base_mem) / r.group_n - commits;
  b = b < room_g ? b : room_g;
  b = b < room_m ? b : room_m;
  if (r.n_list > 256u) {
    const uint32_t t = n_cand * PM_THIN_DIV >= r.n_start ? (n_cand * PM_THIN_DIV - r.n_start) / (PM_THIN_DIV * r.group_n) + 1u : 1u;
    b = b < t ? b : t;
  }
  const uint32_t f = step_forced_in(r.dbg_every, r.step0 + commits);
  return b < f ? b : f;
}
// Why a chain whose budget is used up stops in front of a live seed; FAST_AGAIN: it does not, and takes a new budget.
// step_open holds while full groups fit (max_s >= min_s); the last, partial group is carve_fast_steps' business
// (FAST_SEQ).  FAST_REPROPOSE: a good part of what was alive when the batch started is gone, the neighbour rows are
// thinning out — re-prepare (compact) and re-propose now, before rows start running out of live entries.
__device__ __forceinline__ int chain_stop_reason(const ChainRun& r, uint32_t n_cand, uint32_t commits) {
  if (n_cand < r.group_n) return FAST_SEQ;
  if (r.base_groups + commits >= r.cap_g || r.base_mem + (commits + 1u) * r.group_n > r.cap_m) return FAST_OVERFLOW;
  if (n_cand * PM_THIN_DIV < r.n_start && r.n_list > 256u && commits > 0u) return FAST_REPROPOSE;
  if (step_forced(r.dbg_every, r.step0 + commits)) return FAST_SLOW;
  return FAST_AGAIN;
}
__device__ __forceinline__ void chain_book(StepCtx& c, const ChainRun& r, uint32_t commits, uint32_t n_cand) {
  c.n_groups = r.base_groups + commits;
  c.mem_off = r.base_mem + commits * r.group_n;
  c.n_cand = n_cand;
  c.total_available -= commits * r.group_n;
  c.steps += commits;
  c.fast_steps += commits;
  // sum over the commits of the live candidates before each: base, base - g, base - 2g, ...
  c.cand_sum += (unsigned long long)commits * r.base_cand -
                (unsigned long long)r.group_n * ((unsigned long long)commits * (commits ? commits - 1u : 0u) / 2ull);
}

// lane j holds word j0 + j of a bitmap: the position of the first set bit of the 64 words, PM_NONE: none is set
__device__ __forceinline__ uint32_t first_bit_of(uint64_t w, uint32_t j0) {
  const uint64_t nz = __ballot(w != 0ull);
  if (!nz) return PM_NONE;
  const int src = __builtin_ctzll(nz);
  return (j0 + src) * 64u + __builtin_ctzll(readlane_u64(w, src));
}
// the first position whose bit is set in both bitmaps (lw words each), PM_NONE: there is none
template <typename PA, typename PB>
__device__ __forceinline__ uint32_t first_live_bit(PA words, PB and_words, uint32_t lw, uint32_t lane) {
  for (uint32_t j0 = 0; j0 < lw; j0 += 64u) {
    const uint32_t j = j0 + lane;
    const uint32_t pos = first_bit_of(j < lw ? (words[j] & and_words[j]) : 0ull, j0);
    if (pos != PM_NONE) return pos;
  }
  return PM_NONE;
}
// The lowest `need` live location-less positions become members `mem_at` on and leave the bitmap and its published copy
// (one wave, a lane a word, 64 words a look).  uw: the first word that may still hold one (every word below it holds
// none for good).
template <typename PA, typename PB, typename PF, typename PM>
__device__ __forceinline__ void fill_location_less(PA l_alive, PB l_loc, PF freeg, PM mem_g, uint32_t mem_at, uint32_t need,
                                                   uint32_t lw, uint32_t lane, uint32_t& uw) {
  uint32_t cnt = 0u;
  bool first = true;
  for (uint32_t jb = uw; jb < lw && cnt < need; jb += 64u) {
    const uint32_t jl = jb + lane;
    const uint64_t wl = jl < lw ? (l_alive[jl] & ~l_loc[jl]) : 0ull;
    uint64_t nz = __ballot(wl != 0ull);
    if (nz && first) {
      uw = jb + (uint32_t)__builtin_ctzll(nz);
      first = false;
    }
    for (; nz && cnt < need; nz &= nz - 1ull) {
      const uint32_t src = (uint32_t)__builtin_ctzll(nz), j = jb + src;
      const uint64_t w = readlane_u64(wl, src);
      const uint32_t rk = __builtin_amdgcn_mbcnt_hi((uint32_t)(w >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)w, 0u));
      const bool take_me = ((w >> lane) & 1ull) && rk < need - cnt;
      const uint64_t take = __ballot(take_me);
      if (take_me) mem_g[mem_at + cnt + rk] = j * 64u + lane;
      if (lane == 0u) {
        __hip_atomic_fetch_and(&l_alive[j], ~take, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_and(&freeg[j], ~take, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      cnt += (uint32_t)__popcll(take);
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (the bitmap words are read again by the next step)
}
// (what is the same in every lane is said to be: a divergent loop counter turns a loop into predicated code)
__device__ __forceinline__ void ctx_uniform(StepCtx& c) {
  c.n_list = UNI(c.n_list);
  c.n_cand = UNI(c.n_cand);
  c.total_available = UNI(c.total_available);
  c.min_s = UNI(c.min_s);
  c.max_s = UNI(c.max_s);
  c.n_groups = UNI(c.n_groups);
  c.mem_off = UNI(c.mem_off);
  c.steps = UNI(c.steps);
  c.fast_steps = UNI(c.fast_steps);
  c.cfg = UNI(c.cfg);
}
// ---- (the step rule ends here)

// The proposals of a batch as the validating wave sees them: seed number i (rank among the live located slots below
// prop_limit at preparation time, ascending slot order) -> its slot (seed_slots, dense); its row is row i of `prop`.

// Fast steps one at a time, executed by wave 0 alone while the other waves are parked at a barrier: the expensive
// part of a step (keys for every live candidate + top-k) was done for every possible seed by
// carve_propose_kernel against the live set at the start of the batch.  Because candidates are
// only ever REMOVED, the reference's sorted remaining list is the proposal row minus the dead entries,
// as long as the row still holds enough live entries and the boundary can be certified; otherwise
// the step is handed to the exact full sweep (FAST_SLOW).  The whole wave looks at one row (lane = entry), so this
// path sees all 63 entries and re-derives the certificate from the keys; it takes what the in-order chain
// (carve_chain) hands over — rows that are not certified wholesale, thinned-out rows, wide groups, the last
// partial group of a configuration — and the first-come tail.  At most max_steps steps (FAST_AGAIN when reached).
// STREAM (carve_stream_kernel): the rows arrive per TICKET — seed_cur is the ticket the chain stopped at (PM_NONE =
// none), sl_words the validator's ticket table in LDS (StreamLds), a row lives in the granule rings stream_row_lo / _hi
// under the ticket's tag.
template <bool BIG, bool STREAM = false>
__device__ __noinline__ int carve_fast_steps(const CarveArgs& p, StepCtx& c_ref, const uint32_t* l_site,
                                             uint64_t* l_alive, const uint64_t* l_loc, uint32_t steps_before,
                                             uint32_t& seed_cur, uint32_t max_steps, uint32_t* sl_words = nullptr) {
  StepCtx c = c_ref;  // registers for the whole run (the reference lives in the caller's scratch frame)
  const uint32_t lane = threadIdx.x & 63u;
  // argument-block fields used per step, loaded once: the stores below go through flat pointers the compiler
  // must assume may alias the block itself
  const auto members = G(p.members);
  const auto g_cfg = G(p.g_cfg);
  const auto g_n = G(p.g_n);
  const auto g_off = G(p.g_off);
  const auto prop = G((const uint64_t*)p.prop);
  const auto seed_slots = G((const uint32_t*)p.seed_slots);
  const uint32_t cap_groups = p.cap_groups, cap_members = p.cap_members;
  const uint32_t dbg_every = p.debug_uncertain_every;
  const uint32_t n_seeds = UNI(c.n_seeds);
  constexpr uint32_t SB = BIG ? PM_CARVE_SLOT_BITS_BIG : PM_CARVE_SLOT_BITS;
  constexpr uint64_t SLOT_MASK = (1ull << SB) - 1ull;
  constexpr uint64_t noloc_key = (PM_KEY_NOLOC >> SB) << SB;
  constexpr double band_rel = BIG ? PM_TIE_BAND_BIG : PM_TIE_BAND;
  typedef __attribute__((address_space(3))) unsigned long long lds_u64;
  typedef __attribute__((address_space(3))) uint32_t lds_u32;
  lds_u64* const A = (lds_u64*)l_alive;
  const lds_u64* const LOC = (const lds_u64*)l_loc;
  const lds_u32* const SITE3 = (const lds_u32*)l_site;
  auto alive_at = [A](uint32_t i) -> bool { return (A[i >> 6] >> (i & 63u)) & 1ull; };
  auto kill = [A](uint32_t i) {
    __hip_atomic_fetch_and(&A[i >> 6], ~(1ull << (i & 63u)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  };
  // (streaming carve: the proposers' copy of the candidate bitmap follows every removal)
  const auto candg = G((unsigned long long*)p.bits_scratch);
  auto mirror = [candg](uint32_t i) {
    if (STREAM) __hip_atomic_fetch_and(&candg[i >> 6], ~(1ull << (i & 63u)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };
  // (members are recorded as SLOTS and translated to worker ids by one parallel pass after the run)
  auto site_of = [SITE3, l_site](uint32_t sl) -> uint32_t { return BIG ? l_site[sl] : SITE3[sl]; };
  const uint32_t lw = (c.n_list + 63u) >> 6;
  uint32_t cur = UNI(seed_cur);  // seeds in front of it are dead for good (they are consumed in ascending order)
  uint32_t fc_j = 0;             // first bitmap word that may still hold a live slot (first-come steps)
  uint32_t done = 0;
  PROF_COUNT(20);  // calls
  for (;;) {
    if (done >= max_steps) FAST_RETURN(FAST_AGAIN);
    if (!step_open(c)) FAST_RETURN(FAST_DONE);
    // ---- seed: the first live located slot = the first live entry of the batch's seed list
    uint32_t f_loc = PM_NONE;
    if (c.proximity) {
      if (STREAM) {
        // Tickets are issued in ascending position order to the located candidates alive at that moment, and
        // consumed in order: the first ticket from `cur` on whose seed is still alive names the first live located
        // candidate.  Behind the last ticket issued, the bitmaps say.
        typedef __attribute__((address_space(3))) uint32_t sl_u32;
        const sl_u32* const TP = (const sl_u32*)sl_words;
        const uint32_t t_req = UNI(TP[PM_STREAM_SLW_TREQ]);
        const uint32_t ci_now = (UNI(TP[PM_STREAM_SLW_PAY]) >> 18) & 63u;  // (tickets of other configurations are skipped)
        while (cur != PM_NONE && cur < t_req) {
          const uint32_t tp = UNI(TP[cur & (PM_STREAM_TP - 1u)]);
          const uint32_t pos = tp & 0x3FFFFu;
          if ((tp >> 18) == ci_now && alive_at(pos)) {
            f_loc = pos;
            break;
          }
          ++cur;
        }
        if (f_loc == PM_NONE) {
          cur = PM_NONE;
          f_loc = first_live_bit(A, LOC, lw, lane);
        }
      } else if (c.prop_k) {
        while (cur < n_seeds) {
          const uint32_t i = cur + lane;
          const uint32_t sl = seed_slots[i < n_seeds ? i : n_seeds - 1u];
          const bool al = i < n_seeds && alive_at(sl);
          const uint64_t m = __ballot(al);
          if (m) {
            const int l = __builtin_ctzll(m);
            cur += (uint32_t)l;
            f_loc = (uint32_t)__builtin_amdgcn_readlane((int)sl, l);
            break;
          }
          cur += 64u;
        }
        if (cur > n_seeds) cur = n_seeds;
        if (f_loc == PM_NONE && c.prop_limit < c.n_list) {
          // every proposed slot is used up; located candidates beyond the proposal batch need a new round
          bool more = false;
          for (uint32_t j0 = c.prop_limit >> 6; j0 < lw && !more; j0 += 64u) {
            const uint32_t j = j0 + lane;
            uint64_t ll = j < lw ? (A[j] & LOC[j]) : 0ull;
            if (j == (c.prop_limit >> 6)) ll &= ~((1ull << (c.prop_limit & 63u)) - 1ull);
            more = __ballot(ll != 0ull) != 0ull;
          }
          if (more) {
            if (lane == 0) G(p.status)->why[1] += 1u;
            FAST_RETURN(FAST_REPROPOSE);
          }
        }
      } else {
        f_loc = first_live_bit(A, LOC, lw, lane);
      }
    }
    const uint32_t want = step_want(c);
    if (!step_room(c, want + 1u, cap_groups, cap_members)) FAST_RETURN(FAST_OVERFLOW);

    if (STREAM && f_loc == PM_NONE) FAST_RETURN(FAST_TAIL);  // (the whole workgroup drains the tail: stream_first_come)
    if (f_loc == PM_NONE) {
      // no located candidate (or proximity off): the group is the first `want + 1` live slots in input
      // order (a seed without location makes the sort a no-op, mod.rs:238).
      // Once there is no located candidate there never will be one again, so the rest of the configuration
      // is drained right here; these steps always take the lowest live slots, every word below fc_j is
      // empty for good, and the scan resumes where it stopped.
      uint32_t n_cand = UNI(c.n_cand), total_av = UNI(c.total_available), n_groups = UNI(c.n_groups),
               mem_off = UNI(c.mem_off), steps = 0;
      const uint32_t min_s = UNI(c.min_s), max_s = UNI(c.max_s), cfg = UNI(c.cfg);
      unsigned long long cand_sum = 0;
      int ret = FAST_DONE;
      for (;;) {
        if (!step_open(total_av, n_cand, min_s)) break;
        const uint32_t need = max_s < n_cand ? max_s : n_cand;  // want + 1
        if (n_groups >= cap_groups || mem_off + need > cap_members) {
          ret = FAST_OVERFLOW;
          break;
        }
        uint32_t cnt = 0;
        for (uint32_t j = fc_j; j < lw && cnt < need; ++j) {
          const uint64_t w = A[j];
          const uint32_t w_lo = UNI((uint32_t)w), w_hi = UNI((uint32_t)(w >> 32));
          if (!(w_lo | w_hi)) continue;
          fc_j = j;
          // the lowest (need - cnt) set bits of w: rank of each set bit within the word, one ballot
          const uint32_t rk = __builtin_amdgcn_mbcnt_hi(w_hi, __builtin_amdgcn_mbcnt_lo(w_lo, 0u));
          const bool mine = ((w >> lane) & 1ull) && rk < need - cnt;
          const uint64_t take = __ballot(mine);
          if (mine) members[mem_off + cnt + rk] = j * 64u + lane;
          if (lane == 0) {
            A[j] = w & ~take;
            if (STREAM && take) __hip_atomic_fetch_and(&candg[j], ~take, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
          cnt += __popcll(take);
        }
        if (lane == 0) step_record(g_cfg, g_n, g_off, n_groups, cfg, cnt, mem_off);
        n_groups += 1;
        mem_off += cnt;
        cand_sum += n_cand;
        n_cand -= cnt;
        total_av -= cnt;
        steps += 1;
        PROF_COUNT(21);  // first-come steps
      }
      c.n_groups = n_groups;
      c.mem_off = mem_off;
      c.cand_sum += cand_sum;
      c.n_cand = n_cand;
      c.total_available = total_av;
      c.steps += steps;
      c.fast_steps += steps;
      FAST_RETURN(ret);
    }

    PROF_COUNT(22);  // located sequential steps (attempts)
    const uint32_t seed = f_loc;
    if (c.prop_k == 0 || seed >= c.prop_limit || (STREAM && cur == PM_NONE)) {  SLOW_RETURN(20); }
    if (step_forced(dbg_every, steps_before + c.steps)) SLOW_RETURN(21);

    // ---- the seed's neighbour row: one packed key per lane, ascending.  Candidates with the seed's exact
    // coordinates are at distance 0 and head the row in slot order.  Of the located candidates only those behind the
    // seed are listed (FORM; a swept row — a walk's leaves out the ones at the seed's own site only): a live one in front
    // of it would have been the seed, so at this moment — the only one a row is read at — nothing is missing, and a
    // row flagged complete lists everything that is alive.
    const size_t rbase = STREAM ? (size_t)(cur & (PM_STREAM_RQ - 1u)) * 64u : (size_t)cur * PM_PROP_ROW;
    uint32_t nk_word;
    if (STREAM) {  // (granule 0: the flags word under the ticket's tag — a row that never arrived does not carry it)
      const unsigned long long g0 = __hip_atomic_load(&G(p.stream_row_lo)[rbase], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (UNI((uint32_t)(g0 >> 32)) != UNI(p.stream_tag0) + cur) SLOW_RETURN(20);
      nk_word = UNI((uint32_t)g0);
    } else {
      nk_word = UNI((uint32_t)prop[rbase]);  // the row's flags word
    }
    const uint32_t n_k = nk_word & 0xFFu;
    const bool complete = (nk_word & PM_ROW_COMPLETE) != 0u;
    const bool tail_ok = (nk_word & PM_ROW_TAIL_OK) != 0u;
    const bool row_clean = (nk_word & PM_ROW_CLEAN) != 0u;
    const bool tail_clear = (nk_word & PM_ROW_TAIL_CLEAR) != 0u;
    const bool row_safe = (nk_word & PM_ROW_SAFE) != 0u;
    uint64_t e;
    if (STREAM) {  // entry `lane` = granules lane + 1 of the two rings (low and high half of the packed key)
      const uint32_t gi = (lane + 1u) & 63u;
      const unsigned long long lo = __hip_atomic_load(&G(p.stream_row_lo)[rbase + gi], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const unsigned long long hi = __hip_atomic_load(&G(p.stream_row_hi)[rbase + gi], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const uint32_t tag = UNI(p.stream_tag0) + cur;
      const bool ok = lane >= n_k || ((uint32_t)(lo >> 32) == tag && (uint32_t)(hi >> 32) == tag);
      if (__ballot(!ok)) SLOW_RETURN(20);
      e = lane < n_k ? ((hi << 32) | (lo & 0xFFFFFFFFull)) : ~0ull;
    } else {
      e = lane < n_k ? prop[rbase + 1u + lane] : ~0ull;
    }
    const uint32_t slot = (uint32_t)(e & SLOT_MASK);
    const bool alive = lane < n_k && alive_at(slot);
    const uint64_t am = __ballot(alive);
    const uint32_t rank = __popcll(am & ((1ull << lane) - 1ull));
    // (timeline of the streaming carve: a row that ran out — entries, live ones, wanted, flags)
    PM_PROF(if (STREAM && (uint32_t)__popcll(am) < want && lane == 0) STREAM_TRACE(14, n_k | ((uint32_t)__popcll(am) << 8) | (want << 16), nk_word >> 16);)
    if ((uint32_t)__popcll(am) < want) {  // row exhausted by earlier groups
      if (STREAM) {  // (the streaming carve wants to know: the rows requested along with this one are as old)
        PM_PROF(if (lane == 0) G(p.status)->prof[25] += 1;)
        FAST_RETURN(FAST_RANOUT);
      }
      SLOW_RETURN(25);
    }
    const bool sel = alive && rank < want;
    // the proposer certified the whole row (clean, safe) and its tail (complete / tail_clear): nothing left to prove
    if (want > 0 && !(row_clean && row_safe && (complete || tail_clear))) {
      const uint64_t lm = __ballot(sel && rank == want - 1u);
      const int lane_m = __builtin_ctzll(lm);
      const uint64_t e_m = readlane_u64(e, lane_m);
      const uint64_t kb_m = (e_m >> SB) << SB;
      if (kb_m != noloc_key) {
        // exactness certificate: every live candidate of the row within the band AROUND the last selected one
        // — selected or not — must sit at its site (then the reference's distances tie exactly there and slot
        // order decides).  The test is symmetric: a selected entry of another site just below the boundary and
        // an unselected one of the boundary's site just above it may be ordered either way by the reference.
        const double a_m = __longlong_as_double((long long)kb_m);
        bool unsafe;
        const double band = cert_band(a_m, band_rel, unsafe);
        if (unsafe) SLOW_RETURN(31);
        const uint32_t site_m = site_of((uint32_t)(e_m & SLOT_MASK));
        const uint64_t kb = (e >> SB) << SB;
        const bool near = alive && kb != noloc_key && fabs(__longlong_as_double((long long)kb) - a_m) <= band;
        if (__ballot(near && site_of(slot) != site_m)) {  SLOW_RETURN(31); }
        if (!complete) {
          // candidates beyond the list are >= its last entry: either that entry clears the band, or it sits
          // at e_m's site and the proposer verified (tail_ok) that everything unlisted within the band of
          // the last entry is at that site too (then those tie exactly and have larger slots)
          const int last_l = (int)n_k - 1;
          const uint64_t e_l = readlane_u64(e, last_l);
          const uint64_t kb_l = (e_l >> SB) << SB;
          if (kb_l != noloc_key && (__longlong_as_double((long long)kb_l) - a_m) <= band) {
            if (!(tail_ok && site_of((uint32_t)(e_l & SLOT_MASK)) == site_m)) SLOW_RETURN(31);
          }
        }
      }
    }
    // ---- commit: the seed, then the row's first `want` live entries in key order
    if (sel) {
      kill(slot);
      mirror(slot);
      members[c.mem_off + 1u + rank] = slot;
    }
    if (lane == 0) {
      kill(seed);
      mirror(seed);
      members[c.mem_off] = seed;
      step_record(g_cfg, g_n, g_off, c.n_groups, c.cfg, want + 1u, c.mem_off);
    }
    step_book(c, want + 1u);
    c.fast_steps += 1;
    cur += 1u;  // this seed is dead now
    ++done;
  }
}

// The chain of located steps of a proposal batch, one seed after the other — no speculation: what makes a step cheap
// is that nothing but the step's own dependency is on its critical path.  A step depends on its predecessors through
// the alive bitmap only (row -> live bits -> kill: one LDS read, one ballot, one LDS atomic), and LDS operations of
// one wave execute in order, so the next seed's read is issued right behind this seed's kill without waiting for
// it.  A lone wave issues an instruction every eight or nine cycles, so the step is cut down to that dependency and
// everything else is done by two other waves of the workgroup, a pipeline through LDS rings (no barrier; the waves
// poll a few control words):
//   wave 1, the producer:  walks the batch's seed list, takes the entries whose seed is alive at that moment,
//                          requests their proposal rows (lane = row entry, lane 0 = the seed itself; 256 coalesced
//                          bytes per row, two blocks of CHAIN_BLOCK rows in flight) and parks them, digested — per
//                          lane the LDS address of the slot's bitmap word and its bit — in a ring;
//   wave 0, the chain:     per ring entry: the live lanes of the row (one read, one ballot); a dead seed (absorbed by
//                          a group since its row was requested) is no step; otherwise the seed and its first `want`
//                          live entries are killed (one atomic) and the live mask is passed on;
//   wave 2, the collector: re-derives the selection from the live mask, collects the members in LDS (the key array is
//                          idle while the chain runs) and writes them out with the group records, then hands the ring
//                          entry back to the producer.
// Because candidates are only ever REMOVED, the reference's sorted remaining list (mod.rs:234-255) is the proposal
// row minus its dead entries; the group is the seed plus the row's first `want` live entries (mod.rs:545-561).
// Full groups only (want = max_s - 1), and only rows whose flags word settles the certificate wholesale.  Everything
// else is handed to carve_fast_steps, which looks at the seed at seed_cur with the row's keys: other rows, exhausted
// rows (-> exact sweep), the debug hook (FAST_SLOW: exactly one step), the last partial group, the first-come tail,
// the end of the batch (FAST_SEQ).
#ifndef CHAIN_BLOCK
#define CHAIN_BLOCK 8u
#endif
#ifndef CHAIN_NAP_COLLECT  // the collector's nap between two looks at the chain's progress word
#define CHAIN_NAP_COLLECT 1
#endif
#ifndef CHAIN_RING
#define CHAIN_RING 64u                                 // rows parked in LDS (a power of two, >= 2 blocks; 32 until the
#endif                                                 // streaming carve's four parkers filled it faster than it drained)
// LDS layout of the chain inside the (idle) key array, in 32-bit words: per ring entry and lane (bitmap word address,
// bit) as one 64-bit word and the slot; per ring entry the seed number, the digested flags and the live mask; the
// control block; then the member buffer
#define CHAIN_RING_WORDS (3u * CHAIN_RING * 64u + 5u * CHAIN_RING + 16u)
#define CHAIN_STAGE_WORDS (PM_CARVE_SLOTS * 2u - CHAIN_RING_WORDS)
// control words (u32 index into the control block)
enum { CC_HEAD = 0, CC_CRIT = 1, CC_TAIL = 2, CC_CMD = 3, CC_ACK1 = 4, CC_ACK2 = 5, CC_START = 6, CC_DONE = 7,
       CC_ABORT = 8, CC_G0 = 9, CC_M0 = 10 };
enum { CH_RUN = 1u, CH_STOP = 2u, CH_QUIT = 3u };  // low two bits of a command word (the rest: sequence number)
#define CHAIN_SPIN_LIMIT (1u << 22)  // polls before a wait gives up (a lost hand-shake must never hang the GPU)
typedef __attribute__((address_space(3))) uint32_t chain_lds_u32;
typedef __attribute__((address_space(3))) unsigned long long chain_lds_u64;
__device__ __forceinline__ uint32_t cc_ld(chain_lds_u32* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void cc_st(chain_lds_u32* p, uint32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
struct ChainLds {
  chain_lds_u64 *RAB, *Q;
  chain_lds_u32 *RE, *RI, *RM, *RS, *CC, *STAGE;  // (RS: streaming carve — entry q of a run is parked when RS[q % R] == q + 1)
};
__device__ __forceinline__ ChainLds chain_lds(uint32_t* l_buf) {
  ChainLds L;
  L.RAB = lds_pin<chain_lds_u64*>(l_buf);
  L.Q = L.RAB + CHAIN_RING * 64u;
  L.RE = (chain_lds_u32*)(L.Q + CHAIN_RING);
  L.RI = L.RE + CHAIN_RING * 64u;
  L.RM = L.RI + CHAIN_RING;
  L.RS = L.RM + CHAIN_RING;
  L.CC = L.RS + CHAIN_RING;
  L.STAGE = L.CC + 16u;
  return L;
}
// wait for a command word other than `seen`; 0 = gave up (abort)
__device__ __forceinline__ uint32_t chain_wait_cmd(const ChainLds& L, uint32_t seen) {
  uint32_t cmd, spins = 0u;
  while ((cmd = cc_ld(&L.CC[CC_CMD])) == seen) {
    __builtin_amdgcn_s_sleep(2);
    if (++spins > CHAIN_SPIN_LIMIT || cc_ld(&L.CC[CC_ABORT])) {
      cc_st(&L.CC[CC_ABORT], 1u);
      return 0u;
    }
  }
  return cmd;
}

// ---- producer (wave 1): serves RUN commands until QUIT
template <bool BIG>
__device__ __noinline__ void carve_chain_produce(const CarveArgs& p, const StepCtx& c, uint64_t* l_alive, uint32_t* l_buf) {
  constexpr uint32_t NB = CHAIN_BLOCK, R = CHAIN_RING;
  static_assert(R >= 2u * NB && (R & (R - 1u)) == 0u, "ring geometry");
  const uint32_t lane = threadIdx.x & 63u;
  chain_lds_u32* const A = lds_pin<chain_lds_u32*>(l_alive);
  const ChainLds L = chain_lds(l_buf);
  const uint32_t a_base = (uint32_t)(uintptr_t)A;
  const auto rows32 = G((const uint32_t*)p.prop);  // row r: 2 * PM_PROP_ROW words; its compact slot list (flags word,
                                                   // slot of entry 0, 1, ...) starts at word 2 * PM_PROP_SLOTS
  const auto seed_slots = G((const uint32_t*)p.seed_slots);
  const uint32_t n_seeds = UNI(c.n_seeds);
  uint32_t seen = 0u;  // last command word acted on
  for (;;) {
    uint32_t cmd = chain_wait_cmd(L, seen);
    if (cmd == 0u) return;
    seen = cmd;
    if ((cmd & 3u) == CH_QUIT) return;
    if ((cmd & 3u) != CH_RUN) {  // (a STOP without a RUN in between)
      cc_st(&L.CC[CC_ACK1], cmd);
      continue;
    }
    // ---- RUN: the seed list from CC_START on, 64 entries at a time (q: slots of entries cbase .. cbase + 63; qn: the
    // next 64, on their way)
    const uint32_t start = UNI(cc_ld(&L.CC[CC_START]));
    uint32_t cbase = start & ~63u, cpos = start, head = 0u;  // cpos: first entry not yet handed to a block
    auto load_chunk = [&](uint32_t b) -> uint32_t {
      const uint32_t i = b + lane;
      return seed_slots[i < n_seeds ? i : (n_seeds ? n_seeds - 1u : 0u)];
    };
    uint32_t q = load_chunk(cbase), qn = load_chunk(cbase + 64u);
    uint32_t rowA[NB], rowB[NB], idxA = 0u, idxB = 0u, posA = 0u, posB = 0u, nA = 0u, nB = 0u;
#pragma unroll
    for (uint32_t k = 0; k < NB; ++k) rowA[k] = rowB[k] = 0u;
    // request the rows of the next (up to) NB seeds of the list that are alive right now
    auto request = [&](uint32_t (&prow)[NB], uint32_t& pidx_v, uint32_t& ppos_v, uint32_t& pend_n) {
      pend_n = 0u;
      while (pend_n == 0u && cpos < n_seeds) {
        const uint32_t i = cbase + lane;
        const uint32_t w = A[q >> 5];
        uint64_t m = __ballot(i >= cpos && i < n_seeds && ((w >> (q & 31u)) & 1u) != 0u);
        const uint32_t n_m = (uint32_t)__popcll(m);
        pend_n = n_m < NB ? n_m : NB;
#pragma unroll
        for (uint32_t k = 0; k < NB; ++k) {
          if (k < pend_n) {  // the k-th live entry of the chunk -> lane k of the block registers
            const uint32_t l = (uint32_t)__builtin_ctzll(m);
            m &= m - 1ull;
            const uint32_t si = cbase + l;
            const uint32_t sp = (uint32_t)__builtin_amdgcn_readlane((int)q, (int)l);
            pidx_v = lane == k ? si : pidx_v;
            ppos_v = lane == k ? sp : ppos_v;
            prow[k] = rows32[(size_t)si * (2u * PM_PROP_ROW) + 2u * PM_PROP_SLOTS + lane];
            cpos = si + 1u;
          }
        }
        if (m == 0ull) cpos = cbase + 64u;  // nothing alive behind them in this chunk
        if (cpos >= cbase + 64u) {          // the chunk is used up: on to the next one
          cbase += 64u;
          q = qn;
          qn = load_chunk(cbase + 64u);
        }
      }
    };
    // park a block that has arrived: wait for room, write the digested rows, publish the new head.
    // Returns false when a new command came in while waiting.
    auto park = [&](uint32_t (&prow)[NB], uint32_t pidx_v, uint32_t ppos_v, uint32_t& pend_n) -> bool {
      if (pend_n == 0u) return true;
      uint32_t sp_n = 0u;
      while (head - cc_ld(&L.CC[CC_TAIL]) + pend_n > R) {
        __builtin_amdgcn_s_sleep(1);
        if (cc_ld(&L.CC[CC_CMD]) != seen) return false;
        if (++sp_n > CHAIN_SPIN_LIMIT) {
          cc_st(&L.CC[CC_ABORT], 1u);
          return false;
        }
      }
#pragma unroll
      for (uint32_t k = 0; k < NB; ++k) {
        if (k < pend_n) {
          const uint32_t meta = UNI(prow[k]);
          const uint32_t sp = (uint32_t)__builtin_amdgcn_readlane((int)ppos_v, (int)k);
          const uint32_t si = (uint32_t)__builtin_amdgcn_readlane((int)pidx_v, (int)k);
          const uint32_t e = lane == 0u ? sp : prow[k];
          const uint32_t r = (head + k) & (R - 1u);
          const uint32_t o = r * 64u + lane;
          const uint32_t bit = lane <= (meta & 0xFFu) ? 1u << (e & 31u) : 0u;
          L.RAB[o] = ((unsigned long long)bit << 32) | (a_base + ((e >> 5) << 2));
          L.RE[o] = e;
          // what a step needs of the flags word: bit 0 clean and safe, bit 1 the tail is settled, bits 8..15 the
          // first entry within the band of the last one
          const uint32_t m2 = (((meta & PM_ROW_CLEAN) && (meta & PM_ROW_SAFE)) ? 1u : 0u) |
                              ((meta & (PM_ROW_COMPLETE | PM_ROW_TAIL_CLEAR | PM_ROW_TAIL_OK)) ? 2u : 0u) | (meta & 0xFF00u);
          if (lane == 0u) {
            L.RI[r] = si;
            L.RM[r] = m2;
          }
        }
      }
      head += pend_n;
      pend_n = 0u;
      cc_st(&L.CC[CC_HEAD], head);  // (LDS operations of a wave execute in order: the rows are there before the head)
      return true;
    };
    bool running = true;
    request(rowA, idxA, posA, nA);
    while (running) {
      request(rowB, idxB, posB, nB);
      if (!park(rowA, idxA, posA, nA)) break;
      if (nB == 0u) running = false;
      if (running) {
        request(rowA, idxA, posA, nA);
        if (!park(rowB, idxB, posB, nB)) break;
        if (nA == 0u) running = false;
      }
      if (cc_ld(&L.CC[CC_CMD]) != seen) break;
    }
    if (!running) cc_st(&L.CC[CC_DONE], 1u);  // the list is used up: CC_HEAD is final
    cmd = chain_wait_cmd(L, seen);
    if (cmd == 0u) return;
    seen = cmd;
    if ((cmd & 3u) == CH_QUIT) return;
    cc_st(&L.CC[CC_ACK1], cmd);  // STOP
  }
}

// ---- collector (wave 2): serves RUN commands until QUIT
template <bool BIG, bool STREAM = false>
__device__ __noinline__ void carve_chain_collect(const CarveArgs& p, const StepCtx& c, uint32_t* l_buf) {
  constexpr uint32_t R = CHAIN_RING;
  const uint32_t lane = threadIdx.x & 63u;
  const ChainLds L = chain_lds(l_buf);
  const auto members = G(p.members);
  const auto g_cfg = G(p.g_cfg);
  const auto g_n = G(p.g_n);
  const auto g_off = G(p.g_off);
  const uint32_t group_n = UNI(c.max_s), want = group_n - 1u, cfg = UNI(c.cfg);
  // (read HERE, once: inside the loop the compiler re-reads the argument block behind every store it cannot prove
  // unaliased — a round trip to L2 per collected entry, four times what the chain takes to commit one: the collector
  // fell behind, the ring looked full to the parkers, and the chain ran dry in front of a full ring)
  const auto free32 = G((uint32_t*)p.bits_scratch);
  uint32_t seen = 0u;
  for (;;) {
    uint32_t cmd = chain_wait_cmd(L, seen);
    if (cmd == 0u) return;
    seen = cmd;
    if ((cmd & 3u) == CH_QUIT) return;
    if ((cmd & 3u) != CH_RUN) {
      cc_st(&L.CC[CC_ACK2], cmd);
      continue;
    }
    uint32_t n_groups = UNI(cc_ld(&L.CC[CC_G0])), mem_off = UNI(cc_ld(&L.CC[CC_M0]));  // as of the last write-out
    uint32_t staged = 0u, t2 = 0u;
    // the records of the groups collected since the last write-out (all of them full groups, back to back; their members
    // went out as they were collected)
    auto write_out = [&]() {
      for (uint32_t g = lane; g < staged; g += 64u) {
        g_cfg[n_groups + g] = cfg;
        g_n[n_groups + g] = group_n;
        g_off[n_groups + g] = mem_off + g * group_n;
      }
      n_groups += staged;
      mem_off += staged * group_n;
      staged = 0u;
    };
    uint32_t idle = 0u;
    bool stopping = false;
    for (;;) {
      const uint32_t crit = UNI(cc_ld(&L.CC[CC_CRIT]));
      if (t2 != crit) {
        idle = 0u;
        // Everything the chain has published, in ONE pass: the entries' words in one read (lane j: entry t2 + j), the rows
        // of the committed ones one read each, the next one's on its way while this one's members go out.  (Entry by entry
        // — its word, then its row, then the next entry's word — the collector was two dependent LDS round trips a commit
        // behind a chain that needs one: round 6 slowed each of the validator's waves down in turn, and it was the
        // collector, not the chain or the parkers, whose naps showed up in the carve's time one for one;
        // profiles/r06_pipeline_experiments.txt.  The members go straight to memory: the stores are fire-and-forget, the
        // staging buffer was an LDS write and a read more per member.)
        while (t2 != crit) {
          t2 = UNI(t2);
          staged = UNI(staged);
          const uint32_t n = crit - t2 < R ? crit - t2 : R;
          const uint32_t rj = (t2 + lane) & (R - 1u);
          // (the streaming chain leaves an entry's word where its row was — lane 0's slot — the batch pipeline's in Q)
          const unsigned long long wj = lane < n ? (STREAM ? L.RAB[rj * 64u] : L.Q[rj]) : 0ull;
          uint64_t cm = __ballot(wj != 0ull);  // the committed steps among them
          uint32_t k = cm ? (uint32_t)__builtin_ctzll(cm) : 0u;
          uint32_t re = L.RE[((t2 + k) & (R - 1u)) * 64u + lane];
          while (cm) {
            cm &= cm - 1ull;
            const uint32_t kn = cm ? (uint32_t)__builtin_ctzll(cm) : k;
            const uint32_t re_n = L.RE[((t2 + kn) & (R - 1u)) * 64u + lane];  // (the last one's again: read, not used)
            // a committed step: the seed and its `want` nearest live neighbours, in key order
            const uint64_t a = readlane_u64(wj, k);
            const uint32_t rk = __builtin_amdgcn_mbcnt_hi((uint32_t)(a >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)a, 0u));
            if (((a >> lane) & 1ull) && rk <= want) {
              members[mem_off + staged * group_n + rk] = re;  // slots (translated to worker ids after the run)
              // (streaming carve: the proposers' copy of the candidate bitmap follows the chain, a few steps behind)
              if (STREAM)
                __hip_atomic_fetch_and(&free32[re >> 5], ~(1u << (re & 31u)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            staged += 1u;
            k = kn;
            re = re_n;
          }
          t2 += n;
          cc_st(&L.CC[CC_TAIL], t2);  // room for the producer
        }
        continue;
      }
      if (stopping) break;  // (CC_CRIT was final when the STOP was seen, and everything up to it is collected)
      if (cc_ld(&L.CC[CC_CMD]) != seen) {
        stopping = true;  // one more look at CC_CRIT: the chain publishes its last entries before the STOP
        continue;
      }
      __builtin_amdgcn_s_sleep(CHAIN_NAP_COLLECT);
      if (++idle > CHAIN_SPIN_LIMIT || cc_ld(&L.CC[CC_ABORT])) {
        cc_st(&L.CC[CC_ABORT], 1u);
        return;
      }
    }
    write_out();
    cmd = chain_wait_cmd(L, seen);
    if (cmd == 0u) return;
    seen = cmd;
    if ((cmd & 3u) == CH_QUIT) return;
    cc_st(&L.CC[CC_ACK2], cmd);  // STOP: the members are written
  }
}

// ---- the chain itself (wave 0)
template <bool BIG>
__device__ __noinline__ int carve_chain(const CarveArgs& p, StepCtx& c_ref, uint32_t* l_buf, uint32_t steps_before,
                                        uint32_t& seed_cur, uint32_t& cmd_seq) {
  StepCtx c = c_ref;
  constexpr uint32_t R = CHAIN_RING;
  const uint32_t lane = threadIdx.x & 63u;
  typedef chain_lds_u32 lds_u32;
  const ChainLds L = chain_lds(l_buf);
  const uint32_t n_seeds = UNI(c.n_seeds);
  const ChainRun run = chain_run(p, c, steps_before);
  const uint32_t group_n = run.group_n, want = group_n - 1u;
  uint32_t n_cand = run.base_cand, commits = 0;
  int action = FAST_SEQ;
  uint32_t exit_cur = n_seeds;  // where carve_fast_steps resumes its search for the first live seed
  CH_DECL;

  // ---- start the producer and the collector
  if (lane == 0u) {
    cc_st(&L.CC[CC_HEAD], 0u);
    cc_st(&L.CC[CC_CRIT], 0u);
    cc_st(&L.CC[CC_TAIL], 0u);
    cc_st(&L.CC[CC_DONE], 0u);
    cc_st(&L.CC[CC_START], UNI(seed_cur));
    cc_st(&L.CC[CC_G0], run.base_groups);
    cc_st(&L.CC[CC_M0], run.base_mem);
  }
  cmd_seq += 4u;
  if (lane == 0u) cc_st(&L.CC[CC_CMD], cmd_seq | CH_RUN);
  uint32_t tail = 0u, budget = 0u;
  bool aborted = false;
  if (n_seeds > 0u) {
    for (;;) {
      CH_COUNT(cn_outer);
      tail = UNI(tail);
      // ---- rows parked and not yet looked at
      uint32_t head = UNI(cc_ld(&L.CC[CC_HEAD]));
      if (head == tail) {
        uint32_t sp_n = 0u;
        bool used_up = false;
        for (;;) {
          const uint32_t done = UNI(cc_ld(&L.CC[CC_DONE]));
          head = UNI(cc_ld(&L.CC[CC_HEAD]));  // (read behind the flag: a set flag means this head is final)
          if (head != tail) break;
          if (done) {
            used_up = true;
            break;
          }
          __builtin_amdgcn_s_sleep(1);
          if (++sp_n > CHAIN_SPIN_LIMIT || UNI(cc_ld(&L.CC[CC_ABORT]))) {
            aborted = true;
            break;
          }
        }
        CH_COUNT(cn_wait);
        if (aborted) break;
        if (used_up) {  // the list is used up
          action = FAST_SEQ;
          exit_cur = n_seeds;
          break;
        }
      }
      CH_MARK(ct_wait);
      uint32_t n_steps = head - tail;
      n_steps = n_steps < 16u ? n_steps : 16u;
      bool stop = false;
      unsigned long long rab_n = L.RAB[(tail & (R - 1u)) * 64u + lane];
      uint32_t rm_n = L.RM[tail & (R - 1u)];
      const uint32_t flags_needed = want != 0u ? 3u : 0u;
      uint32_t s = 0u;
      while (s < n_steps) {
        // ---- the steps that need no second look, as straight-line code with ONE way out: a dead seed (absorbed by a
        // group since its row was requested) is a step that selects nothing
        bool good = true;
        uint64_t a = 0ull;
        uint32_t r = 0u, ra = 0u, rb = 0u, m2 = 0u;
        do {
          r = tail & (R - 1u);
          ra = (uint32_t)rab_n;
          rb = (uint32_t)(rab_n >> 32);
          m2 = UNI(rm_n);
          const uint32_t w = *(lds_u32*)(uintptr_t)ra;
          rab_n = L.RAB[((tail + 1u) & (R - 1u)) * 64u + lane];  // (the next step's row, one step early)
          rm_n = L.RM[(tail + 1u) & (R - 1u)];
          a = __ballot((w & rb) != 0u);
          const bool live = (a & 1ull) != 0ull;
          // my rank among the live lanes: 0 for the seed, e + 1 for the e-th live entry
          const uint32_t rk = __builtin_amdgcn_mbcnt_hi((uint32_t)(a >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)a, 0u));
          const uint64_t selm = live ? a & __ballot(rk <= want) : 0ull;  // the seed and its `want` nearest live neighbours
          // enough live entries, a row whose flags settle the certificate wholesale, and no end of the chain in sight
          good = !live || ((uint32_t)__popcll(selm) == group_n && (m2 & flags_needed) == flags_needed && budget != 0u);
          if (__builtin_expect(!good, 0)) break;
          // commit
          if ((selm >> lane) & 1ull)
            __hip_atomic_fetch_and((lds_u32*)(uintptr_t)ra, ~rb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          L.Q[r] = live ? a : 0ull;  // (every lane the same word: the collector re-derives the selection from it)
          ++tail;
          ++s;
          n_cand -= live ? group_n : 0u;
          commits += live ? 1u : 0u;
          budget -= live ? 1u : 0u;
          PM_PROF(cn_dead += live ? 0u : 1u;)
        } while (s < n_steps);
        if (good) break;
        // ---- a live seed that needs a second look (its row is loaded: ra, rb, m2, a)
        if (budget == 0u) {
          exit_cur = UNI(L.RI[r]);
          const int why = chain_stop_reason(run, n_cand, commits);
          if (why != FAST_AGAIN) {
            if (why == FAST_REPROPOSE && lane == 0u) p.status->why[0] += 1u;
            action = why;
            stop = true;
            break;
          }
          budget = chain_budget(run, n_cand, commits);
        }
        {
          const uint32_t rk = __builtin_amdgcn_mbcnt_hi((uint32_t)(a >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)a, 0u));
          const uint64_t selm = a & __ballot(rk <= want);
          // enough live entries, and a row whose flags settle the certificate: no two entries near each other at
          // different sites, nothing near the antipode, and a tail that is complete / clear / at one site — or a
          // selection that ends in front of the tail's band
          bool ok = (uint32_t)__popcll(selm) == group_n;
          if (want != 0u && (m2 & 3u) != 3u)
            ok = ok && (m2 & 1u) && 62u - (uint32_t)__builtin_clzll(selm | 2ull) < ((m2 >> 8) & 0xFFu);
          if (!ok) {
            exit_cur = UNI(L.RI[r]);
            action = FAST_SLOW;
            stop = true;
            break;
          }
          if ((selm >> lane) & 1ull)
            __hip_atomic_fetch_and((lds_u32*)(uintptr_t)ra, ~rb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          L.Q[r] = a;
          ++tail;
          ++s;
          n_cand -= group_n;
          commits += 1u;
          budget -= 1u;
        }
      }
      if (lane == 0u) cc_st(&L.CC[CC_CRIT], tail);  // for the collector
      CH_MARK(ct_steps);
      if (stop) break;
    }
  }
  // ---- stop the other two (they must be off the key array before it is used again; the collector writes out first)
  cmd_seq += 4u;
  if (lane == 0u) cc_st(&L.CC[CC_CMD], cmd_seq | CH_STOP);
  {
    uint32_t sp_n = 0u;
    while (UNI(cc_ld(&L.CC[CC_ACK1])) != (cmd_seq | CH_STOP) || UNI(cc_ld(&L.CC[CC_ACK2])) != (cmd_seq | CH_STOP)) {
      __builtin_amdgcn_s_sleep(1);
      if (++sp_n > CHAIN_SPIN_LIMIT || UNI(cc_ld(&L.CC[CC_ABORT]))) {
        aborted = true;
        break;
      }
    }
  }
  CH_MARK(ct_stop);
  if (aborted) {
    if (lane == 0u) cc_st(&L.CC[CC_ABORT], 1u);
    action = FAST_ABORT;  // a hand-shake inside the workgroup timed out: reported as CARVE_STATE_ABORTED (never seen)
  }
  chain_book(c, run, commits, n_cand);
  CH_BOOK();
  c_ref = c;
  seed_cur = exit_cur;
  return action;
}

// One exact step of a configuration (the reference's filter + sort + take, mod.rs:511-561, evaluated as it stands):
// keys for every live candidate, two-level selection (DPP argmin rounds per wave, 8-way merge), certificate, commit.
// The whole workgroup; three LDS-only barriers.  STEP_CONTINUE = one group committed.
// SPARSE (streaming carve, where slot == position and a list is as long as the eligible list whatever is left of it):
// the sweeps run over the live candidates only — `cl` lists their slots, ascending, n_cl of them, keys are indexed
// like `cl` — so a step costs what is left, not what there was.
template <bool BIG, bool SPARSE = false>
__device__ __noinline__ int carve_exact_step(const CarveArgs& p, BlockRed& red, StepCtx& c, const uint32_t* l_wid,
                                             uint64_t* l_key, uint64_t* l_alive, const uint64_t* l_loc, uint64_t* part,
                                             uint32_t* sel_out, uint32_t steps_before, unsigned long long* mirror,
                                             const uint32_t* cl = nullptr, uint32_t n_cl = 0u) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t n_it = SPARSE ? n_cl : c.n_list;  // entries the sweeps run over
  auto slot_of = [cl](uint32_t i) -> uint32_t { return SPARSE ? cl[i] : i; };
  constexpr uint32_t SB = BIG ? PM_CARVE_SLOT_BITS_BIG : PM_CARVE_SLOT_BITS;
  constexpr double band_rel = BIG ? PM_TIE_BAND_BIG : PM_TIE_BAND;
  const uint32_t lw = (c.n_list + 63u) >> 6;
  auto wid_of = [](uint32_t sl) -> uint32_t { return sl; };  // members are recorded as SLOTS (translated after the run)
  if (!step_open(c, c.mode == CARVE_MODE_MERGE)) return STEP_BREAK;
  PROF_DECL;
  // ---- seed: first live slot with a location, else first live slot; every wave finds it redundantly from the
  // bitmaps with one ballot per 64 words (no barrier, no shuffle tree; both in one pass over LDS)
  uint32_t f_loc = PM_NONE, f_any = PM_NONE;
  for (uint32_t j0 = 0; j0 < lw && (f_loc == PM_NONE || f_any == PM_NONE); j0 += 64u) {
    const uint32_t j = j0 + lane;
    const uint64_t al = j < lw ? l_alive[j] : 0ull;
    const uint64_t ll = j < lw ? (al & l_loc[j]) : 0ull;
    if (f_any == PM_NONE) f_any = first_bit_of(al, j0);
    if (f_loc == PM_NONE) f_loc = first_bit_of(ll, j0);
  }

  const uint32_t want = step_want(c);
  uint32_t seed = f_any;
  bool use_dist = false, located_only = false;
  uint64_t last = 0;
  uint32_t n_sel = 0, total = 0;

  // attempt 0: FORM, or MERGE with proximity (mod.rs:762-821); attempt 1: MERGE first-come (:824-848)
  for (int attempt = 0; attempt < 2; ++attempt) {
    if (c.mode == CARVE_MODE_FORM) {
      if (attempt == 1) break;
      seed = f_any;
      use_dist = false;
      if (c.proximity && f_loc != PM_NONE) {  // seed = first WITH a location
        seed = f_loc;
        use_dist = true;
      }  // else first-come (:553-561), or a seed without location makes the sort a no-op (:238)
      located_only = false;
    } else if (attempt == 0) {
      if (!(c.proximity && f_loc != PM_NONE)) continue;
      seed = f_loc;
      use_dist = true;
      located_only = true;
    } else {
      if (!(total == 0 || (total < c.max_s && total < c.min_s))) break;
      seed = f_any;
      use_dist = false;
      located_only = false;
    }

    // ---- keys (registers only; the seed's coordinates are one uniform load each)
    const double slat = G(p.cc_lat)[seed], slon = G(p.cc_lon)[seed], scos = G(p.cc_cos)[seed];
    uint64_t lmin = ~0ull;
    for (uint32_t i = tid; i < n_it; i += CARVE_THREADS) {
      const uint32_t s = slot_of(i);
      uint64_t k = ~0ull;
      if (s != seed && (SPARSE || bit_at(l_alive, s))) {
        if (!use_dist) {
          k = s;
        } else if (bit_at(l_loc, s)) {
          k = pack_key((uint64_t)__double_as_longlong(
                           hav_a(slat, slon, scos, G(p.cc_lat)[s], G(p.cc_lon)[s], G(p.cc_cos)[s])), s, SB);
        } else if (!located_only) {
          k = pack_key(PM_KEY_NOLOC, s, SB);
        }
      }
      l_key[i] = k;
      lmin = k < lmin ? k : lmin;
    }
      n_sel = 0;
    last = 0;
    if (want > 0) {
      if (want <= PM_CARVE_PART) {
        // ---- level 1: this wave's `want` smallest, DPP argmin rounds, no barrier
        uint32_t cnt = 0;
        while (cnt < want) {
          const uint64_t v = wave_min_u64(lmin);
          if (v == ~0ull) break;
          if (lane == 0) part[wave * PM_CARVE_PART + cnt] = v;
          ++cnt;
          if (lmin == v) {  // the owning lane advances to its next element (keys are unique)
            uint64_t m = ~0ull;
            for (uint32_t i = tid; i < n_it; i += CARVE_THREADS) {
              const uint64_t k = l_key[i];
              m = (k > v && k < m) ? k : m;
            }
            lmin = m;
          }
        }
        if (lane == 0) red.part_n[wave] = cnt;
              lds_barrier();
              // ---- level 2: merge of the waves' sorted partial lists, redundantly in every wave
        uint32_t ptr = 0;
        const uint32_t my_n = lane < CARVE_WAVES ? red.part_n[lane] : 0u;
        uint64_t head = my_n ? part[lane * PM_CARVE_PART] : ~0ull;
        uint64_t mine = ~0ull;
        while (n_sel < want) {
          const uint64_t v = wave_min_u64(head);
          if (v == ~0ull) break;
          if (lane == n_sel) mine = v;
          last = v;
          ++n_sel;
          if (head == v) {
            ++ptr;
            head = ptr < my_n ? part[lane * PM_CARVE_PART + ptr] : ~0ull;
          }
        }
        if (wave == 0 && lane < n_sel) sel_out[lane] = (uint32_t)(mine & ((1ull << SB) - 1ull));
            } else {
        // ---- wide groups: one workgroup-wide round per member (wave argmin -> LDS -> fold)
        while (n_sel < want) {
          const uint64_t v = wave_min_u64(lmin);
          if (lane == 0) part[wave] = v;
          lds_barrier();
          uint64_t b = ~0ull;
#pragma unroll
          for (uint32_t k = 0; k < CARVE_WAVES; ++k) b = part[k] < b ? part[k] : b;
          lds_barrier();
          if (b == ~0ull) break;
          const uint32_t bs = (uint32_t)(b & ((1ull << SB) - 1ull));
          if (tid == 0) {
            if (n_sel < PM_CARVE_SEL_CAP)
              sel_out[n_sel] = bs;
            else if (c.mem_off + 1u + n_sel < p.cap_members)
              G(p.members)[c.mem_off + 1u + n_sel] = wid_of(bs);
          }
          last = b;
          ++n_sel;
          if (lmin == b) {
            uint64_t m = ~0ull;
            for (uint32_t i = tid; i < n_it; i += CARVE_THREADS) {
              const uint64_t k = l_key[i];
              m = (k > b && k < m) ? k : m;
            }
            lmin = m;
          }
        }
      }
    }
    total = 1u + n_sel;
    if (c.mode == CARVE_MODE_FORM) break;
    if (attempt == 0 && want > 0 && want <= PM_CARVE_PART) lds_barrier();  // part/part_n reused by attempt 1
  }
  if (total == 0) return STEP_BREAK;                                   // MERGE: nothing selectable
  if (c.mode == CARVE_MODE_FORM && total < c.min_s) return STEP_BREAK;  // mod.rs:564-566
  if (c.mode == CARVE_MODE_MERGE && total < 2u) return STEP_BREAK;      // is_merge_beneficial (mod.rs:868-870)

  // ---- exactness certificate for a distance-ordered selection (see the comment above carve_kernel)
  int uncertain = step_forced(p.debug_uncertain_every, steps_before + c.steps) && use_dist;
  const uint64_t noloc_key = (PM_KEY_NOLOC >> SB) << SB;
  const uint64_t last_key = (last >> SB) << SB;
  if (use_dist && n_sel > 0 && last_key != noloc_key) {
    const uint32_t ls = (uint32_t)(last & ((1ull << SB) - 1ull));
    const double a_m = __longlong_as_double((long long)last_key);
    bool unsafe;
    const double band = cert_band(a_m, band_rel, unsafe);
    const double mlat = G(p.cc_lat)[ls], mlon = G(p.cc_lon)[ls];  // uniform loads
    if (unsafe) uncertain = 1;
    for (uint32_t i = tid; i < n_it; i += CARVE_THREADS) {
      const uint32_t s = slot_of(i);
      const uint64_t k = l_key[i];
      const uint64_t kb = (k >> SB) << SB;
      const double a = __longlong_as_double((long long)kb);
      const bool near = k != ~0ull && kb != noloc_key && fabs(a - a_m) <= band;
      if (near && (G(p.cc_lat)[s] != mlat || G(p.cc_lon)[s] != mlon)) uncertain = 1;
    }
  }
  const uint64_t ub = __ballot(uncertain != 0);
  if (lane == 0) red.flag[wave] = ub != 0ull;
  lds_barrier();
  uint32_t any = 0;
#pragma unroll
  for (uint32_t k = 0; k < CARVE_WAVES; ++k) any |= red.flag[k];
  if (any) return STEP_UNCERTAIN;
  if (!step_room(c, total, p.cap_groups, p.cap_members)) return STEP_OVERFLOW;

  // ---- commit: selected slots = seed + every key <= last.  Each wave owns whole bitmap words (slot>>6 == j*16 +
  // wave): ballot writes them.
  if (SPARSE) {  // (a handful of bits among the live candidates: one atomic each, here and in the published copy)
    for (uint32_t i = tid; i < n_it; i += CARVE_THREADS) {
      const uint32_t s = slot_of(i);
      if (s == seed || (n_sel > 0 && l_key[i] <= last)) {
        atomicAnd((unsigned long long*)&l_alive[s >> 6], ~(1ull << (s & 63u)));
        if (mirror) __hip_atomic_fetch_and(&mirror[s >> 6], ~(1ull << (s & 63u)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  } else {
    for (uint32_t wj = wave; wj < lw; wj += CARVE_WAVES) {  // wave-uniform
      const uint32_t s = wj * 64u + lane;
      const bool was = bit_at(l_alive, s);
      const bool sel = was && (s == seed || (n_sel > 0 && l_key[s] <= last));
      const uint64_t nw = __ballot(was && !sel);
      const uint64_t ow = __ballot(was);
      if (lane == 0) {
        l_alive[wj] = nw;
        // (streaming carve: the published bitmap of free positions follows every removal — it holds every
        // configuration's candidates, so only the bits this step took are cleared)
        if (mirror && ow != nw) __hip_atomic_fetch_and(&mirror[wj], ~(ow ^ nw), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  if (wave == 0) {  // group record + members: LDS -> fire-and-forget global stores
    if (lane == 0) {
      G(p.members)[c.mem_off] = wid_of(seed);
      step_record(G(p.g_cfg), G(p.g_n), G(p.g_off), c.n_groups, c.cfg, total, c.mem_off);
    }
    const uint32_t lim = n_sel < PM_CARVE_SEL_CAP ? n_sel : PM_CARVE_SEL_CAP;
    for (uint32_t r = lane; r < lim; r += 64u) G(p.members)[c.mem_off + 1u + r] = wid_of(sel_out[r]);
  }
  lds_barrier();
  PROF_MARK(22);  // one exact step
  step_book(c, total);
  return STEP_CONTINUE;
}

// LDS carve of one candidate list of at most PM_CARVE_SLOTS slots: worker ids, site ids, packed keys,
// the alive / loc bitmaps and the per-wave partial selections all live in LDS (slot s is owned by thread
// s % CARVE_THREADS).  Fast steps come from the proposals; a slow step is the exact full sweep: keys for every
// live candidate, two-level selection (DPP argmin rounds per wave, 8-way merge), certificate, commit —
// three LDS-only barriers.  Runs until the configuration is exhausted, a recompaction is due, or a step
// cannot be certified.
template <bool BIG>
__device__ __noinline__ int carve_run_lds(const CarveArgs& p, BlockRed& red, StepCtx& c, const uint32_t* l_wid,
                                          const uint32_t* l_site, uint64_t* l_key, uint64_t* l_alive,
                                          const uint64_t* l_loc, uint64_t* part, uint32_t* sel_out,
                                          uint32_t* l_stage, uint32_t steps_before) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const bool have_props = c.mode == CARVE_MODE_FORM && c.use_props;
  uint32_t seed_cur = 0;  // wave 0: how far into the batch's seed list the carve has come
  const ChainLds CL = chain_lds(l_stage);
  for (;;) {
    if (have_props) {
      // Everything the proposals can serve is done by wave 0 alone (everyone else waits at the barrier): the chain
      // of located steps (carve_chain), and — with the row's keys at hand — whatever it hands over: rows whose
      // flags do not settle the certificate, exhausted rows, the last partial group, the first-come tail.
      const bool chain = c.prop_k && c.proximity && c.max_s - 1u < PM_PROP_KMAX;
      if (chain) {  // the control block of the chain (an exact step in between has used the key array it lives in)
        if (tid < 16u) cc_st(&CL.CC[tid], 0u);
        lds_barrier();
      }
      if (wave == 0) {
        PROF_DECL;
        int act = FAST_SEQ;
        uint32_t cmd_seq = 0u;  // commands to the producer are numbered
        for (;;) {
          if (chain) {
            act = carve_chain<BIG>(p, c, l_stage, steps_before, seed_cur, cmd_seq);
            PROF_MARK(0);
            if (act == FAST_OVERFLOW || act == FAST_REPROPOSE || act == FAST_ABORT) break;
          }
          act = carve_fast_steps<BIG>(p, c, l_site, l_alive, l_loc, steps_before, seed_cur,
                                      (chain && act == FAST_SLOW) ? 1u : 0xFFFFFFFFu);
          if (act != FAST_AGAIN) break;
        }
        if (chain && lane == 0) cc_st(&CL.CC[CC_CMD], (cmd_seq + 4u) | CH_QUIT);  // waves 1 and 2 come to the barrier
        if (lane == 0) {
          red.f_action = (uint32_t)act;
          red.f_n_cand = c.n_cand;
          red.f_total_available = c.total_available;
          red.f_n_groups = c.n_groups;
          red.f_mem_off = c.mem_off;
          red.f_steps = c.steps;
          red.f_fast = c.fast_steps;
          red.f_cand_sum = c.cand_sum;
        }
        PROF_MARK(11);
      } else if (wave == 1 && chain) {
        carve_chain_produce<BIG>(p, c, l_alive, l_stage);
      } else if (wave == 2 && chain) {
        carve_chain_collect<BIG>(p, c, l_stage);
      }
      lds_barrier();
      const uint32_t act = red.f_action;
      c.n_cand = red.f_n_cand;
      c.total_available = red.f_total_available;
      c.n_groups = red.f_n_groups;
      c.mem_off = red.f_mem_off;
      c.steps = red.f_steps;
      c.fast_steps = red.f_fast;
      c.cand_sum = red.f_cand_sum;
      lds_barrier();  // the mailbox is rewritten after the next slow step
      if (act == FAST_DONE) return STEP_BREAK;
      if (act == FAST_OVERFLOW) return STEP_OVERFLOW;
      if (act == FAST_ABORT) return STEP_ABORT;
      if (act == FAST_REPROPOSE) return STEP_CONTINUE;  // re-prepare: next proposal batch
    }
    {
      const int rc = carve_exact_step<BIG>(p, red, c, l_wid, l_key, l_alive, l_loc, part, sel_out, steps_before, nullptr);
      if (rc != STEP_CONTINUE) return rc;
    }
    // drop dead slots once more than half of the list is gone.  With proposals this also ends the launch:
    // the list is re-prepared and the next propose / validate pair continues with fresh neighbour lists.
    if (c.n_cand * (have_props ? PM_THIN_DIV : 2u) < (have_props ? c.n_start : c.n_list) && c.n_list > (have_props ? 256u : CARVE_THREADS)) {
      if (tid == 0) p.status->why[2] += 1u;
      return STEP_CONTINUE;
    }
  }
}

// ---- generic path for candidate lists that do not fit the LDS/register scheme (> PM_CARVE_SLOTS):
// packed keys, positions and bitmaps live in HBM/L2; one workgroup-wide argmin round per member.
__device__ __noinline__ int carve_step_mem(const CarveArgs& p, BlockRed& red, StepCtx& c, uint64_t* part, uint64_t* key,
                              const uint32_t* wid, uint64_t* alive, const uint64_t* loc, uint32_t steps_before) {
  if (!step_open(c, c.mode == CARVE_MODE_MERGE)) return STEP_BREAK;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  constexpr uint32_t SB = PM_CARVE_SLOT_BITS_MEM;
  const uint32_t lw = (c.n_list + 63u) >> 6;
  uint32_t f_loc = PM_NONE, f_any = PM_NONE;
  for (uint32_t j = tid; j < lw; j += CARVE_THREADS) {
    const uint64_t al = alive[j];
    if (al && f_any == PM_NONE) f_any = j * 64u + __builtin_ctzll(al);
    const uint64_t ll = al & loc[j];
    if (ll && f_loc == PM_NONE) f_loc = j * 64u + __builtin_ctzll(ll);
  }
  f_loc = wave_min(f_loc);
  f_any = wave_min(f_any);
  if (lane == 0) {
    red.a[wave] = f_loc;
    red.b[wave] = f_any;
  }
  __syncthreads();
  f_loc = PM_NONE;
  f_any = PM_NONE;
  for (uint32_t k = 0; k < CARVE_WAVES; ++k) {
    f_loc = min(f_loc, red.a[k]);
    f_any = min(f_any, red.b[k]);
  }
  __syncthreads();
  const uint32_t want = step_want(c);
  uint32_t seed = f_any;
  bool use_dist = false, located_only = false;
  uint64_t last = 0;
  uint32_t n_sel = 0, total = 0;
  for (int attempt = 0; attempt < 2; ++attempt) {
    if (c.mode == CARVE_MODE_FORM) {
      if (attempt == 1) break;
      seed = f_any;
      use_dist = false;
      if (c.proximity && f_loc != PM_NONE) {
        seed = f_loc;
        use_dist = true;
      }
      located_only = false;
    } else if (attempt == 0) {
      if (!(c.proximity && f_loc != PM_NONE)) continue;
      seed = f_loc;
      use_dist = true;
      located_only = true;
    } else {
      if (!(total == 0 || (total < c.max_s && total < c.min_s))) break;
      seed = f_any;
      use_dist = false;
      located_only = false;
    }
    const double slat = G(p.cc_lat)[seed], slon = G(p.cc_lon)[seed], scos = G(p.cc_cos)[seed];
    uint64_t lmin = ~0ull;
    for (uint32_t s = tid; s < c.n_list; s += CARVE_THREADS) {
      uint64_t k = ~0ull;
      if (s != seed && bit_at(alive, s)) {
        if (!use_dist) {
          k = s;
        } else if (bit_at(loc, s)) {
          k = pack_key((uint64_t)__double_as_longlong(hav_a(slat, slon, scos, G(p.cc_lat)[s], G(p.cc_lon)[s], G(p.cc_cos)[s])), s, SB);
        } else if (!located_only) {
          k = pack_key(PM_KEY_NOLOC, s, SB);
        }
      }
      key[s] = k;
      lmin = k < lmin ? k : lmin;
    }
    n_sel = 0;
    last = 0;
    while (n_sel < want) {
      const uint64_t v = wave_min_u64(lmin);
      if (lane == 0) part[wave] = v;
      __syncthreads();
      uint64_t b = ~0ull;
      for (uint32_t k = 0; k < CARVE_WAVES; ++k) b = part[k] < b ? part[k] : b;
      __syncthreads();
      if (b == ~0ull) break;
      if (tid == 0 && c.mem_off + 1u + n_sel < p.cap_members)
        G(p.members)[c.mem_off + 1u + n_sel] = wid[(uint32_t)(b & ((1ull << SB) - 1ull))];
      last = b;
      ++n_sel;
      if (lmin == b) {
        uint64_t m = ~0ull;
        for (uint32_t s = tid; s < c.n_list; s += CARVE_THREADS) {
          const uint64_t k = key[s];
          m = (k > b && k < m) ? k : m;
        }
        lmin = m;
      }
    }
    total = 1u + n_sel;
    if (c.mode == CARVE_MODE_FORM) break;
  }
  if (total == 0) return STEP_BREAK;
  if (c.mode == CARVE_MODE_FORM && total < c.min_s) return STEP_BREAK;
  if (c.mode == CARVE_MODE_MERGE && total < 2u) return STEP_BREAK;

  int uncertain = step_forced(p.debug_uncertain_every, steps_before + c.steps) && use_dist;
  const uint64_t last_key = (last >> SB) << SB;
  if (use_dist && n_sel > 0 && last_key != ((PM_KEY_NOLOC >> SB) << SB)) {
    const uint32_t ls = (uint32_t)(last & ((1ull << SB) - 1ull));
    const double a_m = __longlong_as_double((long long)last_key);
    bool unsafe;
    const double band = cert_band(a_m, PM_TIE_BAND_MEM, unsafe);
    const double mlat = G(p.cc_lat)[ls], mlon = G(p.cc_lon)[ls];
    if (unsafe) uncertain = 1;
    for (uint32_t s = tid; s < c.n_list; s += CARVE_THREADS) {
      const uint64_t k = key[s];
      if (k == ~0ull || s == ls) continue;
      const uint64_t kb = (k >> SB) << SB;
      if (kb == ((PM_KEY_NOLOC >> SB) << SB)) continue;
      const double a = __longlong_as_double((long long)kb);
      if (fabs(a - a_m) <= band && (G(p.cc_lat)[s] != mlat || G(p.cc_lon)[s] != mlon)) uncertain = 1;
    }
  }
  if (__syncthreads_or(uncertain)) return STEP_UNCERTAIN;
  if (!step_room(c, total, p.cap_groups, p.cap_members)) return STEP_OVERFLOW;
  for (uint32_t s = tid; s < c.n_list; s += CARVE_THREADS) {
    if (!bit_at(alive, s)) continue;
    if (s == seed || (n_sel > 0 && key[s] <= last))
      atomicAnd((unsigned long long*)&alive[s >> 6], ~(1ull << (s & 63u)));
  }
  if (tid == 0) {
    G(p.members)[c.mem_off] = wid[seed];
    step_record(G(p.g_cfg), G(p.g_n), G(p.g_off), c.n_groups, c.cfg, total, c.mem_off);
  }
  __syncthreads();
  step_book(c, total);
  return STEP_CONTINUE;
}

// Stable compaction of the live positions of this configuration into list slots: two passes over
// contiguous per-wave ranges.  Returns the list length; red.a keeps the per-wave counts for the placement.
__device__ __noinline__ uint32_t carve_compact_count(const CarveArgs& p, BlockRed& red, uint32_t n, uint64_t cbit,
                                                      const uint64_t* alive_bits) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t n_words = (n + 63u) >> 6;
  const uint32_t wpw = (n_words + CARVE_WAVES - 1u) / CARVE_WAVES;
  const uint32_t j0 = wave * wpw, j1 = min(n_words, j0 + wpw);
  uint32_t cnt = 0;
  const bool merge = p.mode == CARVE_MODE_MERGE;
  const auto alive_g = G(alive_bits);
  const auto c_compat = G((const uint64_t*)p.c_compat);
  for (uint32_t jb = j0; jb < j1; jb += 8u) {  // eight words per batch; every load unconditional (clamped
    uint64_t aw[8], cm[8];                     // index) and independent, so the whole batch is in flight at once
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const uint32_t j = jb + (uint32_t)u;
      const uint32_t i = j * 64u + lane;
      aw[u] = alive_g[j < n_words ? j : n_words - 1u];
      cm[u] = merge ? ~0ull : c_compat[i < n ? i : n - 1u];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const uint32_t j = jb + (uint32_t)u;
      const uint32_t i = j * 64u + lane;
      const bool c = j < j1 && i < n && ((aw[u] >> lane) & 1ull) && (cm[u] & cbit) != 0ull;
      cnt += __popcll(__ballot(c));
    }
  }
  __syncthreads();  // previous users of red.a are done
  if (lane == 0) red.a[wave] = cnt;
  __syncthreads();
  uint32_t total = 0;
  for (uint32_t k = 0; k < CARVE_WAVES; ++k) total += red.a[k];
  return total;
}

__device__ __noinline__ void carve_compact_place(const CarveArgs& p, BlockRed& red, uint32_t n, uint64_t cbit, uint32_t n_list,
                                                  const uint64_t* alive_bits) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t n_words = (n + 63u) >> 6;
  const uint32_t wpw = (n_words + CARVE_WAVES - 1u) / CARVE_WAVES;
  const uint32_t j0 = wave * wpw, j1 = min(n_words, j0 + wpw);
  const auto alive = G(p.bits_scratch);
  const auto loc = G(p.bits_scratch) + p.bits_stride;
  uint32_t off = 0;
  for (uint32_t k = 0; k < wave; ++k) off += red.a[k];
  const bool merge = p.mode == CARVE_MODE_MERGE;
  const auto alive_g = G(alive_bits);
  const auto c_compat = G((const uint64_t*)p.c_compat);
  for (uint32_t jb = j0; jb < j1; jb += 4u) {
    uint64_t aw[4], cm[4], lg[4];
    uint32_t ow[4], os[4];
    double la[4], lo[4], co[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {  // every load of the batch first, unconditional (clamped index)
      const uint32_t j = jb + (uint32_t)u;
      const uint32_t i = j * 64u + lane;
      const uint32_t ic = i < n ? i : n - 1u;
      aw[u] = alive_g[j < n_words ? j : n_words - 1u];
      lg[u] = G(p.loc_g)[j < n_words ? j : n_words - 1u];
      cm[u] = merge ? ~0ull : c_compat[ic];
      ow[u] = G(p.order)[ic];
      os[u] = G(p.c_site)[ic];
      la[u] = G(p.c_lat)[ic];
      lo[u] = G(p.c_lon)[ic];
      co[u] = G(p.c_cos)[ic];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const uint32_t j = jb + (uint32_t)u;
      const uint32_t i = j * 64u + lane;
      const bool c = j < j1 && i < n && ((aw[u] >> lane) & 1ull) && (cm[u] & cbit) != 0ull;
      const uint64_t bal = __ballot(c);
      if (c) {
        const uint32_t s = off + __popcll(bal & ((1ull << lane) - 1ull));
        G(p.slot_pos)[s] = i | (((uint32_t)(lg[u] >> lane) & 1u) << 31);  // bit 31: has a location
        G(p.slot_wid)[s] = ow[u];
        G(p.cc_lat)[s] = la[u];
        G(p.cc_lon)[s] = lo[u];
        G(p.cc_cos)[s] = co[u];
        G(p.cc_site)[s] = os[u];
      }
      off += __popcll(bal);
    }
  }
  __syncthreads();
  const uint32_t lw = (n_list + 63u) >> 6;
  // slot bitmaps: alive = all ones, loc from bit 31 of slot_pos (four independent coalesced loads per step)
  for (uint32_t base = 0; base < lw * 64u; base += 4u * CARVE_THREADS) {
    uint32_t sp[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const uint32_t s = base + (uint32_t)u * CARVE_THREADS + tid;
      sp[u] = G(p.slot_pos)[s < n_list ? s : n_list - 1u];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const uint32_t s = base + (uint32_t)u * CARVE_THREADS + tid;
      const bool in = s < n_list;
      const uint64_t ba = __ballot(in), bl = __ballot(in && (sp[u] >> 31));
      if (lane == 0 && (s >> 6) < lw) {
        alive[s >> 6] = ba;
        loc[s >> 6] = bl;
      }
    }
  }
  __syncthreads();
}

