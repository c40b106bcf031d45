// pm_groupdir.inc — the group directory's kernels (included by pm_kernels.hip inside namespace pm, behind pm_directory.inc):
// pm_group_directory of include/pm_engine.h, with their launchers.  They read the liveness ledger, the rollout ledger and the
// host's groups, and write scratch of their own: a pure read.  Integers only: every result is a count or a copy, so nothing
// depends on the grid or on which wave meets which row.
//
// MEMBERS.  One pass over [0, W): a row of a live group adds one to the group's counter word of its liveness status and, where
// the group holds a task, to the word of its rollout relation — ro_member_class of pm_rollout.inc, the rule of
// ro_classify_kernel, asked, not copied.  A group's members are often neighbours in a wave: the lanes that hit one word send
// one atomic (wave_add_words).  Integer sums: the words are the same whatever order the atomics land in.
//
// GROUPS.  One pass over the list, tombstones included, behind the member pass on the stream: the health class and the
// rollout class from the complete counters, the filter, the census — per configuration in LDS, per class by ballots, the
// members by a wave sum; one global atomic a non-zero bin and workgroup — and one flag per class of the chosen order,
// class-major: flag[c * G + k].  BY_SLOT and BY_SIZE_DESC have one class; BY_ID_TEXT has sixteen, the id's hex digits L.  ONE
// exclusive scan over the flags gives every listed entry its place in (class, slot) order and the total behind the last flag.
//
// ORDER.  BY_SLOT: the scan is the order; the entries whose place falls in the window write their index (list_window_kernel of
// pm_directory.inc over list_place below).  BY_ID_TEXT: the text
// order of format!("{:x}", id) is (A, L) ascending, A = id << 4 (16 - L) (DESIGN 4.x has the proof).  The entries stand in
// (L, slot) order behind the compaction; eight stable radix passes over A (launch_ro_radix_pass: fixed chunks, ties keep
// entry order) leave them in (A, L, slot) order.  A and L together are 68 bits; L never enters the key.  BY_SIZE_DESC: four
// stable passes over UINT32_MAX - size.  The window is a slice of the sorted entries.
//
// EMIT.  One thread per window slot: the entry's record, its classes, its counters, one 80-byte row written whole.

__device__ __forceinline__ uint32_t gdir_hex_digits(uint64_t id) {
  return id ? (67u - (uint32_t)__builtin_clzll(id)) >> 2 : 1u;  // ceil(bits / 4); 0 is "0"
}

__global__ __launch_bounds__(256) void gdir_member_kernel(GdirArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t w = blockIdx.x * 256u + threadIdx.x;
  uint32_t w_status = PM_NONE, w_rollout = PM_NONE;  // (PM_NONE: this lane counts nothing)
  if (w < a.W) {
    const int32_t g = a.group_of[w];
    if (g >= 0 && (uint32_t)g < a.G) {
      const RoGroup gr = a.g[g];
      if (gr.slot != PM_NONE) {  // (a tombstone's rows keep a stale group_of only under a stepwise tick; skipped all the same)
        if (a.status) {
          const uint32_t st = a.status[w];
          if (st < PM_NS_N) w_status = (uint32_t)g * PM_GD_CNT + st;
        }
        if (a.state && gr.task != PM_NONE) {
          const uint32_t cls = ro_member_class(a.state[w], a.uid[w], gr.uid);
          w_rollout = (uint32_t)g * PM_GD_CNT + PM_NS_N + (uint32_t)PM_RO_CONVERGED - cls;  // converged, behind, other, silent
        }
      }
    }
  }
  wave_add_words(a.g_cnt, w_status, lane);
  wave_add_words(a.g_cnt, w_rollout, lane);
}

__device__ __forceinline__ uint32_t gdir_health(const uint32_t* __restrict__ c) {
  const uint32_t lost = c[PM_NS_DEAD] + c[PM_NS_EJECTED] + c[PM_NS_BANNED] + c[PM_NS_LOWBALANCE];
  const uint32_t weak = c[PM_NS_DISCOVERED] + c[PM_NS_WAITING] + c[PM_NS_UNHEALTHY];
  return lost ? (uint32_t)PM_GH_LOST : weak ? (uint32_t)PM_GH_DEGRADED : (uint32_t)PM_GH_SOUND;
}

__global__ __launch_bounds__(256) void gdir_group_kernel(GdirArgs a) {
  __shared__ uint32_t s_bin[PM_GD_CENSUS];
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  if (tid < PM_GD_CENSUS) s_bin[tid] = 0u;
  __syncthreads();
  const uint32_t k = blockIdx.x * 256u + tid;
  uint32_t h_bin = PM_NONE, r_bin = PM_NONE, members = 0u;  // (PM_NONE: this lane counts nothing)
  if (k < a.G) {
    const RoGroup gr = a.g[k];
    const uint32_t* c = a.g_cnt + (size_t)k * PM_GD_CNT;
    const bool live = gr.slot != PM_NONE, held = gr.task != PM_NONE;
    const uint32_t health = !a.status ? PM_GH_NONE : gdir_health(c);
    const uint32_t rollout = !a.state ? PM_GR_NONE
                           : !held ? (uint32_t)PM_GR_NO_TASK
                           : c[PM_NS_N] == gr.size ? (uint32_t)PM_GR_CONVERGED : (uint32_t)PM_GR_ROLLING;
    bool pass = live && gr.cfg < PM_MAX_CONFIGS && ((a.config_mask >> gr.cfg) & 1ull) != 0ull;
    pass = pass && (a.holds == PM_GDIR_ANY || (a.holds == PM_GDIR_WITH_TASK) == held);
    pass = pass && gr.size >= a.size_min && gr.size <= a.size_max;
    pass = pass && (!a.status || ((a.health_mask >> health) & 1u) != 0u);
    pass = pass && (!a.state || ((a.rollout_mask >> rollout) & 1u) != 0u);
    const uint32_t cls = !pass ? PM_GD_NO_CLASS : a.order == PM_GDIR_BY_ID_TEXT ? gdir_hex_digits(gr.id) - 1u : 0u;
    a.cls[k] = (uint8_t)cls;
    a.hr[2u * k] = (uint8_t)health;
    a.hr[2u * k + 1u] = (uint8_t)rollout;
    for (uint32_t q = 0; q < a.n_cls; ++q) a.flag[(size_t)q * a.G + k] = cls == q ? 1u : 0u;
    if (pass) {
      atomicAdd(&s_bin[gr.cfg], 1u);
      if (a.status) h_bin = health;
      if (a.state) r_bin = rollout;
      members = gr.size;
    }
  }
  for (uint32_t h = 0; h < PM_GH_N; ++h) {
    const uint64_t m = __ballot(h_bin == h);
    if (lane == 0u && m) atomicAdd(&s_bin[PM_MAX_CONFIGS + h], (uint32_t)__popcll(m));
  }
  for (uint32_t r = 0; r < PM_GR_N; ++r) {
    const uint64_t m = __ballot(r_bin == r);
    if (lane == 0u && m) atomicAdd(&s_bin[PM_MAX_CONFIGS + PM_GH_N + r], (uint32_t)__popcll(m));
  }
#pragma unroll
  for (uint32_t m = 32u; m; m >>= 1) members += (uint32_t)__shfl_xor((int)members, (int)m);
  if (lane == 0u && members) atomicAdd(&s_bin[PM_GD_CENSUS - 1u], members);
  __syncthreads();
  if (tid < PM_GD_CENSUS && s_bin[tid]) atomicAdd(&a.census[tid], s_bin[tid]);
}

__device__ __forceinline__ uint32_t list_place(const GdirArgs& a, uint32_t k) {
  if (k >= a.G) return PM_NONE;
  const uint32_t cls = a.cls[k];
  return cls < a.n_cls ? a.off[(size_t)cls * a.G + k] : PM_NONE;
}

__global__ __launch_bounds__(256) void gdir_keys_kernel(GdirArgs a) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  const uint32_t at = list_place(a, k);
  if (at == PM_NONE) return;
  const uint32_t cls = a.cls[k];
  const RoGroup gr = a.g[k];
  // BY_ID_TEXT: the id's digits pushed to the top (L = cls + 1 of them; 0 stays 0).  BY_SIZE_DESC: largest first.
  a.key[at] = a.order == PM_GDIR_BY_ID_TEXT ? gr.id << (4u * (PM_GD_TEXT_CLASSES - 1u - cls)) : (uint64_t)(0xFFFFFFFFu - gr.size);
  a.val[at] = k;
}

__global__ __launch_bounds__(256) void gdir_emit_kernel(GdirArgs a, const uint32_t* __restrict__ list, uint32_t n,
                                                        pm_gdir_row* __restrict__ rows) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t k = list[i];
  const RoGroup gr = a.g[k];
  const uint32_t* c = a.g_cnt + (size_t)k * PM_GD_CNT;
  pm_gdir_row o;
  o.group_id = gr.id;
  o.slot = gr.slot;
  o.config = gr.cfg;
  o.size = gr.size;
  o.task = gr.task;
  o.member_begin = 0u;  // (the host's, with the members)
  o.health = a.hr[2u * k];
  o.rollout = a.hr[2u * k + 1u];
  o._pad = 0;
#pragma unroll
  for (uint32_t s = 0; s < PM_NS_N; ++s) o.by_status[s] = c[s];
  o.converged = c[PM_NS_N];
  o.behind = c[PM_NS_N + 1u];
  o.other = c[PM_NS_N + 2u];
  o.silent = c[PM_NS_N + 3u];
  rows[i] = o;
}

void launch_gdir_members(const GdirArgs& a, hipStream_t s) {
  if (!a.W || !a.G || (!a.status && !a.state)) return;
  hipLaunchKernelGGL(gdir_member_kernel, dim3((a.W + 255u) / 256u), dim3(256), 0, s, a);
}

void launch_gdir_groups(const GdirArgs& a, hipStream_t s) {
  if (!a.G) return;
  hipLaunchKernelGGL(gdir_group_kernel, dim3((a.G + 255u) / 256u), dim3(256), 0, s, a);
}

// (the template stands in pm_directory.inc, included in front of this file; it finds list_place above by its argument's type)
template void launch_list_window<GdirArgs>(const GdirArgs&, uint32_t, hipStream_t);

void launch_gdir_keys(const GdirArgs& a, hipStream_t s) {
  if (!a.G) return;
  hipLaunchKernelGGL(gdir_keys_kernel, dim3((a.G + 255u) / 256u), dim3(256), 0, s, a);
}

void launch_gdir_emit(const GdirArgs& a, const uint32_t* list, uint32_t n, pm_gdir_row* rows, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(gdir_emit_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, a, list, n, rows);
}
