// pm_directory.inc — the node directory's kernels (included by pm_kernels.hip inside namespace pm): pm_directory of
// include/pm_engine.h, with their launchers.  They read the liveness ledger, the rollout ledger, the worker table's rank column
// and the host's groups, and write scratch of their own: a pure read.  Integers only: every result is a count or a copy, so
// nothing depends on the grid or on which wave meets which row.
//
// CLASSIFY.  One pass over [0, W): whether the query lists the row (its status bit, its membership), its class (Healthy,
// Discovered, the five middle statuses, Dead: the comparator of node_store.rs:195-206 has these four levels and no more), the
// census per status — reduced per wave by ballots, per workgroup in LDS, one atomic a bin and workgroup — and one flag per
// class, class-major: flag[c * W + w].  ONE exclusive scan over the PM_DC_N * W flags then gives every listed row its place in
// (class, row) order at off[cls * W + w]: the class's base and the row's rank inside the class in one word, and the total behind
// the last flag.  That is the whole of BY_ROW's order: a four-class ordered compaction, no sort.
//
// PLACE.  list_place(a, i): entry i's place in scan order, or PM_NONE where it is not listed (or no entry).  Every directory
// states its own once, and both its window and its keys kernel ask it.
//
// WINDOW (BY_ROW).  Only the rows whose place falls in [offset, offset + n_rows) write, their index into win[place - offset]:
// list_window_kernel, the one window kernel of the three directories, over the directory's argument block.
//
// KEYS (BY_ADDRESS).  Every listed row writes (class << 32 | rank, row) at its place; launch_ro_radix_pass then sorts the 34
// significant bits in five passes (stable, fixed chunks: ties keep (class, row) order, and the class is in the key, so ties
// fall back on the row index).  The window is a slice of the sorted rows.
//
// EMIT.  One thread per window slot: the row's ledgers, its group's record, one 48-byte row written whole.

// in a live group of the host's list
__device__ __forceinline__ bool dir_grouped(const DirArgs& a, int32_t g) {
  return g >= 0 && (uint32_t)g < a.G && a.g[g].slot != PM_NONE;
}

__device__ __forceinline__ uint32_t dir_class(uint32_t st) {
  return st == PM_NS_HEALTHY ? (uint32_t)PM_DC_HEALTHY : st == PM_NS_DISCOVERED ? (uint32_t)PM_DC_DISCOVERED
       : st == PM_NS_DEAD ? (uint32_t)PM_DC_DEAD : (uint32_t)PM_DC_OTHER;
}

__global__ __launch_bounds__(256) void dir_classify_kernel(DirArgs a) {
  __shared__ uint32_t s_bin[PM_NS_N];
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  if (tid < PM_NS_N) s_bin[tid] = 0u;
  __syncthreads();
  const uint32_t w = blockIdx.x * 256u + tid;
  uint32_t st_bin = PM_NONE;  // (PM_NONE: this lane counts nothing)
  if (w < a.W) {
    const uint32_t st = a.status[w];
    const bool grouped = dir_grouped(a, a.group_of[w]);
    const bool member_ok = a.membership == PM_DIR_ANY || (a.membership == PM_DIR_GROUPED) == grouped;
    const bool pass = st < PM_NS_N && ((a.status_mask >> st) & 1u) != 0u && member_ok;
    const uint32_t cls = pass ? dir_class(st) : PM_DIR_NO_CLASS;
    if (pass) st_bin = st;
    a.cls[w] = (uint8_t)cls;
#pragma unroll
    for (uint32_t c = 0; c < PM_DC_N; ++c) a.flag[(size_t)c * a.W + w] = cls == c ? 1u : 0u;
  }
  for (uint32_t s = 0; s < PM_NS_N; ++s) {
    const uint64_t m = __ballot(st_bin == s);
    if (lane == 0u && m) atomicAdd(&s_bin[s], (uint32_t)__popcll(m));
  }
  __syncthreads();
  if (tid < PM_NS_N && s_bin[tid]) atomicAdd(&a.census[tid], s_bin[tid]);
}

__device__ __forceinline__ uint32_t list_place(const DirArgs& a, uint32_t w) {
  if (w >= a.W) return PM_NONE;
  const uint32_t cls = a.cls[w];
  return cls < PM_DC_N ? a.off[(size_t)cls * a.W + w] : PM_NONE;
}

// Args: a directory's argument block — list_place(a, i), and offset, n_rows, win
template <class Args>
__global__ __launch_bounds__(256) void list_window_kernel(Args a) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const uint32_t at = list_place(a, i);
  if (at != PM_NONE && at >= a.offset && at - a.offset < a.n_rows) a.win[at - a.offset] = i;
}

__global__ __launch_bounds__(256) void dir_keys_kernel(DirArgs a) {
  const uint32_t w = blockIdx.x * 256u + threadIdx.x;
  const uint32_t at = list_place(a, w);
  if (at == PM_NONE) return;
  a.key[at] = ((uint64_t)a.cls[w] << 32) | a.addr_rank[w];
  a.val[at] = w;
}

__global__ __launch_bounds__(256) void dir_emit_kernel(DirArgs a, const uint32_t* __restrict__ list, uint32_t n,
                                                       pm_dir_row* __restrict__ rows) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n) return;
  const uint32_t w = list[k];
  pm_dir_row o;
  o.worker = w;
  o.status = a.status[w];
  o.cls = (uint8_t)dir_class(o.status);
  o.state = a.state ? a.state[w] : (uint8_t)PM_TS_NONE;
  o._pad = 0;
  o.counter = a.counter[w];
  o.group_slot = PM_NONE;
  o.group_id = (uint64_t)PM_NONE;
  o.group_size = 0u;
  o.config = 0u;
  o.task = PM_NONE;
  const int32_t g = a.group_of[w];
  if (dir_grouped(a, g)) {
    const DirGroup gr = a.g[g];
    o.group_slot = gr.slot;
    o.group_id = gr.id;
    o.group_size = gr.size;
    o.config = gr.cfg;
    o.task = gr.task;
  }
  o._pad2 = 0u;
  o.uid = a.uid ? a.uid[w] : 0ull;
  rows[k] = o;
}

void launch_dir_classify(const DirArgs& a, hipStream_t s) {
  if (!a.W) return;
  hipLaunchKernelGGL(dir_classify_kernel, dim3((a.W + 255u) / 256u), dim3(256), 0, s, a);
}

template <class Args>
void launch_list_window(const Args& a, uint32_t n_index, hipStream_t s) {
  if (!n_index || !a.n_rows) return;
  hipLaunchKernelGGL(list_window_kernel<Args>, dim3((n_index + 255u) / 256u), dim3(256), 0, s, a);
}
// one instantiation a directory, behind its list_place: here, in pm_groupdir.inc and in pm_taskdir.inc (a new directory: its
// kernel file behind this one, a list_place overload for its Args, one such line)
template void launch_list_window<DirArgs>(const DirArgs&, uint32_t, hipStream_t);

void launch_dir_keys(const DirArgs& a, hipStream_t s) {
  if (!a.W) return;
  hipLaunchKernelGGL(dir_keys_kernel, dim3((a.W + 255u) / 256u), dim3(256), 0, s, a);
}

void launch_dir_emit(const DirArgs& a, const uint32_t* list, uint32_t n, pm_dir_row* rows, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(dir_emit_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, a, list, n, rows);
}
