// pm_addresses.inc — part of pm_kernels.hip (included in place, namespace pm, behind pm_keccak.inc and pm_rollout.inc): the
// address book.  A node's rank is its place in a BTreeSet<String> of address.to_string() (node_groups/mod.rs:424-434), and that
// string is the EIP-55 text: the case of hex letter i is nibble i of keccak-256(the 40 lower-case hex characters) >= 8.
//
// Per row: the 20 bytes, the 40-bit case mask, and the text as an ORDER-PRESERVING KEY — 5 bits a character ('0'-'9' -> 0-9,
// 'A'-'F' -> 10-15, 'a'-'f' -> 16-21: the byte order of the three ranges), most significant character first, 10 characters a
// 64-bit word, PM_AB_WORDS words.  Comparing the words in order as integers is comparing the texts as byte strings.
//
// The rank: a stable sort of (key, row) by the ledgers' radix pass (launch_ro_radix_pass).  Shallow path: by word 0 alone (the
// first 10 characters; 7 passes of 8 bits over its 50); when no two neighbours of the result share word 0 — the only case
// random addresses produce — the order is final.  Deep path: least significant word first over all words (28 passes).  Both
// begin in row order and every pass is stable, so equal texts stay in ascending row order.

// 8 characters of the lower-case hex text of bytes b0..b3 (in address order) as one little-endian word
__device__ __forceinline__ uint32_t ab_hex_char(uint32_t nib) { return nib < 10u ? 0x30u + nib : 0x57u + nib; }
__device__ __forceinline__ uint64_t ab_hex_lane(uint32_t w) {  // w: 4 address bytes, the first in the low byte
  uint64_t v = 0ull;
#pragma unroll
  for (uint32_t k = 0; k < 4u; ++k) {
    const uint32_t b = (w >> (8u * k)) & 255u;
    v |= (uint64_t)ab_hex_char(b >> 4) << (16u * k);
    v |= (uint64_t)ab_hex_char(b & 15u) << (16u * k + 8u);
  }
  return v;
}

// the 40-bit case mask of an address (a5[0..5): its bytes as five words): bit i = character i is an upper-case letter
__device__ __forceinline__ uint64_t ab_case_mask(const uint32_t a5[5]) {
  KcState st;
  kc_zero(st);
  st.s0 = ab_hex_lane(a5[0]);
  st.s1 = ab_hex_lane(a5[1]);
  st.s2 = ab_hex_lane(a5[2]);
  st.s3 = ab_hex_lane(a5[3]);
  st.s4 = ab_hex_lane(a5[4]);
  st.s5 = 0x01ull;         // (byte 40: the padding's first byte)
  st.s16 = 0x80ull << 56;  // (byte 135: its last)
  keccak_f1600(st);
  // digest byte j is byte j of (s0, s1, s2) little-endian; nibble 2 j is its high half
  uint64_t mask = 0ull;
#pragma unroll
  for (uint32_t i = 0; i < 40u; ++i) {
    const uint32_t j = i >> 1;
    const uint64_t word = j < 8u ? st.s0 : (j < 16u ? st.s1 : st.s2);
    const uint32_t byte = (uint32_t)(word >> (8u * (j & 7u))) & 255u;
    const uint32_t hn = (i & 1u) ? (byte & 15u) : (byte >> 4);
    const uint32_t an = (a5[j >> 2] >> (8u * (j & 3u) + ((i & 1u) ? 0u : 4u))) & 15u;
    if (an >= 10u && hn >= 8u) mask |= 1ull << i;
  }
  return mask;
}

// one lane an address: in[20 k ..) -> row first + k
__global__ __launch_bounds__(64) void ab_set_kernel(const uint32_t* __restrict__ in, uint32_t first, uint32_t n, uint32_t* __restrict__ bytes,
                                                    uint64_t* __restrict__ mask, uint64_t* __restrict__ key, uint8_t* __restrict__ set) {
  const uint32_t k = blockIdx.x * 64u + threadIdx.x;
  if (k >= n) return;
  const uint32_t row = first + k;
  uint32_t a5[5];
#pragma unroll
  for (uint32_t q = 0; q < 5u; ++q) a5[q] = in[5u * k + q];
  const uint64_t m = ab_case_mask(a5);
#pragma unroll
  for (uint32_t w = 0; w < PM_AB_WORDS; ++w) {
    uint64_t kw = 0ull;
#pragma unroll
    for (uint32_t c = 0; c < 10u; ++c) {
      const uint32_t i = 10u * w + c, j = i >> 1;
      const uint32_t nib = (a5[j >> 2] >> (8u * (j & 3u) + ((i & 1u) ? 0u : 4u))) & 15u;
      const uint32_t code = nib < 10u ? nib : (((m >> i) & 1ull) ? nib : nib + 6u);
      kw = (kw << 5) | code;
    }
    key[(size_t)row * PM_AB_WORDS + w] = kw;
  }
#pragma unroll
  for (uint32_t q = 0; q < 5u; ++q) bytes[5u * (size_t)row + q] = a5[q];
  mask[row] = m;
  set[row] = 1u;
}

// one lane an asked row: "0x", the 40 characters, a NUL
__global__ __launch_bounds__(256) void ab_text_kernel(const uint32_t* __restrict__ rows, uint32_t n, const uint32_t* __restrict__ bytes,
                                                      const uint64_t* __restrict__ mask, uint8_t* __restrict__ out) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n) return;
  const uint32_t row = rows ? rows[k] : k;
  const uint64_t m = mask[row];
  uint8_t* o = out + (size_t)k * PM_AB_TEXT;
  o[0] = 0x30u;
  o[1] = 0x78u;
  for (uint32_t q = 0; q < 5u; ++q) {
    const uint32_t w = bytes[5u * (size_t)row + q];
#pragma unroll
    for (uint32_t c = 0; c < 8u; ++c) {
      const uint32_t i = 8u * q + c;
      const uint32_t nib = (w >> (8u * (c >> 1) + ((c & 1u) ? 0u : 4u))) & 15u;
      o[2u + i] = (uint8_t)(nib < 10u ? 0x30u + nib : (((m >> i) & 1ull) ? 0x37u + nib : 0x57u + nib));
    }
  }
  o[42] = 0u;
}

// key[i] = word `word` of row val[i]'s key (val null: row i), val_out[i] = the row when asked
__global__ __launch_bounds__(256) void ab_gather_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ val, uint32_t W,
                                                        uint32_t word, uint64_t* __restrict__ key_out, uint32_t* __restrict__ val_out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= W) return;
  const uint32_t row = val ? val[i] : i;
  key_out[i] = row < W ? keys[(size_t)row * PM_AB_WORDS + word] : 0ull;
  if (val_out) val_out[i] = row;
}

// *ties += neighbours of the sorted array that share their key
__global__ __launch_bounds__(256) void ab_ties_kernel(const uint64_t* __restrict__ key, uint32_t W, uint32_t* __restrict__ ties) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
  const bool tie = i + 1u < W && key[i] == key[i + 1u];
  const uint64_t m = __ballot(tie);
  if (lane == 0u && m) atomicAdd(ties, (uint32_t)__popcll(m));
}

// rank[val[i]] = i: the engine's column, and a second copy for the caller
__global__ __launch_bounds__(256) void ab_rank_kernel(const uint32_t* __restrict__ val, uint32_t W, uint32_t* __restrict__ rank) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= W) return;
  const uint32_t row = val[i];
  if (row < W) rank[row] = i;
}

// set[first, end) = 0
__global__ __launch_bounds__(256) void ab_clear_kernel(uint8_t* __restrict__ set, uint32_t first, uint32_t end) {
  const uint32_t i = first + blockIdx.x * 256u + threadIdx.x;
  if (i < end) set[i] = 0u;
}

// 32 big-endian bytes of a 64-bit value, as the four little-endian words that hold them: three zero words, the value reversed
__device__ __forceinline__ uint64_t ab_bswap64(uint64_t v) {
  v = ((v & 0x00FF00FF00FF00FFull) << 8) | ((v >> 8) & 0x00FF00FF00FF00FFull);
  v = ((v & 0x0000FFFF0000FFFFull) << 16) | ((v >> 16) & 0x0000FFFF0000FFFFull);
  return (v << 32) | (v >> 32);
}

// one lane an asked row: d = keccak(be32(domain) | be32(pool) | address | nonce | be32(expiration)) (node/invite.rs:86-104: 148
// bytes, two blocks), s = keccak("\x19Ethereum Signed Message:\n32" | d) (sign_message's EIP-191 hash: 60 bytes)
__global__ __launch_bounds__(64) void invite_digest_kernel(const uint32_t* __restrict__ rows, uint32_t n, const uint32_t* __restrict__ bytes,
                                                           uint32_t domain_id, uint32_t pool_id, const uint64_t* __restrict__ nonce,
                                                           const uint64_t* __restrict__ expiration, uint64_t* __restrict__ digest,
                                                           uint64_t* __restrict__ signing) {
  const uint32_t k = blockIdx.x * 64u + threadIdx.x;
  if (k >= n) return;
  const uint32_t row = rows[k];
  uint32_t a[5];
#pragma unroll
  for (uint32_t q = 0; q < 5u; ++q) a[q] = bytes[5u * (size_t)row + q];
  const uint64_t n0 = nonce[4u * (size_t)k], n1 = nonce[4u * (size_t)k + 1u], n2 = nonce[4u * (size_t)k + 2u], n3 = nonce[4u * (size_t)k + 3u];
  // bytes [0, 32) domain, [32, 64) pool, [64, 84) address, [84, 116) nonce, [116, 148) expiration; words of 8 from 0:
  // 3 = domain, 7 = pool, 8, 9 and the low half of 10 = address, then the nonce shifted by four bytes
  KcState st;
  kc_zero(st);
  st.s3 = ab_bswap64((uint64_t)domain_id);
  st.s7 = ab_bswap64((uint64_t)pool_id);
  st.s8 = (uint64_t)a[0] | ((uint64_t)a[1] << 32);
  st.s9 = (uint64_t)a[2] | ((uint64_t)a[3] << 32);
  st.s10 = (uint64_t)a[4] | (n0 << 32);
  st.s11 = (n0 >> 32) | (n1 << 32);
  st.s12 = (n1 >> 32) | (n2 << 32);
  st.s13 = (n2 >> 32) | (n3 << 32);
  st.s14 = n3 >> 32;  // (bytes 112..115; 116..119 are zeros of the expiration)
  // words 15, 16: bytes 120..135 of the expiration's 24 leading zeros
  keccak_f1600(st);
  // second block: bytes 136..139 zero, 140..147 the expiration big-endian, 148 the padding's 0x01, byte 271 its 0x80
  const uint64_t ex = ab_bswap64(expiration[k]);
  st.s0 ^= ex << 32;
  st.s1 ^= (ex >> 32) | (0x01ull << 32);
  st.s16 ^= 0x80ull << 56;
  keccak_f1600(st);
  const uint64_t d0 = st.s0, d1 = st.s1, d2 = st.s2, d3 = st.s3;
  digest[4u * (size_t)k] = d0, digest[4u * (size_t)k + 1u] = d1, digest[4u * (size_t)k + 2u] = d2, digest[4u * (size_t)k + 3u] = d3;
  // "\x19Ethereum Signed Message:\n32": 28 bytes = three words and a half
  kc_zero(st);
  st.s0 = 0x7565726568744519ull;  // 19 'E' 't' 'h' 'e' 'r' 'e' 'u'
  st.s1 = 0x64656E676953206Dull;  // 'm' ' ' 'S' 'i' 'g' 'n' 'e' 'd'
  st.s2 = 0x6567617373654D20ull;  // ' ' 'M' 'e' 's' 's' 'a' 'g' 'e'
  st.s3 = 0x32330A3Aull | (d0 << 32);  // ':' '\n' '3' '2', then the digest
  st.s4 = (d0 >> 32) | (d1 << 32);
  st.s5 = (d1 >> 32) | (d2 << 32);
  st.s6 = (d2 >> 32) | (d3 << 32);
  st.s7 = (d3 >> 32) | (0x01ull << 32);  // (byte 60)
  st.s16 = 0x80ull << 56;
  keccak_f1600(st);
  signing[4u * (size_t)k] = st.s0, signing[4u * (size_t)k + 1u] = st.s1, signing[4u * (size_t)k + 2u] = st.s2,
  signing[4u * (size_t)k + 3u] = st.s3;
}

void launch_ab_set(const uint32_t* in, uint32_t first, uint32_t n, uint32_t* bytes, uint64_t* mask, uint64_t* key, uint8_t* set,
                   hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(ab_set_kernel, dim3((n + 63u) / 64u), dim3(64), 0, s, in, first, n, bytes, mask, key, set);
}

void launch_ab_text(const uint32_t* rows, uint32_t n, const uint32_t* bytes, const uint64_t* mask, uint8_t* out, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(ab_text_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, rows, n, bytes, mask, out);
}

void launch_ab_clear(uint8_t* set, uint32_t first, uint32_t end, hipStream_t s) {
  if (first >= end) return;
  hipLaunchKernelGGL(ab_clear_kernel, dim3((end - first + 255u) / 256u), dim3(256), 0, s, set, first, end);
}

uint32_t launch_ab_sort_shallow(const uint64_t* keys, uint32_t W, const RoSortBufs& b, uint32_t* ties, hipStream_t s) {
  if (!W) return 0u;
  const dim3 grid((W + 255u) / 256u);
  hipLaunchKernelGGL(ab_gather_kernel, grid, dim3(256), 0, s, keys, (const uint32_t*)nullptr, W, 0u, b.key[0], b.val[0]);
  const uint32_t cur = launch_ro_radix_sort(b, W, PM_AB_PASSES, 0u, s);
  hipLaunchKernelGGL(ab_ties_kernel, grid, dim3(256), 0, s, b.key[cur], W, ties);
  return cur;
}

uint32_t launch_ab_sort_deep(const uint64_t* keys, uint32_t W, const RoSortBufs& b, hipStream_t s) {
  if (!W) return 0u;
  const dim3 grid((W + 255u) / 256u);
  uint32_t cur = 0u;
  for (uint32_t w = PM_AB_WORDS; w-- > 0u;) {
    if (w + 1u == PM_AB_WORDS)
      hipLaunchKernelGGL(ab_gather_kernel, grid, dim3(256), 0, s, keys, (const uint32_t*)nullptr, W, w, b.key[cur], b.val[cur]);
    else
      hipLaunchKernelGGL(ab_gather_kernel, grid, dim3(256), 0, s, keys, (const uint32_t*)b.val[cur], W, w, b.key[cur], (uint32_t*)nullptr);
    cur = launch_ro_radix_sort(b, W, PM_AB_PASSES, cur, s);
  }
  return cur;
}

void launch_ab_rank(const uint32_t* val, uint32_t W, uint32_t* rank, hipStream_t s) {
  if (!W) return;
  hipLaunchKernelGGL(ab_rank_kernel, dim3((W + 255u) / 256u), dim3(256), 0, s, val, W, rank);
}

void launch_invite_digests(const uint32_t* rows, uint32_t n, const uint32_t* bytes, uint32_t domain_id, uint32_t pool_id,
                           const uint64_t* nonce, const uint64_t* expiration, uint64_t* digest, uint64_t* signing, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(invite_digest_kernel, dim3((n + 63u) / 64u), dim3(64), 0, s, rows, n, bytes, domain_id, pool_id, nonce, expiration,
                     digest, signing);
}
