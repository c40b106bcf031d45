// pm_keccak.inc — part of pm_kernels.hip (included in place, namespace pm): keccak-256 as Ethereum uses it (the original Keccak
// padding 0x01 ... 0x80, not SHA-3's 0x06; rate 136 bytes, 32 bytes out), one message a lane.
//
// The state is 25 named 64-bit values (lane x + 5 y is s<x + 5 y>): nothing is indexed, so the whole permutation stays in
// registers (50 VGPRs of state, 10 of column parities, 50 of the rotated copy at the widest point).  The 24 rounds are written
// out through a macro with the round constant and every rotation amount as literals: a 64-bit rotate by a constant is two
// v_alignbit_b32 (or a register swap and two of them), and there is no table the rounds would have to index.
struct KcState {
  uint64_t s0, s1, s2, s3, s4, s5, s6, s7, s8, s9, s10, s11, s12, s13, s14, s15, s16, s17, s18, s19, s20, s21, s22, s23, s24;
};

#define KC_ROTL(x, n) (((x) << (n)) | ((x) >> (64 - (n))))

// theta, rho and pi (B<y + 5 ((2 x + 3 y) mod 5)> = rotl(s<x + 5 y>, r[x][y])), chi, iota
#define KC_ROUND(st, rc)                                                                                                       \
  {                                                                                                                            \
    const uint64_t c0 = st.s0 ^ st.s5 ^ st.s10 ^ st.s15 ^ st.s20, c1 = st.s1 ^ st.s6 ^ st.s11 ^ st.s16 ^ st.s21,                 \
                   c2 = st.s2 ^ st.s7 ^ st.s12 ^ st.s17 ^ st.s22, c3 = st.s3 ^ st.s8 ^ st.s13 ^ st.s18 ^ st.s23,                 \
                   c4 = st.s4 ^ st.s9 ^ st.s14 ^ st.s19 ^ st.s24;                                                               \
    const uint64_t d0 = c4 ^ KC_ROTL(c1, 1), d1 = c0 ^ KC_ROTL(c2, 1), d2 = c1 ^ KC_ROTL(c3, 1), d3 = c2 ^ KC_ROTL(c4, 1),       \
                   d4 = c3 ^ KC_ROTL(c0, 1);                                                                                    \
    const uint64_t t0 = st.s0 ^ d0, t1 = st.s1 ^ d1, t2 = st.s2 ^ d2, t3 = st.s3 ^ d3, t4 = st.s4 ^ d4, t5 = st.s5 ^ d0,        \
                   t6 = st.s6 ^ d1, t7 = st.s7 ^ d2, t8 = st.s8 ^ d3, t9 = st.s9 ^ d4, t10 = st.s10 ^ d0, t11 = st.s11 ^ d1,    \
                   t12 = st.s12 ^ d2, t13 = st.s13 ^ d3, t14 = st.s14 ^ d4, t15 = st.s15 ^ d0, t16 = st.s16 ^ d1,               \
                   t17 = st.s17 ^ d2, t18 = st.s18 ^ d3, t19 = st.s19 ^ d4, t20 = st.s20 ^ d0, t21 = st.s21 ^ d1,               \
                   t22 = st.s22 ^ d2, t23 = st.s23 ^ d3, t24 = st.s24 ^ d4;                                                     \
    const uint64_t b0 = t0, b10 = KC_ROTL(t1, 1), b20 = KC_ROTL(t2, 62), b5 = KC_ROTL(t3, 28), b15 = KC_ROTL(t4, 27),            \
                   b16 = KC_ROTL(t5, 36), b1 = KC_ROTL(t6, 44), b11 = KC_ROTL(t7, 6), b21 = KC_ROTL(t8, 55),                     \
                   b6 = KC_ROTL(t9, 20), b7 = KC_ROTL(t10, 3), b17 = KC_ROTL(t11, 10), b2 = KC_ROTL(t12, 43),                    \
                   b12 = KC_ROTL(t13, 25), b22 = KC_ROTL(t14, 39), b23 = KC_ROTL(t15, 41), b8 = KC_ROTL(t16, 45),                \
                   b18 = KC_ROTL(t17, 15), b3 = KC_ROTL(t18, 21), b13 = KC_ROTL(t19, 8), b14 = KC_ROTL(t20, 18),                 \
                   b24 = KC_ROTL(t21, 2), b9 = KC_ROTL(t22, 61), b19 = KC_ROTL(t23, 56), b4 = KC_ROTL(t24, 14);                  \
    st.s0 = b0 ^ (~b1 & b2) ^ (rc);                                                                                            \
    st.s1 = b1 ^ (~b2 & b3);                                                                                                   \
    st.s2 = b2 ^ (~b3 & b4);                                                                                                   \
    st.s3 = b3 ^ (~b4 & b0);                                                                                                   \
    st.s4 = b4 ^ (~b0 & b1);                                                                                                   \
    st.s5 = b5 ^ (~b6 & b7);                                                                                                   \
    st.s6 = b6 ^ (~b7 & b8);                                                                                                   \
    st.s7 = b7 ^ (~b8 & b9);                                                                                                   \
    st.s8 = b8 ^ (~b9 & b5);                                                                                                   \
    st.s9 = b9 ^ (~b5 & b6);                                                                                                   \
    st.s10 = b10 ^ (~b11 & b12);                                                                                               \
    st.s11 = b11 ^ (~b12 & b13);                                                                                               \
    st.s12 = b12 ^ (~b13 & b14);                                                                                               \
    st.s13 = b13 ^ (~b14 & b10);                                                                                               \
    st.s14 = b14 ^ (~b10 & b11);                                                                                               \
    st.s15 = b15 ^ (~b16 & b17);                                                                                               \
    st.s16 = b16 ^ (~b17 & b18);                                                                                               \
    st.s17 = b17 ^ (~b18 & b19);                                                                                               \
    st.s18 = b18 ^ (~b19 & b15);                                                                                               \
    st.s19 = b19 ^ (~b15 & b16);                                                                                               \
    st.s20 = b20 ^ (~b21 & b22);                                                                                               \
    st.s21 = b21 ^ (~b22 & b23);                                                                                               \
    st.s22 = b22 ^ (~b23 & b24);                                                                                               \
    st.s23 = b23 ^ (~b24 & b20);                                                                                               \
    st.s24 = b24 ^ (~b20 & b21);                                                                                               \
  }

__device__ __forceinline__ void keccak_f1600(KcState& st) {
  KC_ROUND(st, 0x0000000000000001ull)
  KC_ROUND(st, 0x0000000000008082ull)
  KC_ROUND(st, 0x800000000000808Aull)
  KC_ROUND(st, 0x8000000080008000ull)
  KC_ROUND(st, 0x000000000000808Bull)
  KC_ROUND(st, 0x0000000080000001ull)
  KC_ROUND(st, 0x8000000080008081ull)
  KC_ROUND(st, 0x8000000000008009ull)
  KC_ROUND(st, 0x000000000000008Aull)
  KC_ROUND(st, 0x0000000000000088ull)
  KC_ROUND(st, 0x0000000080008009ull)
  KC_ROUND(st, 0x000000008000000Aull)
  KC_ROUND(st, 0x000000008000808Bull)
  KC_ROUND(st, 0x800000000000008Bull)
  KC_ROUND(st, 0x8000000000008089ull)
  KC_ROUND(st, 0x8000000000008003ull)
  KC_ROUND(st, 0x8000000000008002ull)
  KC_ROUND(st, 0x8000000000000080ull)
  KC_ROUND(st, 0x000000000000800Aull)
  KC_ROUND(st, 0x800000008000000Aull)
  KC_ROUND(st, 0x8000000080008081ull)
  KC_ROUND(st, 0x8000000000008080ull)
  KC_ROUND(st, 0x0000000080000001ull)
  KC_ROUND(st, 0x8000000080008008ull)
}

__device__ __forceinline__ void kc_zero(KcState& st) {
  st.s0 = st.s1 = st.s2 = st.s3 = st.s4 = st.s5 = st.s6 = st.s7 = st.s8 = st.s9 = st.s10 = st.s11 = st.s12 = 0ull;
  st.s13 = st.s14 = st.s15 = st.s16 = st.s17 = st.s18 = st.s19 = st.s20 = st.s21 = st.s22 = st.s23 = st.s24 = 0ull;
}

// one block of the rate into the state: LANE(i) is the i-th little-endian 64-bit word of the padded block, i < 17
#define KC_ABSORB(st, LANE)                                                                                                    \
  {                                                                                                                            \
    st.s0 ^= LANE(0), st.s1 ^= LANE(1), st.s2 ^= LANE(2), st.s3 ^= LANE(3), st.s4 ^= LANE(4), st.s5 ^= LANE(5);                \
    st.s6 ^= LANE(6), st.s7 ^= LANE(7), st.s8 ^= LANE(8), st.s9 ^= LANE(9), st.s10 ^= LANE(10), st.s11 ^= LANE(11);            \
    st.s12 ^= LANE(12), st.s13 ^= LANE(13), st.s14 ^= LANE(14), st.s15 ^= LANE(15), st.s16 ^= LANE(16);                        \
  }

static constexpr uint32_t PM_KC_RATE = 136;

// word `lane` of a block of the padded message, from the aligned 64-bit words that hold the block (w: the word that holds the
// block's first byte, sh: 8 x that byte's place in it).  left: message bytes from this word's first byte on (<= 0: none).  Bytes
// behind the message read 0x01 at its end — a block has a word with 0 <= left < 8 only if the message ends in it — and `last`
// ors 0x80 into the block's last byte.  Every word loaded holds a byte of the message.
__device__ __forceinline__ uint64_t kc_msg_lane(const uint64_t* __restrict__ w, uint32_t sh, uint32_t lane, int32_t left, bool last) {
  uint64_t v = 0ull;
  if (left > 0) {
    v = w[lane] >> sh;
    if (sh && (uint32_t)left * 8u + sh > 64u) v |= w[lane + 1u] << (64u - sh);
    if (left < 8) v &= (1ull << (8u * (uint32_t)left)) - 1ull;
  }
  if (left >= 0 && left < 8) v |= 0x01ull << (8u * (uint32_t)left);
  if (last && lane == 16u) v |= 0x80ull << 56;
  return v;
}

// keccak-256 of msg[0, len): the digest is the little-endian bytes of out[0..4)
__device__ __forceinline__ void keccak256_bytes(const uint8_t* __restrict__ msg, uint32_t len, uint64_t out[4]) {
  KcState st;
  kc_zero(st);
  const uint32_t blocks = len / PM_KC_RATE + 1u;  // (the padding always adds a byte)
  for (uint32_t blk = 0; blk < blocks; ++blk) {
    const bool last = blk + 1u == blocks;
    const uintptr_t p = (uintptr_t)(msg + (size_t)blk * PM_KC_RATE);
    const uint32_t sh = (uint32_t)(p & 7u) * 8u;
    const uint64_t* w = (const uint64_t*)(p - (p & 7u));
    const int32_t left = (int32_t)(len - blk * PM_KC_RATE);  // (0 .. 135 in the last block, more in front of it)
#define KC_LANE_MSG(i) kc_msg_lane(w, sh, i, left - 8 * (int32_t)(i), last)
    KC_ABSORB(st, KC_LANE_MSG)
#undef KC_LANE_MSG
    keccak_f1600(st);
  }
  out[0] = st.s0, out[1] = st.s1, out[2] = st.s2, out[3] = st.s3;
}

// one lane a message: bytes[off[i], off[i + 1]) -> out[32 i, 32 i + 32).  (The general path: a block comes in as the aligned words
// that hold it, at any alignment.  The book's own kernels build their blocks in registers.)
__global__ __launch_bounds__(64) void keccak_many_kernel(const uint8_t* __restrict__ bytes, const uint32_t* __restrict__ off, uint32_t n,
                                                         uint64_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  const uint32_t first = off[i];
  uint64_t d[4];
  keccak256_bytes(bytes + first, off[i + 1u] - first, d);
#pragma unroll
  for (uint32_t q = 0; q < 4u; ++q) out[4u * i + q] = d[q];
}

void launch_keccak_many(const uint8_t* bytes, const uint32_t* off, uint32_t n, uint64_t* out, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(keccak_many_kernel, dim3((n + 63u) / 64u), dim3(64), 0, s, bytes, off, n, out);
}
