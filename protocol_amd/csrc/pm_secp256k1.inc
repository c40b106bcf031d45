// pm_secp256k1.inc — part of pm_kernels.hip (included in place, namespace pm, behind pm_keccak.inc, pm_rollout.inc for the key
// sort and pm_addresses.inc for the byte swap): the request gate.  Public-key
// recovery on secp256k1 one signature a lane, the EIP-191 hash of a request's text, and the join of a recovered address to the
// address book's row (include/pm_engine.h "request gate").  Everything here is public data: nothing is constant time, and lanes
// may diverge.
//
// A number is four 64-bit limbs as NAMED values (v0 the least significant): nothing is indexed, so nothing goes to scratch.
// A product is eight limbs by column (SP_MAC keeps a three-limb accumulator); mod p = 2^256 - 2^32 - 977 the high half is folded
// in times 0x1000003D1, twice, and one conditional subtraction leaves every field element fully reduced (so equality is limb
// equality); mod the group order n the high half is folded in times 2^256 - n (129 bits) until nothing is left above.
// Inverses and the square root are Fermat powers by square-and-multiply over the exponent's bits: the exponent is the same in
// every lane, so the branch is uniform, and a chain tuned to p would save a sixth of three powers that are a fifth of the work.
// A point is Jacobian (x = X / Z^2, y = Y / Z^3, Z = 0 is infinity); the ladder is one interleaved double-and-add over
// {G, R, G + R} (Shamir / Straus), its entry chosen by selects.
struct Sp256 {
  uint64_t v0, v1, v2, v3;
};
struct Sp512 {
  uint64_t t0, t1, t2, t3, t4, t5, t6, t7;
};

static constexpr uint64_t SP_PC = 0x1000003D1ull;  // 2^256 - p
static constexpr uint64_t SP_P0 = 0xFFFFFFFEFFFFFC2Full;  // p's low limb (the other three are all ones)
static constexpr uint64_t SP_N0 = 0xBFD25E8CD0364141ull, SP_N1 = 0xBAAEDCE6AF48A03Bull, SP_N2 = 0xFFFFFFFFFFFFFFFEull,
                          SP_N3 = 0xFFFFFFFFFFFFFFFFull;
static constexpr uint64_t SP_NC0 = 0x402DA1732FC9BEBFull, SP_NC1 = 0x4551231950B75FC4ull;  // 2^256 - n = 2^128 + NC1 2^64 + NC0
static constexpr uint64_t SP_GX0 = 0x59F2815B16F81798ull, SP_GX1 = 0x029BFCDB2DCE28D9ull, SP_GX2 = 0x55A06295CE870B07ull,
                          SP_GX3 = 0x79BE667EF9DCBBACull;
static constexpr uint64_t SP_GY0 = 0x9C47D08FFB10D4B8ull, SP_GY1 = 0xFD17B448A6855419ull, SP_GY2 = 0x5DA4FBFC0E1108A8ull,
                          SP_GY3 = 0x483ADA7726A3C465ull;
// 2 G, affine: the table's third entry when R = G
static constexpr uint64_t SP_G2X0 = 0xABAC09B95C709EE5ull, SP_G2X1 = 0x5C778E4B8CEF3CA7ull, SP_G2X2 = 0x3045406E95C07CD8ull,
                          SP_G2X3 = 0xC6047F9441ED7D6Dull;
static constexpr uint64_t SP_G2Y0 = 0x236431A950CFE52Aull, SP_G2Y1 = 0xF7F632653266D0E1ull, SP_G2Y2 = 0xA3C58419466CEAEEull,
                          SP_G2Y3 = 0x1AE168FEA63DC339ull;

__device__ __forceinline__ Sp256 sp_make(uint64_t a, uint64_t b, uint64_t c, uint64_t d) {
  Sp256 r;
  r.v0 = a, r.v1 = b, r.v2 = c, r.v3 = d;
  return r;
}
__device__ __forceinline__ bool sp_is_zero(const Sp256& a) { return (a.v0 | a.v1 | a.v2 | a.v3) == 0ull; }
__device__ __forceinline__ bool sp_eq(const Sp256& a, const Sp256& b) {
  return ((a.v0 ^ b.v0) | (a.v1 ^ b.v1) | (a.v2 ^ b.v2) | (a.v3 ^ b.v3)) == 0ull;
}
__device__ __forceinline__ Sp256 sp_select(bool c, const Sp256& a, const Sp256& b) {
  return sp_make(c ? a.v0 : b.v0, c ? a.v1 : b.v1, c ? a.v2 : b.v2, c ? a.v3 : b.v3);
}
// a + b + carry, a - b - borrow: one limb, the carry (0 or 1) in and out
__device__ __forceinline__ uint64_t sp_adc(uint64_t a, uint64_t b, uint64_t& carry) {
  const uint64_t s = a + b, t = s + carry;
  carry = (uint64_t)(s < a) | (uint64_t)(t < s);
  return t;
}
__device__ __forceinline__ uint64_t sp_sbb(uint64_t a, uint64_t b, uint64_t& borrow) {
  const uint64_t d = a - b, t = d - borrow;
  borrow = (uint64_t)(a < b) | (uint64_t)(d < borrow);
  return t;
}
__device__ __forceinline__ uint64_t sp_add(Sp256& r, const Sp256& a, const Sp256& b) {
  uint64_t c = 0ull;
  r.v0 = sp_adc(a.v0, b.v0, c), r.v1 = sp_adc(a.v1, b.v1, c), r.v2 = sp_adc(a.v2, b.v2, c), r.v3 = sp_adc(a.v3, b.v3, c);
  return c;
}
__device__ __forceinline__ uint64_t sp_sub(Sp256& r, const Sp256& a, const Sp256& b) {
  uint64_t c = 0ull;
  r.v0 = sp_sbb(a.v0, b.v0, c), r.v1 = sp_sbb(a.v1, b.v1, c), r.v2 = sp_sbb(a.v2, b.v2, c), r.v3 = sp_sbb(a.v3, b.v3, c);
  return c;
}
// a < b
__device__ __forceinline__ bool sp_less(const Sp256& a, const Sp256& b) {
  Sp256 d;
  return sp_sub(d, a, b) != 0ull;
}

// (cy, hi, lo) += x y
#define SP_MAC(x, y)                                         \
  {                                                          \
    const uint64_t pl_ = (x) * (y), ph_ = __umul64hi(x, y);  \
    lo += pl_;                                               \
    const uint64_t ph2_ = ph_ + (uint64_t)(lo < pl_);        \
    hi += ph2_;                                              \
    cy += (uint64_t)(hi < ph2_);                             \
  }
#define SP_COLUMN(out) out = lo, lo = hi, hi = cy, cy = 0ull;

__device__ __forceinline__ void sp_mul_wide(const Sp256& a, const Sp256& b, Sp512& t) {
  uint64_t lo = 0ull, hi = 0ull, cy = 0ull;
  SP_MAC(a.v0, b.v0)
  SP_COLUMN(t.t0)
  SP_MAC(a.v0, b.v1)
  SP_MAC(a.v1, b.v0)
  SP_COLUMN(t.t1)
  SP_MAC(a.v0, b.v2)
  SP_MAC(a.v1, b.v1)
  SP_MAC(a.v2, b.v0)
  SP_COLUMN(t.t2)
  SP_MAC(a.v0, b.v3)
  SP_MAC(a.v1, b.v2)
  SP_MAC(a.v2, b.v1)
  SP_MAC(a.v3, b.v0)
  SP_COLUMN(t.t3)
  SP_MAC(a.v1, b.v3)
  SP_MAC(a.v2, b.v2)
  SP_MAC(a.v3, b.v1)
  SP_COLUMN(t.t4)
  SP_MAC(a.v2, b.v3)
  SP_MAC(a.v3, b.v2)
  SP_COLUMN(t.t5)
  SP_MAC(a.v3, b.v3)
  t.t6 = lo, t.t7 = hi;
}

// ---- the field: mod p
__device__ __forceinline__ bool fp_at_least_p(const Sp256& a) { return (a.v1 & a.v2 & a.v3) == ~0ull && a.v0 >= SP_P0; }
__device__ __forceinline__ Sp256 fp_add(const Sp256& a, const Sp256& b) {
  Sp256 s;
  const uint64_t c = sp_add(s, a, b);
  if (c || fp_at_least_p(s)) sp_add(s, s, sp_make(SP_PC, 0ull, 0ull, 0ull));  // (- p = + (2^256 - p) mod 2^256)
  return s;
}
__device__ __forceinline__ Sp256 fp_sub(const Sp256& a, const Sp256& b) {
  Sp256 d;
  if (sp_sub(d, a, b)) sp_sub(d, d, sp_make(SP_PC, 0ull, 0ull, 0ull));
  return d;
}
__device__ __forceinline__ Sp256 fp_dbl(const Sp256& a) { return fp_add(a, a); }
// lo + hi (2^256 - p), hi one limb: the limb and the carry out
__device__ __forceinline__ uint64_t fp_fold_limb(uint64_t lo, uint64_t hi, uint64_t& carry) {
  const uint64_t pl = hi * SP_PC, ph = __umul64hi(hi, SP_PC);
  const uint64_t s = lo + pl, t = s + carry;
  carry = ph + (uint64_t)(s < pl) + (uint64_t)(t < s);  // (ph < 2^33)
  return t;
}
__device__ __forceinline__ Sp256 fp_reduce(const Sp512& t) {
  uint64_t c = 0ull;
  Sp256 r;
  r.v0 = fp_fold_limb(t.t0, t.t4, c), r.v1 = fp_fold_limb(t.t1, t.t5, c), r.v2 = fp_fold_limb(t.t2, t.t6, c),
  r.v3 = fp_fold_limb(t.t3, t.t7, c);
  // c < 2^34 is the fifth limb: once more (c (2^256 - p) < 2^67)
  uint64_t c2 = 0ull;
  r.v0 = fp_fold_limb(r.v0, c, c2);
  uint64_t k = 0ull;
  r.v1 = sp_adc(r.v1, c2, k), r.v2 = sp_adc(r.v2, 0ull, k), r.v3 = sp_adc(r.v3, 0ull, k);
  // a carry out here leaves a value below 2^67: adding 2^256 - p once more cannot carry again
  if (k) sp_add(r, r, sp_make(SP_PC, 0ull, 0ull, 0ull));
  if (fp_at_least_p(r)) sp_add(r, r, sp_make(SP_PC, 0ull, 0ull, 0ull));
  return r;
}
__device__ __forceinline__ Sp256 fp_mul(const Sp256& a, const Sp256& b) {
  Sp512 t;
  sp_mul_wide(a, b, t);
  return fp_reduce(t);
}
// a^e, e = (e3, e2, e1, e0) the same in every lane
__device__ __forceinline__ Sp256 fp_pow(const Sp256& a, uint64_t e0, uint64_t e1, uint64_t e2, uint64_t e3) {
  Sp256 r = sp_make(1ull, 0ull, 0ull, 0ull);
#pragma unroll 1
  for (int32_t i = 255; i >= 0; --i) {
    r = fp_mul(r, r);
    const uint64_t w = i >= 192 ? e3 : (i >= 128 ? e2 : (i >= 64 ? e1 : e0));
    if ((w >> (i & 63)) & 1ull) r = fp_mul(r, a);
  }
  return r;
}
// which: 0 = a^(p - 2), the inverse; 1 = a^((p + 1) / 4), the square root if there is one.  One loop for both, so that the
// code of a power is there once.
__device__ __forceinline__ Sp256 fp_pow_inv_or_sqrt(const Sp256& a, bool root) {
  return fp_pow(a, root ? 0xFFFFFFFFBFFFFF0Cull : 0xFFFFFFFEFFFFFC2Dull, ~0ull, ~0ull, root ? 0x3FFFFFFFFFFFFFFFull : ~0ull);
}

// ---- the scalars: mod n
__device__ __forceinline__ Sp256 fn_order() { return sp_make(SP_N0, SP_N1, SP_N2, SP_N3); }
// t mod n
__device__ __forceinline__ Sp256 fn_reduce(const Sp512& t) {
  const Sp256 c = sp_make(SP_NC0, SP_NC1, 1ull, 0ull);
  // the high half (256 bits) times c: below 2^385
  Sp512 f;
  sp_mul_wide(sp_make(t.t4, t.t5, t.t6, t.t7), c, f);
  uint64_t k = 0ull;
  f.t0 = sp_adc(f.t0, t.t0, k), f.t1 = sp_adc(f.t1, t.t1, k), f.t2 = sp_adc(f.t2, t.t2, k), f.t3 = sp_adc(f.t3, t.t3, k);
  f.t4 = sp_adc(f.t4, 0ull, k), f.t5 = sp_adc(f.t5, 0ull, k), f.t6 = sp_adc(f.t6, 0ull, k);
  // its high part (below 2^130) times c: below 2^259
  Sp512 g;
  sp_mul_wide(sp_make(f.t4, f.t5, f.t6, 0ull), c, g);
  k = 0ull;
  g.t0 = sp_adc(g.t0, f.t0, k), g.t1 = sp_adc(g.t1, f.t1, k), g.t2 = sp_adc(g.t2, f.t2, k), g.t3 = sp_adc(g.t3, f.t3, k);
  g.t4 += k;  // (below 16)
  // one limb times c, twice: the first may carry out of 2^256 once more, the second cannot
  Sp256 r = sp_make(g.t0, g.t1, g.t2, g.t3);
  uint64_t h = g.t4;
#pragma unroll
  for (uint32_t round = 0; round < 2u; ++round) {
    const uint64_t a0 = h * SP_NC0, a1 = __umul64hi(h, SP_NC0), b1 = h * SP_NC1, b2 = __umul64hi(h, SP_NC1);
    uint64_t m = 0ull;  // h c = m 2^192 + (b2 + h + carry) 2^128 + (a1 + b1) 2^64 + a0
    const uint64_t w1 = sp_adc(a1, b1, m);
    const uint64_t w2 = sp_adc(b2, h, m);
    k = 0ull;
    r.v0 = sp_adc(r.v0, a0, k), r.v1 = sp_adc(r.v1, w1, k), r.v2 = sp_adc(r.v2, w2, k), r.v3 = sp_adc(r.v3, m, k);
    h = k;
  }
  if (!sp_less(r, fn_order())) sp_sub(r, r, fn_order());
  return r;
}
__device__ __forceinline__ Sp256 fn_mul(const Sp256& a, const Sp256& b) {
  Sp512 t;
  sp_mul_wide(a, b, t);
  return fn_reduce(t);
}
// a^(n - 2): the inverse
__device__ __forceinline__ Sp256 fn_inv(const Sp256& a) {
  Sp256 r = sp_make(1ull, 0ull, 0ull, 0ull);
#pragma unroll 1
  for (int32_t i = 255; i >= 0; --i) {
    r = fn_mul(r, r);
    const uint64_t w = i >= 192 ? SP_N3 : (i >= 128 ? SP_N2 : (i >= 64 ? SP_N1 : SP_N0 - 2ull));
    if ((w >> (i & 63)) & 1ull) r = fn_mul(r, a);
  }
  return r;
}

// ---- points
struct SpJac {
  Sp256 x, y, z;
};
// 2 P (a = 0: dbl-2009-l).  Infinity stays infinity (Z3 = 2 Y Z = 0); the curve has no point with y = 0.
__device__ __forceinline__ SpJac sp_double(const SpJac& p) {
  const Sp256 a = fp_mul(p.x, p.x), b = fp_mul(p.y, p.y), c = fp_mul(b, b);
  Sp256 d = fp_add(p.x, b);
  d = fp_dbl(fp_sub(fp_sub(fp_mul(d, d), a), c));
  const Sp256 e = fp_add(fp_dbl(a), a), f = fp_mul(e, e);
  SpJac r;
  r.x = fp_sub(f, fp_dbl(d));
  r.y = fp_sub(fp_mul(e, fp_sub(d, r.x)), fp_dbl(fp_dbl(fp_dbl(c))));
  r.z = fp_dbl(fp_mul(p.y, p.z));
  return r;
}

__device__ __forceinline__ uint64_t sp_be64(const uint8_t* __restrict__ p) {
  uint64_t v = 0ull;
#pragma unroll
  for (uint32_t j = 0; j < 8u; ++j) v = (v << 8) | (uint64_t)p[j];
  return v;
}

// one lane a signature.  hash: 32 big-endian bytes an entry, as four aligned words; sig: 65 bytes an entry (r | s | v).
// ok[i] = 1 with addr[5 i ..) the address's bytes as five words and pub[8 i ..) (null: not wanted) Qx | Qy as the words that hold
// their 64 big-endian bytes, or ok[i] = 0 with zeros.
__global__ __launch_bounds__(64) void ecrecover_kernel(const uint64_t* __restrict__ hash, const uint8_t* __restrict__ sig, uint32_t n,
                                                       uint32_t* __restrict__ addr, uint64_t* __restrict__ pub, uint8_t* __restrict__ ok) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  const uint8_t* sg = sig + (size_t)i * 65u;
  const uint32_t v = sg[64];
  const Sp256 r = sp_make(sp_be64(sg + 24), sp_be64(sg + 16), sp_be64(sg + 8), sp_be64(sg));
  const Sp256 s = sp_make(sp_be64(sg + 56), sp_be64(sg + 48), sp_be64(sg + 40), sp_be64(sg + 32));
  bool good = (v == 0u || v == 1u || v == 27u || v == 28u) && !sp_is_zero(r) && !sp_is_zero(s) && sp_less(r, fn_order()) &&
              sp_less(s, fn_order());
  const uint64_t parity = (v == 1u || v == 28u) ? 1ull : 0ull;  // (0, 27: even; 1, 28: odd)
  // R: x = r itself (r < n < p: a field element; never r + n), y = a square root of x^3 + 7 with the asked parity
  Sp256 ry = sp_make(0ull, 0ull, 0ull, 0ull);
  if (good) {
    const Sp256 rhs = fp_add(fp_mul(fp_mul(r, r), r), sp_make(7ull, 0ull, 0ull, 0ull));
    ry = fp_pow_inv_or_sqrt(rhs, true);
    good = sp_eq(fp_mul(ry, ry), rhs);
    if ((ry.v0 & 1ull) != parity) ry = fp_sub(sp_make(0ull, 0ull, 0ull, 0ull), ry);
  }
  Sp256 qx = sp_make(0ull, 0ull, 0ull, 0ull), qy = qx;
  if (good) {
    // u1 = -z / r, u2 = s / r (mod n); z = the hash mod n (below 2^256 < 2 n: one subtraction)
    Sp256 z = sp_make(ab_bswap64(hash[4u * (size_t)i + 3u]), ab_bswap64(hash[4u * (size_t)i + 2u]), ab_bswap64(hash[4u * (size_t)i + 1u]),
                      ab_bswap64(hash[4u * (size_t)i]));
    if (!sp_less(z, fn_order())) sp_sub(z, z, fn_order());
    if (!sp_is_zero(z)) sp_sub(z, fn_order(), z);  // (- z)
    const Sp256 ri = fn_inv(r);
    const Sp256 u1 = fn_mul(z, ri), u2 = fn_mul(s, ri);
    const Sp256 gx = sp_make(SP_GX0, SP_GX1, SP_GX2, SP_GX3), gy = sp_make(SP_GY0, SP_GY1, SP_GY2, SP_GY3);
    // the third entry, G + R, affine: by the chord; 2 G when R = G; infinity when R = -G
    Sp256 tx, ty;
    bool t_inf = false;
    if (sp_eq(r, gx)) {
      t_inf = !sp_eq(ry, gy);
      tx = sp_make(SP_G2X0, SP_G2X1, SP_G2X2, SP_G2X3), ty = sp_make(SP_G2Y0, SP_G2Y1, SP_G2Y2, SP_G2Y3);
    } else {
      const Sp256 lam = fp_mul(fp_sub(ry, gy), fp_pow_inv_or_sqrt(fp_sub(r, gx), false));
      tx = fp_sub(fp_sub(fp_mul(lam, lam), gx), r);
      ty = fp_sub(fp_mul(lam, fp_sub(gx, tx)), gy);
    }
    // the ladder.  One doubling site: an addition that meets its own operand (equal points) asks for the doubling of the next
    // turn and does not move to the next bit.
    SpJac acc;
    acc.x = sp_make(1ull, 0ull, 0ull, 0ull), acc.y = acc.x, acc.z = sp_make(0ull, 0ull, 0ull, 0ull);
    int32_t bit = 255;
    bool again = false;
#pragma unroll 1
    while (bit >= 0) {
      acc = sp_double(acc);
      if (again) {
        again = false;
        --bit;
        continue;
      }
      const uint64_t w1 = bit >= 192 ? u1.v3 : (bit >= 128 ? u1.v2 : (bit >= 64 ? u1.v1 : u1.v0));
      const uint64_t w2 = bit >= 192 ? u2.v3 : (bit >= 128 ? u2.v2 : (bit >= 64 ? u2.v1 : u2.v0));
      const uint32_t sel = (uint32_t)((w1 >> (bit & 63)) & 1ull) | ((uint32_t)((w2 >> (bit & 63)) & 1ull) << 1);
      if (sel != 0u && !(sel == 3u && t_inf)) {
        const Sp256 ax = sp_select(sel == 1u, gx, sp_select(sel == 2u, r, tx));
        const Sp256 ay = sp_select(sel == 1u, gy, sp_select(sel == 2u, ry, ty));
        if (sp_is_zero(acc.z)) {  // infinity + T
          acc.x = ax, acc.y = ay, acc.z = sp_make(1ull, 0ull, 0ull, 0ull);
        } else {
          const Sp256 zz = fp_mul(acc.z, acc.z), u = fp_mul(ax, zz), t = fp_mul(ay, fp_mul(acc.z, zz));
          const Sp256 h = fp_sub(u, acc.x), rr = fp_sub(t, acc.y);
          if (sp_is_zero(h)) {
            if (sp_is_zero(rr)) {  // T + T: acc is T; the next turn doubles it
              again = true;
              continue;
            }
            acc.z = sp_make(0ull, 0ull, 0ull, 0ull);  // T + (-T)
          } else {
            const Sp256 hh = fp_mul(h, h), hhh = fp_mul(h, hh), vv = fp_mul(acc.x, hh);
            const Sp256 x3 = fp_sub(fp_sub(fp_mul(rr, rr), hhh), fp_dbl(vv));
            acc.y = fp_sub(fp_mul(rr, fp_sub(vv, x3)), fp_mul(acc.y, hhh));
            acc.x = x3;
            acc.z = fp_mul(acc.z, h);
          }
        }
      }
      --bit;
    }
    good = !sp_is_zero(acc.z);  // Q = infinity is no key
    if (good) {
      const Sp256 zi = fp_pow_inv_or_sqrt(acc.z, false), zi2 = fp_mul(zi, zi);
      qx = fp_mul(acc.x, zi2);
      qy = fp_mul(acc.y, fp_mul(zi, zi2));
    }
  }
  uint32_t a0 = 0u, a1 = 0u, a2 = 0u, a3 = 0u, a4 = 0u;
  const uint64_t p0 = ab_bswap64(qx.v3), p1 = ab_bswap64(qx.v2), p2 = ab_bswap64(qx.v1), p3 = ab_bswap64(qx.v0), p4 = ab_bswap64(qy.v3),
                 p5 = ab_bswap64(qy.v2), p6 = ab_bswap64(qy.v1), p7 = ab_bswap64(qy.v0);
  if (good) {
    KcState st;
    kc_zero(st);
    st.s0 = p0, st.s1 = p1, st.s2 = p2, st.s3 = p3, st.s4 = p4, st.s5 = p5, st.s6 = p6, st.s7 = p7;
    st.s8 = 0x01ull;         // (byte 64: the padding's first byte)
    st.s16 = 0x80ull << 56;  // (byte 135: its last)
    keccak_f1600(st);
    // digest bytes 12 .. 31
    a0 = (uint32_t)(st.s1 >> 32), a1 = (uint32_t)st.s2, a2 = (uint32_t)(st.s2 >> 32), a3 = (uint32_t)st.s3, a4 = (uint32_t)(st.s3 >> 32);
  }
  addr[5u * (size_t)i] = a0, addr[5u * (size_t)i + 1u] = a1, addr[5u * (size_t)i + 2u] = a2, addr[5u * (size_t)i + 3u] = a3,
  addr[5u * (size_t)i + 4u] = a4;
  if (pub) {
    uint64_t* o = pub + 8u * (size_t)i;
    o[0] = p0, o[1] = p1, o[2] = p2, o[3] = p3, o[4] = p4, o[5] = p5, o[6] = p6, o[7] = p7;
  }
  ok[i] = good ? 1u : 0u;
}

// ---- the EIP-191 hash: keccak-256("\x19Ethereum Signed Message:\n" | decimal(len) | msg).  The prefix (26 bytes and up to ten
// digits: five words) is built in registers; the message comes in as the aligned words that hold it, as in keccak256_bytes.
// Word `lane` of the FIRST block.  pre: the prefix word of this lane (lanes 0 .. 4; 0 behind the prefix), P: the prefix's
// length.  (w, sh): the aligned words and the shift of the block's first byte, were the message to begin P bytes in front of
// itself; (w0, sh0): those of the message's own first byte.
__device__ __forceinline__ uint64_t e191_first_lane(uint32_t lane, uint64_t pre, uint32_t P, const uint64_t* __restrict__ w, uint32_t sh,
                                                    const uint64_t* __restrict__ w0, uint32_t sh0, uint32_t len, bool last) {
  const uint32_t q = 8u * lane;
  if (q + 8u <= P) return pre;  // (the prefix alone; P < 40 = 8 x 5 <= 8 x 16: never the block's last word)
  if (q < P) {                  // the prefix ends in this word: k of its bytes, then the message's first 8 - k (and its end)
    const uint32_t k = P - q;
    return pre | (kc_msg_lane(w0, sh0, 0u, (int32_t)len, false) << (8u * k));
  }
  return kc_msg_lane(w, sh, lane, (int32_t)(len + P) - (int32_t)q, last);
}

__global__ __launch_bounds__(64) void eip191_many_kernel(const uint8_t* __restrict__ bytes, const uint32_t* __restrict__ off, uint32_t n,
                                                         uint64_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  const uint32_t first = off[i], len = off[i + 1u] - first;
  // the digits, the most significant in the lowest byte
  uint64_t dlo = 0ull, dhi = 0ull;
  uint32_t nd = 0u, t = len;
  do {
    dhi = (dhi << 8) | (dlo >> 56);
    dlo = (dlo << 8) | (uint64_t)(0x30u + t % 10u);
    t /= 10u;
    ++nd;
  } while (t);
  const uint32_t P = 26u + nd;
  const uint64_t pre0 = 0x7565726568744519ull;  // 19 'E' 't' 'h' 'e' 'r' 'e' 'u'
  const uint64_t pre1 = 0x64656E676953206Dull;  // 'm' ' ' 'S' 'i' 'g' 'n' 'e' 'd'
  const uint64_t pre2 = 0x6567617373654D20ull;  // ' ' 'M' 'e' 's' 's' 'a' 'g' 'e'
  const uint64_t pre3 = 0x0A3Aull | (dlo << 16);  // ':' '\n', six digits
  const uint64_t pre4 = (dlo >> 48) | (dhi << 16);  // four more
  const uint8_t* msg = bytes + first;
  const uintptr_t m0 = (uintptr_t)msg;
  const uint64_t* w0 = (const uint64_t*)(m0 - (m0 & 7u));
  const uint32_t sh0 = (uint32_t)(m0 & 7u) * 8u;
  const uint32_t total = P + len;  // (len < 2^32 - 64: the caller's bound)
  const uint32_t blocks = total / PM_KC_RATE + 1u;
  KcState st;
  kc_zero(st);
  for (uint32_t blk = 0; blk < blocks; ++blk) {
    const bool last = blk + 1u == blocks;
    const uintptr_t p = m0 - P + (size_t)blk * PM_KC_RATE;  // (an address: nothing is read in front of the message)
    const uint32_t sh = (uint32_t)(p & 7u) * 8u;
    const uint64_t* w = (const uint64_t*)(p - (p & 7u));
    if (blk == 0u) {
#define E191_PRE(i) ((i) == 0 ? pre0 : (i) == 1 ? pre1 : (i) == 2 ? pre2 : (i) == 3 ? pre3 : (i) == 4 ? pre4 : 0ull)
#define E191_LANE0(i) e191_first_lane(i, E191_PRE(i), P, w, sh, w0, sh0, len, last)
      KC_ABSORB(st, E191_LANE0)
#undef E191_LANE0
#undef E191_PRE
    } else {
      const int32_t left = (int32_t)(total - blk * PM_KC_RATE);
#define E191_LANE(i) kc_msg_lane(w, sh, i, left - 8 * (int32_t)(i), last)
      KC_ABSORB(st, E191_LANE)
#undef E191_LANE
    }
    keccak_f1600(st);
  }
  out[4u * (size_t)i] = st.s0, out[4u * (size_t)i + 1u] = st.s1, out[4u * (size_t)i + 2u] = st.s2, out[4u * (size_t)i + 3u] = st.s3;
}

// ---- the join: the book's rows sorted by their 20 bytes (as big-endian numbers: three words, least significant first for the
// radix sort), rows without an address behind every row with one
__device__ __forceinline__ uint32_t gate_bswap32(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xFF00u) | ((v << 8) & 0xFF0000u) | (v << 24); }

// key_out[i] = word `word` of row val[i] (val null: row i): 0 = bytes 12 .. 19, 1 = bytes 4 .. 11, 2 = bytes 0 .. 3 under the
// "holds no address" bit; val_out[i] = the row when asked
__global__ __launch_bounds__(256) void gate_key_kernel(const uint32_t* __restrict__ bytes, const uint8_t* __restrict__ set,
                                                       const uint32_t* __restrict__ val, uint32_t W, uint32_t word,
                                                       uint64_t* __restrict__ key_out, uint32_t* __restrict__ val_out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= W) return;
  const uint32_t row = val ? val[i] : i;
  uint64_t k = 0ull;
  if (row < W) {
    const uint32_t* a = bytes + 5u * (size_t)row;
    if (word == 0u)
      k = ((uint64_t)gate_bswap32(a[3]) << 32) | gate_bswap32(a[4]);
    else if (word == 1u)
      k = ((uint64_t)gate_bswap32(a[1]) << 32) | gate_bswap32(a[2]);
    else
      k = set[row] ? (uint64_t)gate_bswap32(a[0]) : 1ull << 32;
  }
  key_out[i] = k;
  if (val_out) val_out[i] = row;
}

// one lane a request: the code by the middleware's precedence, the row by a lower-bound search of the index (the first of equal
// addresses is the lowest row: the sort is stable), the census by ballots
__global__ __launch_bounds__(256) void gate_verdict_kernel(const uint32_t* __restrict__ addr, const uint8_t* __restrict__ ok,
                                                           const uint8_t* __restrict__ sig, const uint32_t* __restrict__ claimed,
                                                           const uint8_t* __restrict__ flags, uint32_t n, const uint32_t* __restrict__ idx,
                                                           uint32_t n_idx, const uint32_t* __restrict__ book,
                                                           const uint8_t* __restrict__ status, uint32_t* __restrict__ out,
                                                           uint32_t* __restrict__ counts) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
  const bool live = i < n;
  uint32_t code = PM_RQ_N_CODES;
  if (live) {
    const uint32_t v = sig[(size_t)i * 65u + 64u];
    uint32_t a[5], b[5];
#pragma unroll
    for (uint32_t q = 0; q < 5u; ++q) a[q] = addr[5u * (size_t)i + q], b[q] = gate_bswap32(a[q]);
    uint32_t row = 0xFFFFFFFFu, st = 0xFFu;
    if (!(v == 0u || v == 1u || v == 27u || v == 28u)) {
      code = PM_RQ_BAD_SIGNATURE;
    } else if (!ok[i]) {
      code = PM_RQ_NO_KEY;
    } else if (flags && (flags[i] & PM_RQ_FLAG_BAD_ADDRESS)) {
      code = PM_RQ_BAD_ADDRESS;
    } else {
      bool same = true;
#pragma unroll
      for (uint32_t q = 0; q < 5u; ++q) same = same && claimed[5u * (size_t)i + q] == a[q];
      uint32_t lo = 0u, hi = n_idx;
      while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const uint32_t* r = book + 5u * (size_t)idx[mid];
        bool less = false, decided = false;  // the row's address < the recovered one
#pragma unroll
        for (uint32_t q = 0; q < 5u; ++q) {
          const uint32_t x = gate_bswap32(r[q]);
          if (!decided && x != b[q]) less = x < b[q], decided = true;
        }
        if (less)
          lo = mid + 1u;
        else
          hi = mid;
      }
      if (lo < n_idx) {
        const uint32_t cand = idx[lo];
        const uint32_t* r = book + 5u * (size_t)cand;
        bool eq = true;
#pragma unroll
        for (uint32_t q = 0; q < 5u; ++q) eq = eq && r[q] == a[q];
        if (eq) row = cand;
      }
      if (row != 0xFFFFFFFFu && status) st = status[row];
      if (!same)
        code = PM_RQ_MISMATCH;
      else if (row == 0xFFFFFFFFu)
        code = PM_RQ_UNKNOWN;
      else if (st == PM_NS_EJECTED)
        code = PM_RQ_EJECTED;
      else if (st == PM_NS_BANNED)
        code = PM_RQ_BANNED;
      else
        code = PM_RQ_OK;
    }
    uint32_t* o = out + 8u * (size_t)i;
    o[0] = code, o[1] = row, o[2] = st;
#pragma unroll
    for (uint32_t q = 0; q < 5u; ++q) o[3u + q] = a[q];
  }
#pragma unroll
  for (uint32_t c = 0; c < (uint32_t)PM_RQ_N_CODES; ++c) {
    const uint64_t m = __ballot(code == c);
    if (lane == 0u && m) atomicAdd(counts + c, (uint32_t)__popcll(m));
  }
}

void launch_ecrecover(const uint64_t* hash, const uint8_t* sig, uint32_t n, uint32_t* addr, uint64_t* pub, uint8_t* ok, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(ecrecover_kernel, dim3((n + 63u) / 64u), dim3(64), 0, s, hash, sig, n, addr, pub, ok);
}

void launch_eip191_many(const uint8_t* bytes, const uint32_t* off, uint32_t n, uint64_t* out, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(eip191_many_kernel, dim3((n + 63u) / 64u), dim3(64), 0, s, bytes, off, n, out);
}

uint32_t launch_gate_index(const uint32_t* bytes, const uint8_t* set, uint32_t W, const RoSortBufs& b, hipStream_t s) {
  if (!W) return 0u;
  const dim3 grid((W + 255u) / 256u);
  hipLaunchKernelGGL(gate_key_kernel, grid, dim3(256), 0, s, bytes, set, (const uint32_t*)nullptr, W, 0u, b.key[0], b.val[0]);
  uint32_t cur = launch_ro_radix_sort(b, W, 8u, 0u, s);
  hipLaunchKernelGGL(gate_key_kernel, grid, dim3(256), 0, s, bytes, set, (const uint32_t*)b.val[cur], W, 1u, b.key[cur], (uint32_t*)nullptr);
  cur = launch_ro_radix_sort(b, W, 8u, cur, s);
  hipLaunchKernelGGL(gate_key_kernel, grid, dim3(256), 0, s, bytes, set, (const uint32_t*)b.val[cur], W, 2u, b.key[cur], (uint32_t*)nullptr);
  return launch_ro_radix_sort(b, W, 5u, cur, s);
}

void launch_gate_verdict(const uint32_t* addr, const uint8_t* ok, const uint8_t* sig, const uint32_t* claimed, const uint8_t* flags,
                         uint32_t n, const uint32_t* idx, uint32_t n_idx, const uint32_t* book, const uint8_t* status, uint32_t* out,
                         uint32_t* counts, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(gate_verdict_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, addr, ok, sig, claimed, flags, n, idx, n_idx, book,
                     status, out, counts);
}
