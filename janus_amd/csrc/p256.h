// NIST P-256 for the GPU HPKE open of DHKEM(P-256, HKDF-SHA256) (KEM 0x0010), free of HIP so the
// device kernels (hpke_dh_gpu.h: k_p256_dh, k_p256_dh_idx) and a CPU test
// (tests/native/p256_host.cpp) run the same code:
//   Fp256, fp_*            GF(p), p = 2^256 - 2^224 + 2^192 + 2^96 - 1            FIPS 186-4 D.1.2.3
//   p256_decode            DeserializePublicKey with the on-curve check           RFC 9180 §7.1.1, §7.1.4
//   p256_dh_x, p256_mul_xy x([k] P) and (x, y)([k] P), one instruction sequence for every scalar,
//                          wave-uniform (the recipient's key) or the lane's own (the sender's
//                          ephemeral key, hpke_dh_gpu.h: k_p256_eph)
// The KEM half (ExtractAndExpand, RFC 9180 §4.1) and the kernels' lane are p256_kem.h's, which
// hashes; this header has no dependency, so the host planning (plan_hpke.h) validates keypairs
// with the kernels' own decoder.
//
// Field elements are eight 32-bit limbs, little-endian, in Montgomery form (x R mod p, R = 2^256)
// and ALWAYS canonical (< p): every fp_* function takes canonical inputs and returns a canonical
// output, so equality is limb equality and there is no lazy-reduction bound to track.
// Products are (uint64_t)a * b + acc + carry <= 2^64 - 1, i.e. one v_mad_u64_u32 each.  p = -1
// (mod 2^32), so the quotient digit of a word-wise Montgomery step is the low word itself
// (m = t0), and (t + m p) / 2^32 = (t >> 32) + m (2^64 + 2^160 - 2^192 + 2^224): three adds and a
// subtract of m into a signed carry chain, no products.  Inside fp_mul the accumulator t stays
// below 2 p (nine words, the ninth 0 or 1): t' = (t + a_i b + m p) / 2^32 < (2 p + 2 (2^32 - 1) p)
// / 2^32 < 2 p for b < p; one masked subtraction of p ends it.
//
// Nothing here branches or indexes memory by the scalar or by a field value: a wave-uniform
// scalar's words are picked with selects on the loop counter (as x25519_lane does), a lane's own
// scalar is shifted out of fixed registers, its bits are used as select masks only; the inversion
// is a fixed addition chain for p - 2.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define P3G_P256 __host__ __device__ inline __attribute__((always_inline))
#else
#define P3G_P256 inline
#endif

namespace p3g {

// ------------------------------------------------------------------------------------------------
// GF(p)
// ------------------------------------------------------------------------------------------------
struct Fp256 {
  uint32_t v[8];
};
struct P256Scalar {  // k in [1, n), little-endian words; a kernel argument (SGPRs)
  uint32_t w[8];
};
struct P256LaneScalar {  // the same, a lane's own (VGPRs): the sender's ephemeral key
  uint32_t w[8];
};

// p's limbs are 0xffffffff at 0, 1, 2, 7; 1 at 6; 0 at 3, 4, 5
P3G_P256 constexpr uint32_t fp_p(int i) {
  return (i <= 2 || i == 7) ? 0xffffffffu : (i == 6 ? 1u : 0u);
}

P3G_P256 void fp_set(Fp256& r, uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3, uint32_t a4,
                     uint32_t a5, uint32_t a6, uint32_t a7) {
  r.v[0] = a0; r.v[1] = a1; r.v[2] = a2; r.v[3] = a3;
  r.v[4] = a4; r.v[5] = a5; r.v[6] = a6; r.v[7] = a7;
}
P3G_P256 void fp_one(Fp256& r) {  // R mod p
  fp_set(r, 0x00000001u, 0x00000000u, 0x00000000u, 0xffffffffu, 0xffffffffu, 0xffffffffu,
         0xfffffffeu, 0x00000000u);
}
P3G_P256 void fp_r2(Fp256& r) {  // R^2 mod p
  fp_set(r, 0x00000003u, 0x00000000u, 0xffffffffu, 0xfffffffbu, 0xfffffffeu, 0xffffffffu,
         0xfffffffdu, 0x00000004u);
}
P3G_P256 void fp_curve_b(Fp256& r) {  // b R mod p
  fp_set(r, 0x29c4bddfu, 0xd89cdf62u, 0x78843090u, 0xacf005cdu, 0xf7212ed6u, 0xe5a220abu,
         0x04874834u, 0xdc30061du);
}

// r = t - p if t >= p else t, for a nine-word t < 2 p (hi = the ninth word)
P3G_P256 void fp_cond_sub_p(Fp256& r, const uint32_t t[8], uint32_t hi) {
  uint32_t d[8];
  int64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    c += (int64_t)t[i] - (int64_t)fp_p(i);
    d[i] = (uint32_t)c;
    c >>= 32;
  }
  // t >= p iff the subtraction does not borrow out of the ninth word
  const uint32_t keep = ((int64_t)hi + c < 0) ? 0xffffffffu : 0u;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = (t[i] & keep) | (d[i] & ~keep);
}

P3G_P256 void fp_add(Fp256& r, const Fp256& a, const Fp256& b) {
  uint32_t t[8];
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    c += (uint64_t)a.v[i] + b.v[i];
    t[i] = (uint32_t)c;
    c >>= 32;
  }
  fp_cond_sub_p(r, t, (uint32_t)c);
}

P3G_P256 void fp_sub(Fp256& r, const Fp256& a, const Fp256& b) {
  uint32_t d[8];
  int64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    c += (int64_t)a.v[i] - (int64_t)b.v[i];
    d[i] = (uint32_t)c;
    c >>= 32;
  }
  const uint32_t m = (uint32_t)c;  // all ones after a borrow: add p back
  uint64_t k = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    k += (uint64_t)d[i] + (fp_p(i) & m);
    r.v[i] = (uint32_t)k;
    k >>= 32;
  }
}

// r = a b / R mod p (word-wise Montgomery, see the header): 64 products.
P3G_P256 void fp_mul(Fp256& r, const Fp256& a, const Fp256& b) {
  uint32_t t[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) t[i] = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      c += (uint64_t)a.v[i] * b.v[j] + t[j];
      t[j] = (uint32_t)c;
      c >>= 32;
    }
    c += t[8];  // < 2^33
    const uint32_t m = t[0];
    // (t + m p) / 2^32: drop word 0, add m at words 2, 5, 7 and subtract it at word 6
    t[0] = t[1];
    t[1] = t[2];
    int64_t s = (int64_t)t[3] + m;
    t[2] = (uint32_t)s; s >>= 32;
    s += t[4];
    t[3] = (uint32_t)s; s >>= 32;
    s += t[5];
    t[4] = (uint32_t)s; s >>= 32;
    s += (int64_t)t[6] + m;
    t[5] = (uint32_t)s; s >>= 32;
    s += (int64_t)t[7] - (int64_t)m;
    t[6] = (uint32_t)s; s >>= 32;
    s += (int64_t)(uint32_t)c + m;
    t[7] = (uint32_t)s; s >>= 32;
    t[8] = (uint32_t)(s + (int64_t)(c >> 32));
  }
  fp_cond_sub_p(r, t, t[8]);
}

P3G_P256 void fp_sqr(Fp256& r, const Fp256& a) { fp_mul(r, a, a); }

P3G_P256 void fp_sqn(Fp256& r, const Fp256& a, int n) {
  fp_sqr(r, a);
#pragma unroll 1
  for (int i = 1; i < n; ++i) fp_sqr(r, r);
}

// a^(p - 2) (0 for a = 0), p - 2 = 2^256 - 2^224 + 2^192 + 2^96 - 3: with x_k = a^(2^k - 1),
//   ((((x32 2^32 + 1) 2^128 + x32) 2^32 + x32) 2^30 + x30) 2^2 + 1   (exponents, additively)
// 255 squarings and 12 multiplications, the same for every a.
P3G_P256 void fp_inv(Fp256& r, const Fp256& a) {
  Fp256 x2, x3, x6, x12, x15, x30, x32, t;
  fp_sqr(t, a);
  fp_mul(x2, t, a);
  fp_sqr(t, x2);
  fp_mul(x3, t, a);
  fp_sqn(t, x3, 3);
  fp_mul(x6, t, x3);
  fp_sqn(t, x6, 6);
  fp_mul(x12, t, x6);
  fp_sqn(t, x12, 3);
  fp_mul(x15, t, x3);
  fp_sqn(t, x15, 15);
  fp_mul(x30, t, x15);
  fp_sqn(t, x30, 2);
  fp_mul(x32, t, x2);
  fp_sqn(t, x32, 32);
  fp_mul(t, t, a);
  fp_sqn(t, t, 128);
  fp_mul(t, t, x32);
  fp_sqn(t, t, 32);
  fp_mul(t, t, x32);
  fp_sqn(t, t, 30);
  fp_mul(t, t, x30);
  fp_sqn(t, t, 2);
  fp_mul(r, t, a);
}

P3G_P256 void fp_to_mont(Fp256& r, const Fp256& a) {  // a < p as plain limbs
  Fp256 r2;
  fp_r2(r2);
  fp_mul(r, a, r2);
}
P3G_P256 void fp_from_mont(Fp256& r, const Fp256& a) {
  Fp256 one;
  fp_set(one, 1u, 0u, 0u, 0u, 0u, 0u, 0u, 0u);
  fp_mul(r, a, one);
}

P3G_P256 void fp_select(Fp256& r, const Fp256& a, const Fp256& b, uint32_t take_b) {  // 0 or 1
  const uint32_t m = 0u - take_b;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = a.v[i] ^ (m & (a.v[i] ^ b.v[i]));
}

// 8 big-endian words (word 0 the most significant, the form SHA-256 consumes) <-> plain limbs
P3G_P256 void fp_from_be(Fp256& r, const uint32_t be[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = be[7 - i];
}
P3G_P256 bool fp_is_canonical(const Fp256& a) {  // a < p
  int64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    c += (int64_t)a.v[i] - (int64_t)fp_p(i);
    c >>= 32;
  }
  return c < 0;
}

// ------------------------------------------------------------------------------------------------
// The curve y^2 = x^3 - 3 x + b
// ------------------------------------------------------------------------------------------------
// 32 big-endian bytes at p (any alignment) as 8 big-endian words
P3G_P256 void p256_load_be_words8(const uint8_t* p, uint32_t w[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i)
    w[i] = ((uint32_t)p[4 * i] << 24) | ((uint32_t)p[4 * i + 1] << 16) |
           ((uint32_t)p[4 * i + 2] << 8) | (uint32_t)p[4 * i + 3];
}

// (x, y) given as big-endian words -> Montgomery coordinates; true iff x < p, y < p and the point
// is on the curve (the invalid-curve attack is refused here).  On false X, Y are unspecified.
P3G_P256 bool p256_validate(const uint32_t xbe[8], const uint32_t ybe[8], Fp256& X, Fp256& Y) {
  Fp256 x, y;
  fp_from_be(x, xbe);
  fp_from_be(y, ybe);
  const bool canon = fp_is_canonical(x) & fp_is_canonical(y);
  // a non-canonical coordinate is masked to zero so that fp_mul's precondition holds; the point is
  // refused by `canon` whatever the equation says
  const uint32_t m = canon ? 0xffffffffu : 0u;
#pragma unroll
  for (int i = 0; i < 8; ++i) x.v[i] &= m, y.v[i] &= m;
  fp_to_mont(X, x);
  fp_to_mont(Y, y);
  Fp256 lhs, rhs, t, b;
  fp_curve_b(b);
  fp_sqr(lhs, Y);
  fp_sqr(t, X);
  fp_mul(rhs, t, X);
  fp_add(t, X, X);
  fp_add(t, t, X);
  fp_sub(rhs, rhs, t);
  fp_add(rhs, rhs, b);
  uint32_t diff = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) diff |= lhs.v[i] ^ rhs.v[i];
  return canon & (diff == 0u);
}

// DeserializePublicKey: 65 bytes, 0x04 || x || y.  xbe / ybe get the coordinates' words as they
// stand in the encoding (the kem_context uses them).
P3G_P256 bool p256_decode(const uint8_t* enc, uint32_t xbe[8], uint32_t ybe[8], Fp256& X,
                          Fp256& Y) {
  p256_load_be_words8(enc + 1, xbe);
  p256_load_be_words8(enc + 33, ybe);
  const bool ok = p256_validate(xbe, ybe, X, Y);
  return ok & (enc[0] == 0x04);
}

struct P256Proj {  // homogeneous projective (X : Y : Z), Montgomery coordinates; (0 : 1 : 0) = O
  Fp256 X, Y, Z;
};

// The complete formulas of Renes, Costello and Batina ("Complete addition formulas for prime order
// elliptic curves", Eurocrypt 2016) for a = -3: valid for EVERY pair of inputs on a prime-order
// curve, the point at infinity and P = Q included, so the ladder below has no exceptional case.
// Doubling (their Algorithm 6): 8 M + 3 S + 2 m_b.
P3G_P256 void p256_double(P256Proj& r, const P256Proj& p) {
  Fp256 b, t0, t1, t2, t3, X3, Y3, Z3;
  fp_curve_b(b);
  fp_sqr(t0, p.X);
  fp_sqr(t1, p.Y);
  fp_sqr(t2, p.Z);
  fp_mul(t3, p.X, p.Y);
  fp_add(t3, t3, t3);
  fp_mul(Z3, p.X, p.Z);
  fp_add(Z3, Z3, Z3);
  fp_mul(Y3, b, t2);
  fp_sub(Y3, Y3, Z3);
  fp_add(X3, Y3, Y3);
  fp_add(Y3, X3, Y3);
  fp_sub(X3, t1, Y3);
  fp_add(Y3, t1, Y3);
  fp_mul(Y3, X3, Y3);
  fp_mul(X3, X3, t3);
  fp_add(t3, t2, t2);
  fp_add(t2, t2, t3);
  fp_mul(Z3, b, Z3);
  fp_sub(Z3, Z3, t2);
  fp_sub(Z3, Z3, t0);
  fp_add(t3, Z3, Z3);
  fp_add(Z3, Z3, t3);
  fp_add(t3, t0, t0);
  fp_add(t0, t3, t0);
  fp_sub(t0, t0, t2);
  fp_mul(t0, t0, Z3);
  fp_add(Y3, Y3, t0);
  fp_mul(t0, p.Y, p.Z);
  fp_add(t0, t0, t0);
  fp_mul(Z3, t0, Z3);
  fp_sub(r.X, X3, Z3);
  fp_mul(Z3, t0, t1);
  fp_add(Z3, Z3, Z3);
  fp_add(r.Z, Z3, Z3);
  r.Y = Y3;
}

// Mixed addition r = p + (x2, y2) with an affine second point, never O (their Algorithm 5):
// 11 M + 2 m_b.
P3G_P256 void p256_add_affine(P256Proj& r, const P256Proj& p, const Fp256& x2, const Fp256& y2) {
  Fp256 b, t0, t1, t2, t3, t4, X3, Y3, Z3;
  fp_curve_b(b);
  fp_mul(t0, p.X, x2);
  fp_mul(t1, p.Y, y2);
  fp_add(t3, x2, y2);
  fp_add(t4, p.X, p.Y);
  fp_mul(t3, t3, t4);
  fp_add(t4, t0, t1);
  fp_sub(t3, t3, t4);
  fp_mul(t4, y2, p.Z);
  fp_add(t4, t4, p.Y);
  fp_mul(Y3, x2, p.Z);
  fp_add(Y3, Y3, p.X);
  fp_mul(Z3, b, p.Z);
  fp_sub(X3, Y3, Z3);
  fp_add(Z3, X3, X3);
  fp_add(X3, X3, Z3);
  fp_sub(Z3, t1, X3);
  fp_add(X3, t1, X3);
  fp_mul(Y3, b, Y3);
  fp_add(t1, p.Z, p.Z);
  fp_add(t2, t1, p.Z);
  fp_sub(Y3, Y3, t2);
  fp_sub(Y3, Y3, t0);
  fp_add(t1, Y3, Y3);
  fp_add(Y3, t1, Y3);
  fp_add(t1, t0, t0);
  fp_add(t0, t1, t0);
  fp_sub(t0, t0, t2);
  fp_mul(t1, t4, Y3);
  fp_mul(t2, t0, Y3);
  fp_mul(Y3, X3, Z3);
  fp_add(r.Y, Y3, t2);
  fp_mul(X3, t3, X3);
  fp_sub(r.X, X3, t1);
  fp_mul(Z3, t4, Z3);
  fp_mul(t1, t3, t0);
  fp_add(r.Z, Z3, t1);
}

// [k] P in projective coordinates, for k in [1, n) and P = (X, Y) a valid point: double-and-add-
// always from the point at infinity over all 256 bits, the addition's result taken with a select.
// [k] P is never O (the group has prime order n and 0 < k < n), so Z != 0 at the end.
// 256 (8 M + 3 S + 2 m_b + 11 M + 2 m_b) = 6,656 field products of 64 v_mad_u64_u32.
// Scalar is P256Scalar (wave-uniform: a kernel argument in SGPRs) or P256LaneScalar (the lane's
// own, in VGPRs); the two differ only in how bit t is read (p256_next_bit), one text of the
// formulas for both.  Either way the bit is a select mask and nothing is indexed by the scalar.
// The uniform scalar's words are picked with selects on the loop counter.
P3G_P256 uint32_t p256_next_bit(P256Scalar& k, int t) {
  const int wi = t >> 5;
  uint32_t kw = k.w[0];
#pragma unroll
  for (int i = 1; i < 8; ++i) kw = wi == i ? k.w[i] : kw;
  return (kw >> (t & 31)) & 1u;
}
// The lane's own scalar is consumed from the top: its eight words shift left by one per step, so
// every word keeps a fixed register and no word is ever chosen by an index (a choice among eight
// per-lane words is what a compiler turns into an indexed array in memory).
P3G_P256 uint32_t p256_next_bit(P256LaneScalar& k, int) {
  const uint32_t kt = k.w[7] >> 31;
#pragma unroll
  for (int i = 7; i > 0; --i) k.w[i] = (k.w[i] << 1) | (k.w[i - 1] >> 31);
  k.w[0] <<= 1;
  return kt;
}

template <class Scalar>
P3G_P256 void p256_ladder(const Scalar& k_in, const Fp256& X, const Fp256& Y, P256Proj& r) {
  P256Proj s;
  Scalar k = k_in;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.X.v[i] = r.Z.v[i] = 0u;
  fp_one(r.Y);
#pragma unroll 1
  for (int t = 255; t >= 0; --t) {
    const uint32_t kt = p256_next_bit(k, t);
    p256_double(r, r);
    p256_add_affine(s, r, X, Y);
    fp_select(r.X, r.X, s.X, kt);
    fp_select(r.Y, r.Y, s.Y, kt);
    fp_select(r.Z, r.Z, s.Z, kt);
  }
}

// x([k] P) as 8 big-endian words: the ladder, the inversion's 267 products and three more, 443 K
// products per DH.
template <class Scalar>
P3G_P256 void p256_dh_x(const Scalar& k, const Fp256& X, const Fp256& Y, uint32_t out_be[8]) {
  P256Proj r;
  p256_ladder(k, X, Y, r);
  Fp256 zi, x;
  fp_inv(zi, r.Z);
  fp_mul(x, r.X, zi);
  fp_from_mont(x, x);
#pragma unroll
  for (int i = 0; i < 8; ++i) out_be[i] = x.v[7 - i];
}

// Both affine coordinates of [k] P as 8 big-endian words each (one inversion, two products): what
// SerializePublicKey writes behind the 0x04 of an encapsulated key.
template <class Scalar>
P3G_P256 void p256_mul_xy(const Scalar& k, const Fp256& X, const Fp256& Y, uint32_t x_be[8],
                          uint32_t y_be[8]) {
  P256Proj r;
  p256_ladder(k, X, Y, r);
  Fp256 zi, x, y;
  fp_inv(zi, r.Z);
  fp_mul(x, r.X, zi);
  fp_mul(y, r.Y, zi);
  fp_from_mont(x, x);
  fp_from_mont(y, y);
#pragma unroll
  for (int i = 0; i < 8; ++i) x_be[i] = x.v[7 - i], y_be[i] = y.v[7 - i];
}

// The group order n's limbs, little-endian
P3G_P256 constexpr uint32_t p256_order(int i) {
  return i == 0 ? 0xfc632551u : i == 1 ? 0xf3b9cac2u : i == 2 ? 0xa7179e84u : i == 3 ? 0xbce6faadu
         : i == 6 ? 0u : 0xffffffffu;
}

// A lane's own scalar from 32 big-endian bytes (any alignment); true iff 1 <= k < n.  A scalar
// outside that range is replaced by 1, so the ladder's precondition holds and the lane runs the
// same instructions; its caller zeroes what such a lane computes.  No branch on the value.
P3G_P256 bool p256_lane_scalar(const uint8_t* be, P256LaneScalar& k) {
  uint32_t w[8];
  p256_load_be_words8(be, w);
  uint32_t nz = 0;
  int64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    k.w[i] = w[7 - i];
    nz |= k.w[i];
    c += (int64_t)k.w[i] - (int64_t)p256_order(i);
    c >>= 32;
  }
  const bool ok = (c < 0) & (nz != 0u);  // k - n borrows, and k is not zero
  const uint32_t m = ok ? 0xffffffffu : 0u;
#pragma unroll
  for (int i = 0; i < 8; ++i) k.w[i] = (k.w[i] & m) | (i == 0 ? (~m & 1u) : 0u);
  return ok;
}

}  // namespace p3g
