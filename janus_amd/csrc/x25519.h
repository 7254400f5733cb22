// X25519 (RFC 7748 §5) for one lane: GF(2^255 - 19) in ten unsigned limbs and the Montgomery ladder
// the DH kernels run per report (hpke_dh_gpu.h: k_x25519, k_x25519_idx and
// k_x25519_eph).  Free of HIP: the kernels and a CPU test
// (tests/native/hpke_lane_host.cpp) run the same text; DEVI is sha256.h's.
#pragma once
#include "sha256.h"

namespace p3g {

// ------------------------------------------------------------------------------------------------
// GF(2^255 - 19), ten limbs of 26 / 25 bits (value = sum v[i] 2^ceil(25.5 i)), unsigned.
// A "carried" element (output of fe_carry) has v[0], v[2..9] below 2^26 / 2^25 and v[1] below
// 2^25 + 2^18.  fe_add / fe_sub do not carry: their outputs stay below 3 * 2^26 (even limbs) and
// 3 * 2^25 (odd limbs), for which a 10-term column of fe_mul / fe_sq stays below
// 10 * 19 * 9.2 * 2^52 < 2^63 and every 32-bit premultiple (19 x, 2 x, 4 x) below 2^32.
// Products are (uint64_t)a * b + acc, i.e. one v_mad_u64_u32 each.
// ------------------------------------------------------------------------------------------------
struct Fe25 {
  uint32_t v[10];
};
struct X25519Scalar {  // clamped scalar, little-endian words; a kernel argument (SGPRs)
  uint32_t w[8];
};

DEVI void fe_carry(Fe25& h, uint64_t t[10]) {
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const int bits = (i & 1) ? 25 : 26;
    t[i] += c;
    c = t[i] >> bits;
    t[i] &= (1ull << bits) - 1;
  }
  t[0] += 19 * c;  // c < 2^39
  c = t[0] >> 26;
  t[0] &= (1ull << 26) - 1;
  t[1] += c;
#pragma unroll
  for (int i = 0; i < 10; ++i) h.v[i] = (uint32_t)t[i];
}

DEVI void fe_mul(Fe25& h, const Fe25& f, const Fe25& g) {
  uint32_t g19[10];
#pragma unroll
  for (int j = 0; j < 10; ++j) g19[j] = 19u * g.v[j];
  uint64_t t[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) t[k] = 0;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
#pragma unroll
    for (int j = 0; j < 10; ++j) {
      const int k = i + j;
      // 2^(off_i + off_j) = 2 * 2^off_(i+j) when both are odd limbs; 2^255 = 19
      const uint32_t a = ((i & 1) && (j & 1)) ? 2u * f.v[i] : f.v[i];
      const uint32_t b = k >= 10 ? g19[j] : g.v[j];
      t[k % 10] += (uint64_t)a * b;
    }
  }
  fe_carry(h, t);
}

DEVI void fe_sq(Fe25& h, const Fe25& f) {  // 55 products instead of 100
  uint32_t f19[10];
#pragma unroll
  for (int j = 0; j < 10; ++j) f19[j] = 19u * f.v[j];
  uint64_t t[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) t[k] = 0;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
#pragma unroll
    for (int j = i; j < 10; ++j) {
      const int k = i + j;
      const uint32_t m = (i < j ? 2u : 1u) * (((i & 1) && (j & 1)) ? 2u : 1u);
      const uint32_t a = m * f.v[i];
      const uint32_t b = k >= 10 ? f19[j] : f.v[j];
      t[k % 10] += (uint64_t)a * b;
    }
  }
  fe_carry(h, t);
}

DEVI void fe_mul_small(Fe25& h, const Fe25& f, uint32_t k) {  // k < 2^18
  uint64_t t[10];
#pragma unroll
  for (int i = 0; i < 10; ++i) t[i] = (uint64_t)f.v[i] * k;
  fe_carry(h, t);
}

DEVI void fe_add(Fe25& h, const Fe25& f, const Fe25& g) {  // f, g carried
#pragma unroll
  for (int i = 0; i < 10; ++i) h.v[i] = f.v[i] + g.v[i];
}

DEVI void fe_sub(Fe25& h, const Fe25& f, const Fe25& g) {  // f - g + 2p;  f, g carried
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint32_t bias = i == 0 ? 0x7FFFFDAu : ((i & 1) ? 0x3FFFFFEu : 0x7FFFFFEu);
    h.v[i] = f.v[i] + bias - g.v[i];
  }
}

DEVI void fe_cswap(Fe25& a, Fe25& b, uint32_t swap) {  // swap is wave-uniform; still a select
  const uint32_t m = 0u - swap;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint32_t t = m & (a.v[i] ^ b.v[i]);
    a.v[i] ^= t;
    b.v[i] ^= t;
  }
}

DEVI void fe_sqn(Fe25& h, const Fe25& f, int n) {
  fe_sq(h, f);
#pragma unroll 1
  for (int i = 1; i < n; ++i) fe_sq(h, h);
}

// z^(p-2): the usual addition chain (254 squarings, 11 multiplications)
DEVI void fe_invert(Fe25& out, const Fe25& z) {
  Fe25 z2, z9, z11, z_5_0, z_10_0, z_20_0, z_50_0, z_100_0, t;
  fe_sq(z2, z);
  fe_sqn(t, z2, 2);
  fe_mul(z9, t, z);
  fe_mul(z11, z9, z2);
  fe_sq(t, z11);
  fe_mul(z_5_0, t, z9);
  fe_sqn(t, z_5_0, 5);
  fe_mul(z_10_0, t, z_5_0);
  fe_sqn(t, z_10_0, 10);
  fe_mul(z_20_0, t, z_10_0);
  fe_sqn(t, z_20_0, 20);
  fe_mul(t, t, z_20_0);
  fe_sqn(t, t, 10);
  fe_mul(z_50_0, t, z_10_0);
  fe_sqn(t, z_50_0, 50);
  fe_mul(z_100_0, t, z_50_0);
  fe_sqn(t, z_100_0, 100);
  fe_mul(t, t, z_100_0);
  fe_sqn(t, t, 50);
  fe_mul(t, t, z_50_0);
  fe_sqn(t, t, 5);
  fe_mul(out, t, z11);
}

constexpr int fe_off(int i) { return (51 * i + 1) / 2; }  // 0, 26, 51, 77, ..., 230

// 32 little-endian bytes as words -> limbs; bit 255 is dropped and u >= p is accepted as it is
// (RFC 7748 §5), like the host ladders.
DEVI void fe_from_words(Fe25& h, const uint32_t w[8]) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const int off = fe_off(i), wd = off >> 5, sh = off & 31, bits = (i & 1) ? 25 : 26;
    uint32_t x = w[wd] >> sh;
    if (sh + bits > 32 && wd + 1 < 8) x |= w[wd + 1] << (32 - sh);
    h.v[i] = x & ((1u << bits) - 1);
  }
}

// carried limbs -> the canonical value (< p) as 8 little-endian words
DEVI void fe_to_words(uint32_t w[8], const Fe25& f) {
  uint32_t h[10];
#pragma unroll
  for (int i = 0; i < 10; ++i) h[i] = f.v[i];
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
      const int bits = (i & 1) ? 25 : 26;
      h[i] += c;
      c = h[i] >> bits;
      h[i] &= (1u << bits) - 1;
    }
    h[0] += 19u * c;
  }
  uint32_t q = (h[0] + 19u) >> 26;  // q = 1 iff h >= p
#pragma unroll
  for (int i = 1; i < 10; ++i) q = (h[i] + q) >> ((i & 1) ? 25 : 26);
  h[0] += 19u * q;
  uint32_t c = 0;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const int bits = (i & 1) ? 25 : 26;
    h[i] += c;
    c = h[i] >> bits;
    h[i] &= (1u << bits) - 1;  // the last carry is 2^255: dropped
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) w[k] = 0;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const int off = fe_off(i), wd = off >> 5, sh = off & 31, bits = (i & 1) ? 25 : 26;
    w[wd] |= h[i] << sh;
    if (sh + bits > 32) w[wd + 1] |= h[i] >> (32 - sh);
  }
}

// 32 bytes at p (any alignment) as little-endian words
DEVI void load_le_words8(const uint8_t* p, uint32_t w[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i)
    w[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) |
           ((uint32_t)p[4 * i + 3] << 24);
}

// w = X25519(k, w) for this lane's point (little-endian words).  The Montgomery ladder of RFC 7748
// §5; the scalar is wave-uniform, its bits are read with uniform selects and used only as swap
// masks, so no branch and no address depends on the scalar or on a field value.
DEVI void x25519_lane(const X25519Scalar& k, uint32_t w[8]) {
  Fe25 x1, x2, z2, x3, z3;
  fe_from_words(x1, w);
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    x2.v[i] = z3.v[i] = i ? 0u : 1u;
    z2.v[i] = 0u;
  }
  x3 = x1;
  uint32_t swap = 0;
#pragma unroll 1
  for (int t = 254; t >= 0; --t) {
    const int wi = t >> 5;
    uint32_t kw = k.w[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) kw = wi == i ? k.w[i] : kw;
    const uint32_t kt = (kw >> (t & 31)) & 1u;
    swap ^= kt;
    fe_cswap(x2, x3, swap);
    fe_cswap(z2, z3, swap);
    swap = kt;
    Fe25 A, AA, B, BB, E, C, D, DA, CB, t0, t1;
    fe_add(A, x2, z2);
    fe_sq(AA, A);
    fe_sub(B, x2, z2);
    fe_sq(BB, B);
    fe_sub(E, AA, BB);
    fe_add(C, x3, z3);
    fe_sub(D, x3, z3);
    fe_mul(DA, D, A);
    fe_mul(CB, C, B);
    fe_add(t0, DA, CB);
    fe_sq(x3, t0);
    fe_sub(t1, DA, CB);
    fe_sq(t1, t1);
    fe_mul(z3, x1, t1);
    fe_mul(x2, AA, BB);
    fe_mul_small(t0, E, 121665u);
    fe_add(t0, AA, t0);
    fe_mul(z2, E, t0);
  }
  fe_cswap(x2, x3, swap);
  fe_cswap(z2, z3, swap);
  Fe25 inv;
  fe_invert(inv, z2);
  fe_mul(x2, x2, inv);
  fe_to_words(w, x2);
}

}  // namespace p3g
