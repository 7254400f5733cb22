// The fold at the end of k_accum_spec (prio3_kernels.h): two 64-bit word sums with their carry
// counts -> one canonical Field128 element.  No HIP in it: the kernel and, for
// tests/test_accum_fold.py, the host build the same source (g++, tests/native/accum_fold_host.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define P3G_FOLD_HD __host__ __device__ __forceinline__
#else
#define P3G_FOLD_HD inline
#endif

namespace accum_fold {

typedef unsigned __int128 u128;

// alo + 2^64 (ahi + blo) + 2^128 bhi  mod p,  p = 2^128 - 28 2^64 + 1 (2^128 = 28 2^64 - 1 mod p):
// (alo, ahi) is the column sum of an element's low words, (blo, bhi) that of its high words.
//
// Domain: any alo, ahi, blo; bhi < 2^59.  With x2 = bhi + carry(ahi + blo) <= 2^59 the steps
// need 28 x2 + 28 <= 2^64: k << 64 fits 128 bits, and after a wrap past 2^128 the wrapped sum is
// below k 2^64, so the + 28 2^64 - 1 correction cannot wrap again and leaves t >= 28 2^64 - 1
// > x2.  t < 2^128 < 2 p on every path, so the loop subtracts p at most once.  k_accum_spec's
// ahi, bhi are carry counts of at most 2,048 rows per chunk (32 waves x 64): below 2^32, far
// inside.
P3G_FOLD_HD u128 fold128(uint64_t alo, uint64_t ahi, uint64_t blo, uint64_t bhi) {
  // value = alo + 2^64 (ahi + blo) + 2^128 bhi
  const u128 P = ((u128)0xFFFFFFFFFFFFFFFFull << 64) - ((u128)27ull << 64) + 1;  // 2^128-28*2^64+1
  const u128 x1 = (u128)ahi + blo;                  // < 2^65
  const u128 x2 = (u128)bhi + (uint64_t)(x1 >> 64);  // small
  const u128 v = ((u128)(uint64_t)x1 << 64) | alo;   // < 2^128
  const u128 k = (u128)(uint64_t)x2 * 28u;           // 2^128 x2 = x2 (28 2^64 - 1)
  u128 t = v + (k << 64);
  if (t < v) t += ((u128)28u << 64) - 1;              // carry out of 2^128
  t -= (uint64_t)x2;                                  // no underflow: k << 64 >= x2
  while (t >= P) t -= P;
  return t;
}

}  // namespace accum_fold
