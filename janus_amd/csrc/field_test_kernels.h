// TEST ONLY (prio3gpu_test_field_op, include/prio3gpu_test.h): one field primitive over
// caller-supplied operands, one lane per tuple, so tests can feed the carry chains and selects the
// operands that SHAKE128 output reaches with probability 2^-32 .. 2^-59 (sums in [p, 2^128), zero
// reduction words, equal low limbs, ...).  Every op calls the DEVI function the product kernels
// call; nothing is re-implemented here.
//
// A tuple is arity(op) elements of FO::ES little-endian bytes, a result results(op) elements.
// The operands are read in the order of the device function's signature, outputs skipped:
//   add, sub, mul, addsub_A     a, b                                    -> r
//   neg, dbl, to_mont, from_mont, is_canonical, inv, inv_plain, pow  a  -> r
//   mul2          a0 b0 | a1 b1                                         -> r0 r1
//   mul3          a0 b0 | a1 b1 | a2 b2                                 -> r0 r1 r2
//   mul5          a0 b0 | ... | a4 b4                                   -> r0 .. r4
//   fma2_mul1     a0 b0 c0 d0 | a1 b1 c1 d1 | a2 b2                     -> r0 r1 r2
//                 r0 = (a0 b0 + c0 d0)/R, r1 = (a1 b1 + c1 d1)/R, r2 = a2 b2/R
//   q1_fma1_mul1  a0 b0 c0 d0 e0 f0 i0 j0 | a1 b1 c1 d1 | a2 b2         -> r0 r1 r2
//                 r0 = (a0 b0 + c0 d0 + e0 f0 + i0 j0)/R, r1 = (a1 b1 + c1 d1)/R, r2 = a2 b2/R
//   addsub_AASS   a0 b0 | a1 b1 | a2 b2 | a3 b3    -> a0+b0, a1+b1, a2-b2, a3-b3
//   addsub_ASAA   a0 b0 | a1 b1 | a2 b2 | a3 b3    -> a0+b0, a1-b1, a2+b2, a3+b3
//   dot           a_0 x_0 | ... | a_(param-1) x_(param-1)   -> (sum a_k x_k)/R
//   limb_sums     xs[0..3] as four little-endian u64 (two element slots)  -> sum xs[q] 2^(32 q)
#pragma once
#include "prio3_kernels.h"

namespace p3g {

enum FieldTestOp : int {
  FT_ADD = 0,
  FT_SUB = 1,
  FT_NEG = 2,
  FT_DBL = 3,
  FT_MUL = 4,
  FT_TO_MONT = 5,
  FT_FROM_MONT = 6,
  FT_IS_CANONICAL = 7,
  FT_INV = 8,
  FT_INV_PLAIN = 9,  // Field128 only from here on, except FT_POW
  FT_POW = 10,
  FT_MUL2 = 11,
  FT_MUL3 = 12,
  FT_MUL5 = 13,
  FT_FMA2_MUL1 = 14,
  FT_Q1_FMA1_MUL1 = 15,
  FT_ADDSUB_AASS = 16,
  FT_ADDSUB_ASAA = 17,
  FT_ADDSUB_A = 18,
  FT_DOT = 19,
  FT_LIMB_SUMS = 20,
  FT_NOPS = 21
};

// elements per tuple (FT_DOT: 2 * param, given at run time) and per result
__host__ __device__ constexpr uint32_t field_test_arity(int op) {
  switch (op) {
    case FT_ADD: case FT_SUB: case FT_MUL: case FT_ADDSUB_A: case FT_LIMB_SUMS: return 2;
    case FT_MUL2: return 4;
    case FT_MUL3: return 6;
    case FT_MUL5: case FT_FMA2_MUL1: return 10;
    case FT_Q1_FMA1_MUL1: return 14;
    case FT_ADDSUB_AASS: case FT_ADDSUB_ASAA: return 8;
    case FT_DOT: return 0;
    default: return 1;
  }
}
__host__ __device__ constexpr uint32_t field_test_results(int op) {
  switch (op) {
    case FT_MUL2: return 2;
    case FT_MUL3: case FT_FMA2_MUL1: case FT_Q1_FMA1_MUL1: return 3;
    case FT_MUL5: return 5;
    case FT_ADDSUB_AASS: case FT_ADDSUB_ASAA: return 4;
    default: return 1;
  }
}
inline bool field_test_op_has_field64(int op) {
  return (op >= FT_ADD && op <= FT_INV) || op == FT_POW;
}

// Tail lanes read tuple n - 1 (so the asm chains run in every lane of the last wave) and store
// nothing.
template <class FO, int OP>
__global__ void __launch_bounds__(64) k_test_field_op(uint32_t n, uint32_t param,
                                                      const uint8_t* in, uint8_t* out) {
  using T = typename FO::T;
  constexpr size_t ES = FO::ES;
  constexpr uint32_t NR = field_test_results(OP);
  const uint32_t arity = OP == FT_DOT ? 2u * param : field_test_arity(OP);
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = r < n;
  const uint8_t* src = in + (size_t)(live ? r : n - 1) * arity * ES;
  auto ld = [&](uint32_t k) { return FO::load(src + (size_t)k * ES); };
  T res[NR];
  if constexpr (OP == FT_ADD) res[0] = FO::add(ld(0), ld(1));
  if constexpr (OP == FT_SUB) res[0] = FO::sub(ld(0), ld(1));
  if constexpr (OP == FT_NEG) res[0] = FO::neg(ld(0));
  if constexpr (OP == FT_DBL) res[0] = FO::dbl(ld(0));
  if constexpr (OP == FT_MUL) res[0] = FO::mul(ld(0), ld(1));
  if constexpr (OP == FT_TO_MONT) res[0] = FO::to_mont(ld(0));
  if constexpr (OP == FT_FROM_MONT) res[0] = FO::from_mont(ld(0));
  if constexpr (OP == FT_IS_CANONICAL) res[0] = FO::from_u32(FO::is_canonical(ld(0)) ? 1u : 0u);
  if constexpr (OP == FT_INV) res[0] = inv_mont<FO>(ld(0));
  if constexpr (OP == FT_INV_PLAIN) {
    const T x = ld(0);
    inv128::inverse(x.w, res[0].w);
  }
  if constexpr (OP == FT_POW) res[0] = mont_pow<FO>(ld(0), (uint64_t)param);
  if constexpr (OP == FT_MUL2) mont_mul2(ld(0), ld(1), res[0], ld(2), ld(3), res[1]);
  if constexpr (OP == FT_MUL3)
    mont_mul3(ld(0), ld(1), ld(2), ld(3), ld(4), ld(5), res[0], res[1], res[2]);
  if constexpr (OP == FT_MUL5)
    mont_mul5(ld(0), ld(1), res[0], ld(2), ld(3), res[1], ld(4), ld(5), res[2], ld(6), ld(7),
              res[3], ld(8), ld(9), res[4]);
  if constexpr (OP == FT_FMA2_MUL1)
    mont_fma2_mul1(ld(0), ld(1), ld(2), ld(3), res[0], ld(4), ld(5), ld(6), ld(7), res[1], ld(8),
                   ld(9), res[2]);
  if constexpr (OP == FT_Q1_FMA1_MUL1)
    mont_q1_fma1_mul1(ld(0), ld(1), ld(2), ld(3), ld(4), ld(5), ld(6), ld(7), res[0], ld(8), ld(9),
                      ld(10), ld(11), res[1], ld(12), ld(13), res[2]);
  if constexpr (OP == FT_ADDSUB_AASS)
    modaddsub_AASS(ld(0), ld(1), res[0], ld(2), ld(3), res[1], ld(4), ld(5), res[2], ld(6), ld(7),
                   res[3]);
  if constexpr (OP == FT_ADDSUB_ASAA)
    modaddsub_ASAA(ld(0), ld(1), res[0], ld(2), ld(3), res[1], ld(4), ld(5), res[2], ld(6), ld(7),
                   res[3]);
  if constexpr (OP == FT_ADDSUB_A) modaddsub_A(ld(0), ld(1), res[0]);
  if constexpr (OP == FT_DOT) {
    Wide w;
    wide_zero(w);
#pragma unroll 1
    for (uint32_t k = 0; k < param; ++k) wide_mac(w, ld(2 * k), ld(2 * k + 1));
    res[0] = wide_reduce(w);
  }
  if constexpr (OP == FT_LIMB_SUMS) {
    const uint4 lo = *reinterpret_cast<const uint4*>(src);
    const uint4 hi = *reinterpret_cast<const uint4*>(src + 16);
    const uint64_t xs[4] = {((uint64_t)lo.y << 32) | lo.x, ((uint64_t)lo.w << 32) | lo.z,
                            ((uint64_t)hi.y << 32) | hi.x, ((uint64_t)hi.w << 32) | hi.z};
    res[0] = f128_reduce_limb_sums(xs);
  }
  if (live) {
#pragma unroll
    for (uint32_t k = 0; k < NR; ++k) FO::store(out + ((size_t)r * NR + k) * ES, res[k]);
  }
}

}  // namespace p3g
