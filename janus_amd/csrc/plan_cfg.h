// Host planning of one VDAF instance, no HIP: every length of the instance from
// (kind, bits, length, chunk), the ABI's size report, and the Montgomery-form FLP tables the
// engine uploads.  Included by engine.hip; built alone with g++ by tests/test_host_plan.py.
#pragma once
#include <stdint.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/prio3gpu.h"
#include "cfg.h"

namespace p3g {

typedef unsigned __int128 u128;

// ---- host modular arithmetic for table setup only ---------------------------------------------
inline u128 addmod(u128 x, u128 y, u128 p) {
  u128 s = x + y;
  if (s < x || s >= p) s -= p;
  return s;
}
inline u128 mulmod(u128 a, u128 b, u128 p) {
  u128 r = 0;
  a %= p;
  while (b) {
    if (b & 1) r = addmod(r, a, p);
    a = addmod(a, a, p);
    b >>= 1;
  }
  return r;
}
inline u128 powmod(u128 a, u128 e, u128 p) {
  u128 r = 1;
  while (e) {
    if (e & 1) r = mulmod(r, a, p);
    a = mulmod(a, a, p);
    e >>= 1;
  }
  return r;
}
const u128 P128 = ((u128)0xFFFFFFFFFFFFFFE4ull << 64) | 1u;
const u128 P64 = (u128)0xFFFFFFFF00000001ull;

inline uint32_t next_pow2(uint32_t x) {
  uint32_t r = 1;
  while (r < x) r <<= 1;
  return r;
}
inline uint32_t ilog2(uint32_t x) {
  uint32_t l = 0;
  while ((1u << l) < x) ++l;
  return l;
}

// prio `optimal_chunk_length` (src/vdaf/prio3.rs, ext): among gadget_calls = 2^k - 1,
// k = round(log2(len + 1)) .. 1, the chunk length minimising the ParallelSum(Mul) proof length
// 2 chunk + 2 ((1 + calls).next_power_of_two() - 1) + 1; the first minimum (largest k) wins.
inline uint32_t optimal_chunk_length(uint32_t len) {
  if (len <= 1) return 1;
  const int max_log2 = (int)std::lround(std::log2((double)len + 1.0));
  uint64_t best_cost = ~0ull;
  uint32_t best = 1;
  for (int k = max_log2; k >= 1; --k) {
    const uint64_t calls = (1ull << k) - 1;
    const uint64_t chunk = (len + calls - 1) / calls;
    const uint64_t cost = 2 * chunk + 2 * (next_pow2((uint32_t)(1 + calls)) - 1) + 1;
    if (cost < best_cost) {
      best_cost = cost;
      best = (uint32_t)chunk;
    }
  }
  return best;
}

// Every field of `g` except the engine options (exact_squeeze, wave_prio stays 1, xof) and the
// device table pointers, which are left null.  A bad shape is PRIO3GPU_E_ARG with *err set.
inline int derive_cfg(int kind, uint32_t bits, uint32_t length, uint32_t chunk, Cfg* out,
                      std::string* err) {
  Cfg& g = *out;
  auto bad = [&](const std::string& msg) {
    *err = msg;
    return (int)PRIO3GPU_E_ARG;
  };
  g = Cfg{};
  g.kind = (uint32_t)kind;
  g.wave_prio = 1u;
  // VDAF-07 algorithm IDs: Count 0, Sum 1, SumVec 2, Histogram 3; FixedPoint L2 0xFFFF0000
  g.algo_id = kind == PRIO3GPU_FPVEC ? 0xFFFF0000u : (uint32_t)kind;
  g.qr_len = kind == PRIO3GPU_FPVEC ? 2u : 1u;
  uint32_t calls = 0, arity = 0, prove_rand = 0;
  switch (kind) {
    case PRIO3GPU_COUNT:
      g.es = 8;
      g.meas_len = 1;
      g.out_len = 1;
      g.jr_len = 0;
      calls = 1;
      arity = 2;
      prove_rand = 2;
      break;
    case PRIO3GPU_SUM:
      if (bits == 0 || bits > 64) return bad("Prio3Sum: bits must be in 1..64");
      g.es = 16;
      g.meas_len = bits;
      g.out_len = 1;
      g.jr_len = 1;
      calls = bits;
      arity = 1;
      prove_rand = 1;
      break;
    case PRIO3GPU_SUMVEC:
      if (bits == 0 || bits > 64 || length == 0 || chunk == 0)
        return bad("Prio3SumVec: bad parameters");
      g.es = 16;
      g.meas_len = bits * length;
      g.out_len = length;
      g.jr_len = 1;
      calls = (g.meas_len + chunk - 1) / chunk;
      arity = 2 * chunk;
      prove_rand = 2 * chunk;
      break;
    case PRIO3GPU_HISTOGRAM:
      if (length == 0 || chunk == 0) return bad("Prio3Histogram: bad parameters");
      g.es = 16;
      g.meas_len = length;
      g.out_len = length;
      g.jr_len = 2;
      calls = (length + chunk - 1) / chunk;
      arity = 2 * chunk;
      prove_rand = 2 * chunk;
      break;
    case PRIO3GPU_FPVEC:
      if ((bits != 16 && bits != 32 && bits != 64) || length == 0)
        return bad("Prio3FixedPointBoundedL2VecSum: bits must be 16, 32 or 64 and length >= 1");
      g.es = 16;
      g.meas_len = bits * length + 2 * bits - 2;  // entry bits || norm bits
      g.out_len = length;
      g.jr_len = 2;
      chunk = optimal_chunk_length(g.meas_len);
      calls = (g.meas_len + chunk - 1) / chunk;
      arity = 2 * chunk;
      g.chunk1 = optimal_chunk_length(length);
      g.calls1 = (length + g.chunk1 - 1) / g.chunk1;
      prove_rand = 2 * chunk + g.chunk1;
      break;
    default:
      return bad("unknown kind " + std::to_string(kind));
  }
  g.bits = bits;
  g.length = length;
  g.chunk =
      (kind == PRIO3GPU_SUMVEC || kind == PRIO3GPU_HISTOGRAM || kind == PRIO3GPU_FPVEC) ? chunk : 0;
  g.calls = calls;
  g.arity = arity;
  g.prove_rand_len = prove_rand;
  g.m = next_pow2(1 + calls);
  g.logm = ilog2(g.m);
  if (g.m > 4096) return bad("gadget too large (m = " + std::to_string(g.m) + ")");
  g.gp_len = 2 * (g.m - 1) + 1;  // every gadget here has degree 2
  g.proof_len = arity + g.gp_len;
  g.verifier_len = 1 + arity + 1;
  if (kind == PRIO3GPU_FPVEC) {
    g.m1 = next_pow2(1 + g.calls1);
    g.logm1 = ilog2(g.m1);
    g.gp_len1 = 2 * (g.m1 - 1) + 1;
    g.proof_len += g.chunk1 + g.gp_len1;
    g.verifier_len += g.chunk1 + 1;
    // k_fpv_weights keeps three m-entry tables and an r-power table in LDS
    if (g.m > 2048 || g.chunk + 1 > 4096 ||
        (size_t)16 * (3 * (size_t)g.m + g.chunk + 1 + 12) + 16 > 160 * 1024)
      return bad("FixedPointBoundedL2VecSum: length " + std::to_string(length) +
                 " too large (m = " + std::to_string(g.m) + ", chunk = " +
                 std::to_string(g.chunk) + ")");
  }
  const uint32_t es = g.es;
  g.leader_share_len = es * (g.meas_len + g.proof_len) + (g.jr_len ? 16 : 0);
  g.helper_share_len = g.jr_len ? 48 : 32;
  g.public_share_len = g.jr_len ? 32 : 0;
  g.prep_share_len = es * g.verifier_len + (g.jr_len ? 16 : 0);
  g.prep_msg_len = g.jr_len ? 16 : 0;
  return 0;
}

// What prio3gpu_ctx_sizes reports for a derived Cfg.
inline prio3gpu_sizes cfg_sizes(const Cfg& g) {
  prio3gpu_sizes s{};
  s.field_size = g.es;
  s.meas_len = g.meas_len;
  s.proof_len = g.proof_len;
  s.verifier_len = g.verifier_len;
  s.joint_rand_len = g.jr_len;
  s.output_len = g.out_len;
  s.leader_input_share = g.leader_share_len;
  s.helper_input_share = g.helper_share_len;
  s.public_share = g.public_share_len;
  s.prep_share = g.prep_share_len;
  s.prep_msg = g.prep_msg_len;
  s.aggregate_share = g.out_len * g.es;
  return s;
}

inline u128 field_modulus(uint32_t es) { return es == 16 ? P128 : P64; }

// The little-endian es-byte encodings of tv[k] * R mod p (Montgomery form, R = 2^(8 es)).
inline std::vector<uint8_t> mont_table(const std::vector<u128>& tv, uint32_t es) {
  const u128 p = field_modulus(es);
  const u128 R = (es == 16) ? (u128)0 - P128 /* 2^128 mod p */ : ((u128)1 << 64) % P64;
  std::vector<uint8_t> tw(tv.size() * es);
  for (size_t k = 0; k < tv.size(); ++k) {
    const u128 mv = mulmod(tv[k], R, p);
    for (uint32_t b = 0; b < es; ++b) tw[k * es + b] = (uint8_t)(mv >> (8 * b));
  }
  return tw;
}

// FLP tables of one gadget (Montgomery form), 3m + 1 entries:
//   [0, m)        alpha_m^k
//   m             1/m
//   [m+1, 2m+1)   S_i = sum_{k=1..calls} alpha_m^(ik)   (gadget-output sum as a dot product)
//   [2m+1, 3m+1)  alpha_m^k / m                          (Lagrange weight scale)
inline std::vector<uint8_t> gadget_table(uint32_t m, uint32_t calls, uint32_t es) {
  const u128 p = field_modulus(es);
  const u128 alpha = powmod(7, (p - 1) / m, p);
  const u128 inv_m = p - (p - 1) / m;
  std::vector<u128> tv(3 * (size_t)m + 1);
  u128 a = 1;
  for (uint32_t k = 0; k < m; ++k) {
    tv[k] = a;
    tv[2 * m + 1 + k] = mulmod(a, inv_m, p);
    a = mulmod(a, alpha, p);
  }
  tv[m] = inv_m;
  for (uint32_t i = 0; i < m; ++i) {
    const u128 x = tv[i];  // alpha^i
    u128 y = x, acc = 0;
    for (uint32_t k = 1; k <= calls; ++k) {
      acc = addmod(acc, y, p);
      y = mulmod(y, x, p);
    }
    tv[m + 1 + i] = acc;
  }
  return mont_table(tv, es);
}

// prover table: w^k (k < 2m, w = primitive 2m-th root), 1/m, 1/(2m); Montgomery
inline std::vector<uint8_t> prover_table(uint32_t m, uint32_t es) {
  const u128 p = field_modulus(es);
  const uint32_t m2 = 2 * m;
  const u128 w = powmod(7, (p - 1) / m2, p);
  std::vector<u128> tv((size_t)m2 + 2);
  u128 x = 1;
  for (uint32_t k = 0; k < m2; ++k) {
    tv[k] = x;
    x = mulmod(x, w, p);
  }
  tv[m2] = p - (p - 1) / m;
  tv[m2 + 1] = p - (p - 1) / m2;
  return mont_table(tv, es);
}

}  // namespace p3g
