/* prio3gpu_test.h -- test and benchmark hooks of libprio3gpu.so, kept out of the product ABI
 * (include/prio3gpu.h).  A Janus build binds only prio3gpu.h (rust/aggregator/src/gpu/ffi.rs);
 * these entry points exist for the parity tests (tests/test_gpu_squeeze.py,
 * tests/test_gpu_flp_branches.py, tests/test_gpu_field_ops.py) and the host benchmarks
 * (tools/hpke_bench.py). */
#ifndef PRIO3GPU_TEST_H
#define PRIO3GPU_TEST_H

#include "prio3gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* TEST ONLY.  The XOF squeeze every kernel runs (prio `into_field_vec`, reached through
 * XofShake128::next_vec: ES-byte LE chunks, reject >= p) over caller-crafted rate blocks instead
 * of Keccak output: blocks[25 i .. 25 i + 25) is the state after the i-th permutation (words
 * 0..20 are the 168-byte rate block).  field_size 8 or 16; exact != 0 forces the per-element path
 * (as PRIO3GPU_EXACT_SQUEEZE=1 does in the real kernels).  Runs on the current HIP device. */
int prio3gpu_test_squeeze(int field_size, const uint64_t* blocks, size_t nblocks, uint32_t n,
                          uint8_t* out, int exact);
/* TEST ONLY.  The FLP-query phase of prepare_init (agg_id 0) over caller-supplied randomness
 * instead of the XOF's: leader_input_shares n x leader_input_share, query_rand n x qr_len x
 * field_size (qr_len = 1, 2 for FixedPoint), joint_rand n x joint_rand_len x field_size, own_parts
 * n x 16 (the prep share's joint-rand part).  Writes the prep shares; a query point that is a root
 * of unity sets status 5 (VdafPrepError), as prio does.  Lets tests reach the branches that
 * SHAKE128 output reaches with negligible probability (t^m == 1, r^m == 1). */
int prio3gpu_test_flp_query(prio3gpu_ctx* ctx, size_t n, const uint8_t* leader_input_shares,
                            const uint8_t* query_rand, const uint8_t* joint_rand,
                            const uint8_t* own_parts, uint8_t* out_prep_shares, uint8_t* status);

/* Device memory helpers (bench / tests that stage inputs in HBM without torch). */
int prio3gpu_dev_alloc(prio3gpu_ctx* ctx, size_t bytes, void** out);
int prio3gpu_dev_free(prio3gpu_ctx* ctx, void* p);
int prio3gpu_memcpy(prio3gpu_ctx* ctx, void* dst, const void* src, size_t bytes);

/* The batched HPKE open's X25519 ladder: on != 0 (default where the CPU has AVX-512 IFMA) runs
 * 8 reports per AVX-512 IFMA ladder, 0 the scalar radix-2^51 ladder for every report (A/B of the
 * two ladders in tools/hpke_bench.py; both are checked against each other in tests/test_hpke.py).
 * Process-wide; returns the previous setting, or PRIO3GPU_E_UNSUPPORTED for on != 0 on a CPU
 * without IFMA. */
int prio3gpu_test_hpke_set_ifma(int on);

/* TEST ONLY.  The GPU open's X25519 ladder alone (k_x25519, one lane per point): out[i] =
 * X25519(sk, points[i]) for n 32-byte points under one 32-byte private key (clamped inside), the
 * GPU counterpart of prio3gpu_x25519_batch.  points / out may be host or device memory. */
int prio3gpu_test_x25519_gpu(prio3gpu_ctx* ctx, const uint8_t* sk, const uint8_t* points, size_t n,
                             uint8_t* out);

/* TEST ONLY.  The GPU open's P-256 scalar multiplication alone (k_p256_dh without its KEM half,
 * one lane per point), the counterpart of prio3gpu_test_x25519_gpu: for n 65-byte uncompressed
 * encodings under one 32-byte big-endian scalar sk, out_x[32 i .. 32 i + 32) is the big-endian x
 * coordinate of [sk] P_i and ok[i] = 1 -- or 32 zero bytes and ok[i] = 0 for an encoding
 * DeserializePublicKey refuses (first byte not 0x04, a coordinate >= p, a point off the curve).
 * An all-zero x with ok[i] = 1 is a result, not a failure.  sk = 0 or sk >= n returns
 * PRIO3GPU_E_HPKE and launches nothing.  All host memory; n == 0 returns 0 and launches
 * nothing. */
int prio3gpu_test_p256_gpu(prio3gpu_ctx* ctx, const uint8_t* sk, const uint8_t* points, size_t n,
                           uint8_t* out_x, uint8_t* ok);

/* TEST ONLY.  The GPU seal's P-256 ladders alone (k_p256_eph without the KEM half that follows it,
 * two lanes per report), the counterpart of prio3gpu_test_p256_gpu for the sender: for n 32-byte
 * big-endian ephemeral scalars sk_es under one recipient key pk65 (0x04 || x || y),
 * out_enc[65 i .. 65 i + 65) is enc = 0x04 || x || y of [sk_e_i] G, out_dh_x[32 i .. 32 i + 32)
 * the big-endian x coordinate of [sk_e_i] pk, and ok[i] = 1 -- or zeros in both and ok[i] = 0 for
 * a scalar outside [1, n).  An all-zero x with ok[i] = 1 is a result, not a failure.  A pk65 that
 * DeserializePublicKey refuses returns PRIO3GPU_E_HPKE and launches nothing.  All host memory;
 * n == 0 returns 0 and launches nothing. */
int prio3gpu_test_p256_eph_gpu(prio3gpu_ctx* ctx, const uint8_t* pk65, const uint8_t* sk_es,
                               size_t n, uint8_t* out_enc, uint8_t* out_dh_x, uint8_t* ok);

/* TEST ONLY.  The device Poly1305 (janus_amd/csrc/hpke_prims.h: poly1305_mac, RFC 8439 §2.5) alone,
 * one lane per message: tags[16 i .. 16 i + 16) is the MAC of msgs[msg_offsets[i] ..
 * msg_offsets[i + 1]) under keys[32 i .. 32 i + 32) (r || s; r is clamped inside).  The HPKE-level
 * calls derive r from the key schedule, so only this hook can feed the final reduction the
 * accumulators p - 1, p and 2^130 - 2.  keys n x 32, msg_offsets n + 1 (ascending), tags n x 16;
 * all host memory.  n == 0 returns 0 and launches nothing. */
int prio3gpu_test_poly1305_gpu(prio3gpu_ctx* ctx, const uint8_t* keys, const uint8_t* msgs,
                               const uint64_t* msg_offsets, size_t n, uint8_t* tags);

/* TEST ONLY.  One field primitive over caller-supplied operands, one lane per tuple: the device
 * functions the product kernels call (Field128Ops / Field64Ops, the generated carry chains and
 * fused Montgomery programs, the lazy dot product, the inverses), run alone so that tests can
 * feed them the operands uniform XOF output never produces (tests/test_gpu_field_ops.py).
 * field_size 8 or 16; in is n x arity(op) x field_size bytes of little-endian elements, out
 * n x results(op) x field_size bytes, both host memory.  op (operands -> results; R = 2^64 or
 * 2^128; "128" = Field128 only):
 *    0 add  1 sub            a b -> a + b, a - b
 *    2 neg  3 dbl            a -> -a, 2a
 *    4 mul                   a b -> a b / R
 *    5 to_mont  6 from_mont  a -> a R, a / R
 *    7 is_canonical          any field_size-byte value -> 1 if < p, else 0
 *    8 inv                   x -> R^2 / x (Montgomery in and out), 0 -> 0
 *    9 inv_plain (128)       x -> 1 / x, 0 -> 0
 *   10 pow                   x -> x^param in Montgomery form (x R -> x^param R)
 *   11 mul2  12 mul3  13 mul5 (128)   a0 b0 .. a(k-1) b(k-1) -> k products a_s b_s / R
 *   14 fma2_mul1 (128)       a0 b0 c0 d0  a1 b1 c1 d1  a2 b2
 *                            -> (a0 b0 + c0 d0)/R, (a1 b1 + c1 d1)/R, a2 b2/R
 *   15 q1_fma1_mul1 (128)    a0 b0 c0 d0 e0 f0 i0 j0  a1 b1 c1 d1  a2 b2
 *                            -> (a0 b0 + c0 d0 + e0 f0 + i0 j0)/R, (a1 b1 + c1 d1)/R, a2 b2/R
 *   16 addsub_AASS (128)     a0 b0 .. a3 b3 -> a0 + b0, a1 + b1, a2 - b2, a3 - b3
 *   17 addsub_ASAA (128)     a0 b0 .. a3 b3 -> a0 + b0, a1 - b1, a2 + b2, a3 + b3
 *   18 addsub_A (128)        a b -> a + b
 *   19 dot (128)             a_0 x_0 .. a_(param-1) x_(param-1) -> (sum a_k x_k) / R,
 *                            1 <= param < 2^30
 *   20 limb_sums (128)       four little-endian u64 xs[0..3] (32 bytes) -> sum xs[q] 2^(32 q)
 * All results are canonical (mod p).  Inputs must be < p except for is_canonical and limb_sums.
 * n == 0 returns 0 and launches nothing; an unknown op, a Field128-only op with field_size 8, or
 * null pointers with n > 0 return PRIO3GPU_E_ARG.  Runs on the current HIP device. */
int prio3gpu_test_field_op(int field_size, int op, uint32_t param, const uint8_t* in, size_t n,
                           uint8_t* out);

/* k_req_gather alone (janus_amd/csrc/helper_request.h): the gather stage of
 * prio3gpu_helper_init_request over the n views of `msg` (host or device memory; the views are
 * host memory and are checked against msg_len first, PRIO3GPU_E_ARG if one does not fit), with the
 * outputs of prio3gpu_gather_prepare_inits copied back to host memory: nonces n x 16, public
 * shares n x public_share, leader prep shares n x prep_share (rows of faulty reports zeroed) and
 * faults n bytes.  n == 0 returns 0 and launches nothing. */
int prio3gpu_test_req_gather(prio3gpu_ctx* ctx, const uint8_t* msg, size_t msg_len,
                             const prio3gpu_prepare_init_view* views, size_t n, uint8_t* nonces,
                             uint8_t* public_shares, uint8_t* leader_prep_shares,
                             uint8_t* faults);

#ifdef __cplusplus
}
#endif

#endif /* PRIO3GPU_TEST_H */
