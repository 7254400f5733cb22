// What the wave-per-report kernels share (hpke_open_team.h, hpke_seal_team.h, hpke_team_split.h):
// a wave's place in its block, what crosses its lanes, and the wave's open of one report after
// the DH.  Device code, but no kernel: each of the three kernel headers is one unit's alone, and
// this header is what lets every one of them stand without another.  Every lane of a wave derives
// the same key, nonce, round keys, H and AAD hash (registers only); the lanes then share the
// ciphertext by stripes (aes_gcm_team.h).  One pass: a block is absorbed by GHASH, decrypted and
// stored; the lanes' sums are XORed, every lane computes the tag, and on a mismatch each lane
// overwrites what it stored with zeros -- no unauthenticated plaintext outlives the kernel.  The
// wave's table of H^1 .. H^64 (LDS, key-derived) is zeroed before the wave ends.  With
// ChaCha20-Poly1305 (AEAD 3) the lanes share the ciphertext by 64-byte chunks
// (chacha_poly_team.h): a block is absorbed by Poly1305, decrypted and stored, the lanes' sums are
// added with a carry pass between the butterfly's halves, and the same verdict and wipe follow.
// That path builds no S-box, has no block barrier and takes no LDS: r's powers stay in registers.
// A lane's arithmetic is aes_gcm_team.h's and chacha_poly_team.h's, free of HIP and run by CPU
// tests too; kTeam and kTeamsPerBlock are hpke_shared.h's, where the host sees them.
#pragma once
#include "aes_gcm_team.h"
#include "chacha_poly_team.h"
#include "cfg.h"
#include "hpke_lane.h"

namespace p3g {

// Orders a wave's LDS writes before its later LDS reads (other lanes' entries of the table).
__device__ __forceinline__ void team_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// The sum of the 64 lanes' Poly1305 sums, on every lane: eight lanes' limbs fit 32 bits, sixty-four
// lanes' do not, so a carry pass sits between the butterfly's halves (poly1305_carry's bounds).
__device__ __forceinline__ void poly_team_sum(uint32_t h[5]) {
#pragma unroll
  for (int m = 1; m < 8; m *= 2) {
#pragma unroll
    for (int i = 0; i < 5; ++i) h[i] += (uint32_t)__shfl_xor((int)h[i], m);
  }
  poly1305_carry(h);
#pragma unroll
  for (int m = 8; m < (int)kTeam; m *= 2) {
#pragma unroll
    for (int i = 0; i < 5; ++i) h[i] += (uint32_t)__shfl_xor((int)h[i], m);
  }
  poly1305_carry(h);
}

// hpke_open_team_wave for ChaCha20-Poly1305: no S-box and no table.
template <int KDF, class Aad, class Sink>
__device__ __forceinline__ bool hpke_open_team_wave_chacha(const HpkeBatchConsts& bc,
                                                           const uint32_t* dhw, uint32_t nz,
                                                           const uint32_t* encw, const Aad& aad,
                                                           const uint8_t* ct, uint64_t body,
                                                           uint32_t lane, Sink& sink) {
  uint32_t key[8], nonce[3], tag[4], t[4], sum[5];
  hpke_key_nonce<KDF, 3>(bc, dhw, encw, key, nonce);
#pragma unroll
  for (int i = 0; i < 8; ++i) key[i] = bswap32(key[i]);
#pragma unroll
  for (int i = 0; i < 3; ++i) nonce[i] = bswap32(nonce[i]);
  PolyTeam pt;
  chacha_team_start(pt, key, nonce, aad, body, lane, kTeam);
  chacha_team_stripe<false>(pt, key, nonce, PackedBytes{ct, body}, lane, kTeam, sink);
#pragma unroll
  for (int i = 0; i < 5; ++i) sum[i] = pt.mac.h[i];
  poly_team_sum(sum);
  poly_team_tag(pt, sum, aad.len(), body, t);
  load_block(ct + body, 16, tag);
  uint32_t diff = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) diff |= t[i] ^ tag[i];  // no early exit
  const bool ok = diff == 0u && nz != 0u;
  if (!ok) chacha_team_wipe(sink, body, lane, kTeam);
  return ok;
}

// The wave's open of one report after the DH: true when the tag matches and the DH value is not
// all zero.  The plaintext has then gone through sink (body bytes); otherwise what the sink stored
// is zeros again.  tbl: 4 kTeam words of LDS of this wave's own, zero when the call returns.
template <int KDF, int AEAD, class Aad, class Sink>
__device__ __forceinline__ bool hpke_open_team_wave_gcm(const uint8_t* sbox, uint32_t* tbl,
                                                        const HpkeBatchConsts& bc,
                                                        const uint32_t* dhw, uint32_t nz,
                                                        const uint32_t* encw, const Aad& aad,
                                                        const uint8_t* ct, uint64_t body,
                                                        uint32_t lane, Sink& sink) {
  constexpr int NKW = hpke_aead_nk(AEAD) / 4;
  uint32_t key[NKW], nonce[3], rk[4 * (NKW + 7)], h[4], y0[4], ctr[4], tag[4], t[4];
  hpke_key_nonce<KDF, AEAD>(bc, dhw, encw, key, nonce);
  aes_gcm_start<NKW>(sbox, key, nonce, aad, rk, h, y0, ctr);
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) tbl[i] = h[i];
  }
  for (uint32_t half = 1; half < kTeam; half *= 2) {
    team_lds_sync();
    gf128_powers_step(tbl, lane, half);
  }
  team_lds_sync();
  uint32_t acc[4] = {0, 0, 0, 0}, y[4];
  gcm_team_stripe<NKW, true, true>(sbox, rk, ctr, tbl, y0, ct, body, lane, kTeam, acc, sink);
#pragma unroll
  for (int i = 0; i < 4; ++i) {  // the XOR of the 64 sums, on every lane
#pragma unroll
    for (int m = 1; m < (int)kTeam; m *= 2) acc[i] ^= (uint32_t)__shfl_xor((int)acc[i], m);
  }
  gcm_team_join(y, acc, y0, body);
  aes_gcm_tag<NKW>(sbox, rk, h, y, ctr, aad.len(), body, t);
  load_block(ct + body, 16, tag);
  uint32_t diff = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) diff |= t[i] ^ tag[i];  // no early exit
  const bool ok = diff == 0u && nz != 0u;
  if (!ok) gcm_team_wipe(sink, body, lane, kTeam);
#pragma unroll
  for (int i = 0; i < 4; ++i) tbl[4 * lane + i] = 0;
  return ok;
}

// Either of them, from the report's dh (8 words as k_x25519 wrote them) and enc (32 bytes); sbox
// and tbl are not read (null) for ChaCha20-Poly1305.  With bc.dh_ok set (P-256) dh is the
// shared_secret k_p256_dh left, dh_flag the report's validity byte in place of the all-zero test,
// and enc is not read: what hpke_open_lane does, on a wave-uniform branch.
template <int KDF, int AEAD, class Aad, class Sink>
__device__ __forceinline__ bool hpke_open_team_wave(const uint8_t* sbox, uint32_t* tbl,
                                                    const HpkeBatchConsts& bc, const uint32_t* dh,
                                                    const uint8_t* enc, const Aad& aad,
                                                    const uint8_t* ct, uint64_t body,
                                                    uint32_t lane, Sink& sink, uint32_t dh_flag) {
  uint32_t dhw[8], encw[8], nz = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t d = dh[i];
    nz |= d;
    dhw[i] = bswap32(d);
    encw[i] = 0;
  }
  if (bc.dh_ok) {
    nz = dh_flag;
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint8_t* e = enc + 4 * i;
      encw[i] = ((uint32_t)e[0] << 24) | ((uint32_t)e[1] << 16) | ((uint32_t)e[2] << 8) | e[3];
    }
  }
  if constexpr (AEAD == 3)
    return hpke_open_team_wave_chacha<KDF>(bc, dhw, nz, encw, aad, ct, body, lane, sink);
  else
    return hpke_open_team_wave_gcm<KDF, AEAD>(sbox, tbl, bc, dhw, nz, encw, aad, ct, body, lane,
                                              sink);
}

// A wave's place in its block: the block's S-box (built here, with the kernel's only block
// barrier), the wave's own table of powers, its lane and its report.  For ChaCha20-Poly1305
// (AEAD 3) only the lane and the report: no S-box, no table, no barrier and no LDS.
struct TeamWave {
  const uint8_t* sbox;
  uint32_t* tbl;
  uint32_t lane, r;
};

template <int AEAD>
__device__ __forceinline__ TeamWave team_wave_setup() {
  // the wave's index stays a per-lane value: made a scalar, everything a report's lanes derive
  // alike (the whole key schedule) would be compiled for the scalar unit
  const uint32_t wave = threadIdx.x / kTeam;
  const uint32_t lane = threadIdx.x % kTeam, r = blockIdx.x * kTeamsPerBlock + wave;
  if constexpr (AEAD == 3) {
    return TeamWave{nullptr, nullptr, lane, r};
  } else {
    __shared__ uint8_t sbox[256];
    __shared__ uint32_t tbls[kTeamsPerBlock][4 * kTeam];
    aes_sbox_fill(sbox, threadIdx.x, blockDim.x);
    __syncthreads();
    return TeamWave{sbox, tbls[wave], lane, r};
  }
}

// Zeros over what the wave's stripes stored, with the block-to-lane map of the suite's team AEAD.
template <int AEAD, class Sink>
__device__ __forceinline__ void team_wipe(Sink& sink, uint64_t len, uint32_t lane) {
  if constexpr (AEAD == 3) chacha_team_wipe(sink, len, lane, kTeam);
  else gcm_team_wipe(sink, len, lane, kTeam);
}

}  // namespace p3g
