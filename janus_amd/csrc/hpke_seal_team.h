// Batched HPKE seal of long plaintexts on the GPU, one WAVE per report: DHKEM(X25519, HKDF-SHA256)
// (and DHKEM(P-256, HKDF-SHA256) behind the context's "hpke_gpu_p256" option; its ladders are
// hpke_dh_gpu.h's k_p256_eph) with HKDF-SHA256 / -SHA384 / -SHA512 and AES-128-GCM / AES-256-GCM / ChaCha20-Poly1305, RFC 9180
// base mode, single shot.  What a DAP client does for the leader's input share of a hundred
// kilobytes, where hpke_seal_gpu.h's lane per report would walk it alone; the mirror of
// hpke_open_team.h:
//   k_hpke_seal_team<KDF, AEAD>          packed inputs with offsets, as k_hpke_seal takes them
//   k_hpke_seal_team_shares<KDF, AEAD>   Prio3 input-share rows in, enc and payload columns out: the
//                                        PlaintextInputShare and the InputShareAad are byte sources
//                                        over the caller's rows and are never written to memory
// The ladders are hpke_dh_gpu.h's k_x25519_eph, one lane per report and point, launched before.
// Four reports per block; the only block barrier is the one after the S-box build (reports differ
// in length).  Every lane of a wave derives the same key, nonce, round keys, H and AAD hash
// (registers only); the lanes then share the plaintext by stripes (aes_gcm_team.h): a block is
// encrypted, stored and absorbed by GHASH; the lanes' sums are XORed, every lane computes the tag
// and one lane stores it.  The wave's table of H^1 .. H^64 (LDS, key-derived) is zeroed before the
// wave ends.  With ChaCha20-Poly1305 (AEAD 3) the lanes share the plaintext by 64-byte chunks
// (chacha_poly_team.h): a block is encrypted, stored and absorbed by Poly1305, and the lanes' sums
// are added by hpke_team_wave.h's poly_team_sum; no S-box, no block barrier, no LDS.  Only the
// kernels and what crosses lanes are here; a lane's arithmetic is aes_gcm_team.h's and
// chacha_poly_team.h's, free of HIP and run by CPU tests too.  The wave's place in its block
// (team_wave_setup, team_lds_sync) is hpke_team_wave.h's.  Included by
// engine_hpke_team.hip alone.
#pragma once
#include "hpke_team_wave.h"

namespace p3g {

// A report that is not sealed, by the whole team: zeros in its enc and ciphertext slots; status 4
// unless it was skipped on entry.
__device__ __forceinline__ void hpke_seal_team_reject(uint8_t* enc_out, uint8_t* ct,
                                                      uint64_t ct_cap, uint8_t* status, bool skip,
                                                      uint32_t lane, uint32_t nenc) {
  team_zero(enc_out, nenc, lane, kTeam);
  team_zero(ct, ct_cap, lane, kTeam);
  if (!skip && lane == 0) *status = ST_HPKE_DECRYPT;
}

// The wave's seal of one report after the ladders, with hpke_seal_lane's contract: enc and dh are
// the report's 8 little-endian words each as k_x25519_eph wrote them; enc_out gets the 32 bytes of
// enc, ct gets pt.len() + 16 bytes (ciphertext || tag) and zeros up to ct_cap -- or everything
// zeros and status 4 when the DH value is all zero, before any key is derived.  With bc.dh_ok set
// (P-256) dh is the finished shared_secret, dh_flag the report's validity byte in place of the
// all-zero test, enc the 64 bytes x || y, and enc_out gets the 65 bytes 0x04 || x || y, a byte per
// lane; the KEM is a wave-uniform branch.  tbl: 4 kTeam words of LDS of this wave's own, zero when
// the call returns; sbox and tbl are not read (null) for ChaCha20-Poly1305.
template <int KDF, int AEAD, class Pt, class Aad>
__device__ __forceinline__ void hpke_seal_team_wave(const uint8_t* sbox, uint32_t* tbl,
                                                    const HpkeBatchConsts& bc, const uint32_t* enc,
                                                    const uint32_t* dh, const Pt& pt,
                                                    const Aad& aad, uint8_t* enc_out, uint8_t* ct,
                                                    uint64_t ct_cap, uint8_t* status,
                                                    uint32_t lane, uint32_t dh_flag) {
  uint32_t dhw[8], encw[8], ence[8], nz = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t d = dh[i];
    nz |= d;
    dhw[i] = bswap32(d);
    ence[i] = encw[i] = 0;
  }
  if (bc.dh_ok) {
    nz = dh_flag;
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      ence[i] = enc[i];
      encw[i] = bswap32(ence[i]);
    }
  }
  if (nz == 0u) {  // alike on every lane of the wave
    hpke_seal_team_reject(enc_out, ct, ct_cap, status, false, lane, bc.nenc);
    return;
  }
  constexpr int NKW = hpke_aead_nk(AEAD) / 4;
  uint32_t key[NKW], nonce[3], t[4];
  hpke_key_nonce<KDF, AEAD>(bc, dhw, encw, key, nonce);
  const uint64_t plen = pt.len();
  CtSink sink{ct};
  if constexpr (AEAD == 3) {  // chacha_poly_team.h: no S-box and no table
    uint32_t sum[5];
#pragma unroll
    for (int i = 0; i < NKW; ++i) key[i] = bswap32(key[i]);
#pragma unroll
    for (int i = 0; i < 3; ++i) nonce[i] = bswap32(nonce[i]);
    PolyTeam mac;
    chacha_team_start(mac, key, nonce, aad, plen, lane, kTeam);
    chacha_team_stripe<true>(mac, key, nonce, pt, lane, kTeam, sink);
#pragma unroll
    for (int i = 0; i < 5; ++i) sum[i] = mac.mac.h[i];
    poly_team_sum(sum);
    poly_team_tag(mac, sum, aad.len(), plen, t);
  } else {
    uint32_t rk[4 * (NKW + 7)], h[4], y0[4], ctr[4];
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
    gcm_team_seal_stripe<NKW>(sbox, rk, ctr, tbl, y0, pt, lane, kTeam, acc, sink);
#pragma unroll
    for (int i = 0; i < 4; ++i) {  // the XOR of the 64 sums, on every lane
#pragma unroll
      for (int m = 1; m < (int)kTeam; m *= 2) acc[i] ^= (uint32_t)__shfl_xor((int)acc[i], m);
    }
    gcm_team_join(y, acc, y0, plen);
    aes_gcm_tag<NKW>(sbox, rk, h, y, ctr, aad.len(), plen, t);
  }
  if (lane == 0) store_block_any(ct + plen, t);
  if (bc.dh_ok) {  // enc: 0x04, then a byte of x || y from each lane
    if (lane == 0) enc_out[0] = 0x04;
    enc_out[1 + lane] = reinterpret_cast<const uint8_t*>(enc)[lane];
  } else if (lane < 2) {  // enc: sixteen bytes from each of two lanes
    uint32_t e[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) e[i] = lane ? ence[4 + i] : ence[i];
    store_block_any(enc_out + 16 * lane, e);
  }
  team_zero(ct + plen + 16, ct_cap - plen - 16, lane, kTeam);
  if constexpr (AEAD != 3) {
#pragma unroll
    for (int i = 0; i < 4; ++i) tbl[4 * lane + i] = 0;
  }
}

// One wave per report over packed inputs, with k_hpke_seal's arguments and contracts: report r's
// ciphertext || tag goes to cts[ct_off[r] .. ct_off[r + 1]) and its enc to encs[bc.nenc r ..].  A slot
// shorter than the plaintext + 16 or offsets that do not fit: zeros and status 4.  A report whose
// status is non-zero on entry keeps it and gets zeros.  `eph` is k_x25519_eph's output (n encs,
// then n DH values) or, with bc.dh_ok set, k_p256_eph's and k_p256_eph_kem's.
template <int KDF, int AEAD>
__global__ void __launch_bounds__(256) k_hpke_seal_team(
    uint32_t n, HpkeBatchConsts bc, const uint32_t* eph, const uint8_t* aads,
    const uint64_t* aad_off, uint64_t aad_total, const uint8_t* pts, const uint64_t* pt_off,
    uint64_t pt_total, uint8_t* encs, uint8_t* cts, const uint64_t* ct_off, uint64_t ct_total,
    uint8_t* status) {
  const TeamWave w = team_wave_setup<AEAD>();
  const uint32_t r = w.r, lane = w.lane;
  if (r >= n) return;
  const uint64_t a0 = aad_off[r], a1 = aad_off[r + 1], p0 = pt_off[r], p1 = pt_off[r + 1];
  const uint64_t c0 = ct_off[r], c1 = ct_off[r + 1];
  const bool ct_fits = c0 <= c1 && c1 <= ct_total;
  const uint64_t ct_cap = ct_fits ? c1 - c0 : 0;
  uint8_t* ct = cts + (ct_fits ? c0 : 0);
  uint8_t* enc_out = encs + (size_t)r * bc.nenc;
  const bool skip = status[r] != 0;
  const bool ok = !skip && ct_fits && a0 <= a1 && a1 <= aad_total && p0 <= p1 && p1 <= pt_total &&
                  ct_cap >= 16 && p1 - p0 <= ct_cap - 16;
  if (!ok) {  // nothing to read: skip the work, not just the result
    hpke_seal_team_reject(enc_out, ct, ct_cap, status + r, skip, lane, bc.nenc);
    return;
  }
  hpke_seal_team_wave<KDF, AEAD>(w.sbox, w.tbl, bc, eph_enc(bc, eph, r), eph_dh(bc, eph, n, r),
                                 PackedBytes{pts + p0, p1 - p0}, PackedBytes{aads + a0, a1 - a0},
                                 enc_out, ct, ct_cap, status + r, lane,
                                 bc.dh_ok ? bc.dh_ok[r] : 1u);
}

// One wave per report over the rows of a batch of Prio3 input shares to one aggregator, with
// k_hpke_seal_shares' arguments and contracts.  Report r's plaintext is the PlaintextInputShare of
// shares[r spitch ..] (slen bytes), its AAD the InputShareAad of (tid, rids[16 r ..], times[r],
// pubs[r pslen ..]); neither frame exists in memory.  Its enc goes to encs[r enc_pitch ..]
// (bc.nenc bytes) and its payload, exactly 6 + slen + 16 bytes, to payloads[r ppitch ..], at whatever
// alignment the columns have; nothing else of either buffer is written.
template <int KDF, int AEAD>
__global__ void __launch_bounds__(256) k_hpke_seal_team_shares(
    uint32_t n, HpkeBatchConsts bc, ReqTaskId tid, const uint32_t* eph, const uint8_t* rids,
    const uint64_t* times, const uint8_t* pubs, uint32_t pslen, const uint8_t* shares,
    uint32_t slen, uint64_t spitch, uint8_t* encs, uint64_t enc_pitch, uint8_t* payloads,
    uint64_t ppitch, uint8_t* status) {
  const TeamWave w = team_wave_setup<AEAD>();
  const uint32_t r = w.r, lane = w.lane;
  if (r >= n) return;
  uint8_t* enc_out = encs + (uint64_t)r * enc_pitch;
  uint8_t* ct = payloads + (uint64_t)r * ppitch;
  const uint64_t ct_cap = 6 + (uint64_t)slen + 16;
  if (status[r] != 0) {
    hpke_seal_team_reject(enc_out, ct, ct_cap, status + r, true, lane, bc.nenc);
    return;
  }
  const ReqAad aad{tid, rids + (size_t)r * 16, times[r], pslen, pubs + (size_t)r * pslen};
  hpke_seal_team_wave<KDF, AEAD>(w.sbox, w.tbl, bc, eph_enc(bc, eph, r), eph_dh(bc, eph, n, r),
                                 SharePlaintext{shares + (uint64_t)r * spitch, slen}, aad, enc_out,
                                 ct, ct_cap, status + r, lane, bc.dh_ok ? bc.dh_ok[r] : 1u);
}

}  // namespace p3g
