// Several WAVES per report for the share-row HPKE open and seal (the context's "hpke_team_split"
// option): small batches of very long input shares, where hpke_open_team.h's and hpke_seal_team.h's
// one wave per report leaves most of the chip idle.  The body (6 + share bytes) of every report is
// cut into S segments of L blocks (plan_hpke.h's team_split_plan; every report of a call has the
// same length, so one S and L per call) and three kernels run in stream order:
//   k_hpke_open_team_split / k_hpke_seal_team_split<KDF, AEAD>
//        n S waves, four to a block; wave i is segment s = i % S of report r = i / S.  It derives the
//        key, nonce, round keys and H^1 .. H^64 itself from the DH value, exactly as the one-wave
//        kernels do (registers, and the wave's LDS table, zeroed before the wave ends), runs its
//        blocks [s L, min((s + 1) L, nb)) with the body's own block indices, and writes the
//        segment's sum, carried to the segment's own end, to parts[r][s]: four words of GHASH or
//        five limbs of Poly1305.  Segment 0 alone absorbs the AAD, and in an open alone sees the
//        PlaintextInputShare's header: it writes flags[r].
//   k_hpke_open_team_join / k_hpke_seal_team_join<KDF, AEAD>
//        one wave per report, every lane alike: derives what the tag needs, folds the S sums
//        (gcm_split_join, poly_split_join) and computes the tag.  The seal stores the tag and the
//        enc, or zeros and status 4 as hpke_seal_team_reject does; the open compares the tag with
//        no early exit and sets status 4 (bad tag, all-zero DH value, invalid P-256 point) or 8
//        (an authentic plaintext with another header).
//   k_hpke_team_wipe (open only)
//        zeros over the whole share row of every report whose status is not zero.
// No wave waits for another: stream order between the kernels is the only synchronisation.  The
// opened rows hold unauthenticated plaintext between the first kernel and the third; the host
// queues all three back to back, so nothing queued later on the stream, and no copy-out, sees it.
// parts and flags are key-derived and the host's to zero (CallSecrets).  A report skipped on entry
// gets its slice zeroed by each of its waves, and so does a seal whose DH value is refused.
// Only the kernels are here; a lane's arithmetic is aes_gcm_team.h's and chacha_poly_team.h's,
// free of HIP and run by a CPU test (tests/native/team_split_host.cpp); the wave's place in its
// block (team_wave_setup, team_lds_sync, poly_team_sum) is hpke_team_wave.h's.  Included by
// engine_hpke_split.hip alone.
#pragma once
#include "hpke_team_wave.h"

namespace p3g {

constexpr uint32_t kSplitPartWords = 8;  // a segment's sum: parts[(r S + s) 8 ..], 4 or 5 used

// A wave's segment of its report: blocks [b0, b1) of nb.
struct SplitSeg {
  uint32_t r, s;
  uint64_t b0, b1;
};
__device__ __forceinline__ SplitSeg split_seg(uint32_t wave, uint32_t S, uint64_t L, uint64_t nb) {
  SplitSeg g;
  g.r = wave / S;
  g.s = wave % S;
  g.b0 = (uint64_t)g.s * L;
  g.b1 = g.b0 + L < nb ? g.b0 + L : nb;
  return g;
}

// The DH value and the enc of an open's report as the key schedule takes them: hpke_open_team_wave's
// first lines.  nz: zero when the DH failed.
__device__ __forceinline__ uint32_t split_open_dh(const HpkeBatchConsts& bc, const uint32_t* dh,
                                                  const uint8_t* enc, uint32_t dh_flag,
                                                  uint32_t dhw[8], uint32_t encw[8]) {
  uint32_t nz = 0;
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
  return nz;
}

// The same of a seal's report, from the ladders' words: hpke_seal_team_wave's first lines.  ence:
// the enc as it is stored.
__device__ __forceinline__ uint32_t split_seal_dh(const HpkeBatchConsts& bc, const uint32_t* enc,
                                                  const uint32_t* dh, uint32_t dh_flag,
                                                  uint32_t dhw[8], uint32_t encw[8],
                                                  uint32_t ence[8]) {
  uint32_t nz = 0;
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
  return nz;
}

// One segment after the key schedule's inputs are loaded: the key, the nonce, the AEAD's start,
// the wave's stripes over blocks [g.b0, g.b1) of the body src (src.len() bytes), and the segment's
// sum to part (lane 0 stores).  SEAL: src is the plaintext source and sink takes the ciphertext;
// else src is the ciphertext, a PackedBytes, and sink takes the plaintext.  tbl is zero when the
// call returns.
template <int KDF, int AEAD, bool SEAL, class Aad, class Src, class Sink>
__device__ __forceinline__ void split_segment(const uint8_t* sbox, uint32_t* tbl,
                                              const HpkeBatchConsts& bc, const uint32_t dhw[8],
                                              const uint32_t encw[8], const Aad& aad,
                                              const Src& src, const SplitSeg& g,
                                              uint32_t lane, Sink& sink, uint32_t* part) {
  constexpr int NKW = hpke_aead_nk(AEAD) / 4;
  uint32_t key[NKW], nonce[3];
  hpke_key_nonce<KDF, AEAD>(bc, dhw, encw, key, nonce);
  if constexpr (AEAD == 3) {
    uint32_t sum[5], ks[16];
#pragma unroll
    for (int i = 0; i < NKW; ++i) key[i] = bswap32(key[i]);
#pragma unroll
    for (int i = 0; i < 3; ++i) nonce[i] = bswap32(nonce[i]);
    const uint64_t c0 = g.b0 / 4, c1 = (g.b1 + 3) / 4;  // b0 is a multiple of 4 kTeam
    PolyTeam pt;
    chacha20_block(key, 0u, nonce, ks);
    poly_team_start_range(pt, ks, aad, g.s == 0, c0, c1, g.b1, lane, kTeam);
    chacha_team_stripe_range<SEAL>(pt, key, nonce, src, c0, c1, lane, kTeam, sink);
#pragma unroll
    for (int i = 0; i < 5; ++i) sum[i] = pt.mac.h[i];
    poly_team_sum(sum);
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < 5; ++i) part[i] = sum[i];
    }
  } else {
    uint32_t rk[4 * (NKW + 7)], h[4], y0[4], ctr[4];
    const FirstSegmentAad<Aad> seg_aad{aad, g.s == 0};
    aes_gcm_start<NKW>(sbox, key, nonce, seg_aad, rk, h, y0, ctr);
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) tbl[i] = h[i];
    }
    for (uint32_t half = 1; half < kTeam; half *= 2) {
      team_lds_sync();
      gf128_powers_step(tbl, lane, half);
    }
    team_lds_sync();
    uint32_t acc[4] = {0, 0, 0, 0};
    if constexpr (SEAL)
      gcm_team_seal_stripe_range<NKW>(sbox, rk, ctr, tbl, y0, src, g.b0, g.b1, lane, kTeam, acc,
                                      sink);
    else
      gcm_team_stripe_range<NKW, true, true>(sbox, rk, ctr, tbl, y0, src.p, src.n, g.b0, g.b1, lane,
                                             kTeam, acc, sink);
#pragma unroll
    for (int i = 0; i < 4; ++i) {  // the XOR of the 64 sums, on every lane
#pragma unroll
      for (int m = 1; m < (int)kTeam; m *= 2) acc[i] ^= (uint32_t)__shfl_xor((int)acc[i], m);
    }
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) part[i] = acc[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) tbl[4 * lane + i] = 0;
  }
}

// The tag of a report of `body` bytes under an AAD of alen bytes from its S segments' sums at
// parts, every lane alike: the key schedule again, then H and the tag mask, or r and s.  The AAD
// itself is not read (its hash is inside segment 0's sum).
template <int KDF, int AEAD>
__device__ __forceinline__ void split_join_tag(const uint8_t* sbox, const HpkeBatchConsts& bc,
                                               const uint32_t dhw[8], const uint32_t encw[8],
                                               uint64_t alen, uint64_t body, const uint32_t* parts,
                                               uint32_t S, uint64_t L, uint32_t t[4]) {
  constexpr int NKW = hpke_aead_nk(AEAD) / 4;
  const uint64_t nb = (body + 15) / 16;
  uint32_t key[NKW], nonce[3];
  hpke_key_nonce<KDF, AEAD>(bc, dhw, encw, key, nonce);
  if constexpr (AEAD == 3) {
    uint32_t ks[16], sum[5];
#pragma unroll
    for (int i = 0; i < NKW; ++i) key[i] = bswap32(key[i]);
#pragma unroll
    for (int i = 0; i < 3; ++i) nonce[i] = bswap32(nonce[i]);
    chacha20_block(key, 0u, nonce, ks);
    PolyTeam pt;
    poly1305_init(pt.mac, ks);
    poly_split_join(pt.mac.r, parts, kSplitPartWords, S, L, nb, sum);
    poly_team_tag(pt, sum, alen, body, t);
  } else {
    uint32_t rk[4 * (NKW + 7)], h[4], y0[4], ctr[4], y[4];
    aes_gcm_start<NKW>(sbox, key, nonce, PackedBytes{nullptr, 0}, rk, h, y0, ctr);
    gcm_split_join(h, parts, kSplitPartWords, S, L, nb, y);
    aes_gcm_tag<NKW>(sbox, rk, h, y, ctr, alen, body, t);
  }
}

// The open's segments over the columns k_hpke_open_team_shares takes (its arguments and layout):
// wave i < n S opens blocks [s L, ..) of report r's payload into its share row, without a verdict.
template <int KDF, int AEAD>
__global__ void __launch_bounds__(256) k_hpke_open_team_split(
    uint32_t n, uint32_t S, uint64_t L, HpkeBatchConsts bc, ReqTaskId tid, const uint32_t* dh,
    const uint8_t* rids, const uint64_t* times, const uint8_t* pubs, uint32_t pslen,
    const uint8_t* encs, uint64_t enc_pitch, const uint8_t* payloads, uint64_t ppitch,
    uint32_t slen, uint8_t* out, uint64_t spitch, const uint8_t* status, uint32_t* parts,
    uint8_t* flags) {
  const TeamWave w = team_wave_setup<AEAD>();
  const uint32_t lane = w.lane;
  if ((uint64_t)w.r >= (uint64_t)n * S) return;
  const uint64_t body = 6 + (uint64_t)slen, nb = (body + 15) / 16;
  const SplitSeg g = split_seg(w.r, S, L, nb);
  const uint32_t r = g.r;
  uint8_t* row = out + (uint64_t)r * spitch;
  if (status[r] != 0) {  // the segment's slice of the row: plaintext byte p is row[p - 6]
    const uint64_t p0 = 16 * g.b0 < 6 ? 6 : 16 * g.b0, p1 = 16 * g.b1 < body ? 16 * g.b1 : body;
    team_zero(row + (p0 - 6), p1 - p0, lane, kTeam);
    return;
  }
  const ReqAad aad{tid, rids + (size_t)r * 16, times[r], pslen, pubs + (size_t)r * pslen};
  ShareSink sink{row, slen, 0u};
  uint32_t dhw[8], encw[8];
  (void)split_open_dh(bc, dh + (size_t)r * 8, encs + (uint64_t)r * enc_pitch,
                      bc.dh_ok ? bc.dh_ok[r] : 1u, dhw, encw);
  const uint8_t* ct = payloads + (uint64_t)r * ppitch;
  split_segment<KDF, AEAD, false>(w.sbox, w.tbl, bc, dhw, encw, aad, PackedBytes{ct, body}, g,
                                  lane, sink, parts + ((size_t)r * S + g.s) * kSplitPartWords);
  if (g.s == 0 && lane == 0) flags[r] = sink.bad != 0u;  // block 0 is lane 0's
}

// The open's verdicts: a wave per report (every lane alike, lane 0 stores).
template <int KDF, int AEAD>
__global__ void __launch_bounds__(256) k_hpke_open_team_join(
    uint32_t n, uint32_t S, uint64_t L, HpkeBatchConsts bc, const uint32_t* dh,
    const uint8_t* encs, uint64_t enc_pitch, const uint8_t* payloads, uint64_t ppitch,
    uint32_t pslen, uint32_t slen, const uint32_t* parts, const uint8_t* flags, uint8_t* status) {
  const TeamWave w = team_wave_setup<AEAD>();
  const uint32_t r = w.r;
  if (r >= n || status[r] != 0) return;
  const uint64_t body = 6 + (uint64_t)slen;
  uint32_t dhw[8], encw[8], t[4], tag[4];
  const uint32_t nz = split_open_dh(bc, dh + (size_t)r * 8, encs + (uint64_t)r * enc_pitch,
                                    bc.dh_ok ? bc.dh_ok[r] : 1u, dhw, encw);
  split_join_tag<KDF, AEAD>(w.sbox, bc, dhw, encw, 60 + (uint64_t)pslen, body,
                            parts + (size_t)r * S * kSplitPartWords, S, L, t);
  load_block(payloads + (uint64_t)r * ppitch + body, 16, tag);
  uint32_t diff = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) diff |= t[i] ^ tag[i];  // no early exit
  const bool ok = diff == 0u && nz != 0u;
  if (w.lane == 0) {
    if (!ok) status[r] = ST_HPKE_DECRYPT;
    else if (flags[r]) status[r] = ST_INVALID_MESSAGE;
  }
}

// Zeros over the whole share row of every report whose status is not zero: grid (x, n), the x
// blocks of a row share its sixteen-byte pieces.
__global__ void __launch_bounds__(256) k_hpke_team_wipe(uint32_t n, uint8_t* out, uint64_t spitch,
                                                        uint32_t slen, const uint8_t* status) {
  const uint32_t r = blockIdx.y;
  if (r >= n || status[r] == 0) return;
  team_zero(out + (uint64_t)r * spitch, slen, blockIdx.x * blockDim.x + threadIdx.x,
            gridDim.x * blockDim.x);
}

// The seal's segments over the rows k_hpke_seal_team_shares takes (its arguments and layout): wave
// i < n S seals blocks [s L, ..) of report r's PlaintextInputShare into its payload.
template <int KDF, int AEAD>
__global__ void __launch_bounds__(256) k_hpke_seal_team_split(
    uint32_t n, uint32_t S, uint64_t L, HpkeBatchConsts bc, ReqTaskId tid, const uint32_t* eph,
    const uint8_t* rids, const uint64_t* times, const uint8_t* pubs, uint32_t pslen,
    const uint8_t* shares, uint32_t slen, uint64_t spitch, uint8_t* payloads, uint64_t ppitch,
    const uint8_t* status, uint32_t* parts) {
  const TeamWave w = team_wave_setup<AEAD>();
  const uint32_t lane = w.lane;
  if ((uint64_t)w.r >= (uint64_t)n * S) return;
  const uint64_t body = 6 + (uint64_t)slen, nb = (body + 15) / 16;
  const SplitSeg g = split_seg(w.r, S, L, nb);
  const uint32_t r = g.r;
  uint8_t* ct = payloads + (uint64_t)r * ppitch;
  const uint64_t p0 = 16 * g.b0, p1 = 16 * g.b1 < body ? 16 * g.b1 : body;  // the segment's slice
  uint32_t dhw[8], encw[8], ence[8];
  const uint32_t nz = status[r] != 0 ? 0u
                                      : split_seal_dh(bc, eph_enc(bc, eph, r), eph_dh(bc, eph, n, r),
                                                      bc.dh_ok ? bc.dh_ok[r] : 1u, dhw, encw, ence);
  if (nz == 0u) {  // skipped on entry, or the DH refused: alike on every lane of the wave
    team_zero(ct + p0, p1 - p0, lane, kTeam);
    return;
  }
  const ReqAad aad{tid, rids + (size_t)r * 16, times[r], pslen, pubs + (size_t)r * pslen};
  const SharePlaintext pt{shares + (uint64_t)r * spitch, slen};
  CtSink sink{ct};
  split_segment<KDF, AEAD, true>(w.sbox, w.tbl, bc, dhw, encw, aad, pt, g, lane, sink,
                                 parts + ((size_t)r * S + g.s) * kSplitPartWords);
}

// The seal's tags and encs: a wave per report.  A report skipped on entry gets zeros in its enc
// and tag; one whose DH value is refused the same and status 4 (what hpke_seal_team.h's
// hpke_seal_team_reject does, whose ciphertext part the segments' waves have done).
template <int KDF, int AEAD>
__global__ void __launch_bounds__(256) k_hpke_seal_team_join(
    uint32_t n, uint32_t S, uint64_t L, HpkeBatchConsts bc, const uint32_t* eph, uint32_t pslen,
    uint32_t slen, const uint32_t* parts, uint8_t* encs, uint64_t enc_pitch, uint8_t* payloads,
    uint64_t ppitch, uint8_t* status) {
  const TeamWave w = team_wave_setup<AEAD>();
  const uint32_t r = w.r, lane = w.lane;
  if (r >= n) return;
  const uint64_t body = 6 + (uint64_t)slen;
  uint8_t* enc_out = encs + (uint64_t)r * enc_pitch;
  uint8_t* ct = payloads + (uint64_t)r * ppitch;
  const bool skip = status[r] != 0;
  const uint32_t* enc = eph_enc(bc, eph, r);
  uint32_t dhw[8], encw[8], ence[8], t[4];
  const uint32_t nz = skip ? 0u
                           : split_seal_dh(bc, enc, eph_dh(bc, eph, n, r),
                                           bc.dh_ok ? bc.dh_ok[r] : 1u, dhw, encw, ence);
  if (nz == 0u) {
    team_zero(enc_out, bc.nenc, lane, kTeam);
    team_zero(ct + body, 16, lane, kTeam);
    if (!skip && lane == 0) status[r] = ST_HPKE_DECRYPT;
    return;
  }
  split_join_tag<KDF, AEAD>(w.sbox, bc, dhw, encw, 60 + (uint64_t)pslen, body,
                            parts + (size_t)r * S * kSplitPartWords, S, L, t);
  if (lane == 0) store_block_any(ct + body, t);
  if (bc.dh_ok) {  // enc: 0x04, then a byte of x || y from each lane
    if (lane == 0) enc_out[0] = 0x04;
    enc_out[1 + lane] = reinterpret_cast<const uint8_t*>(enc)[lane];
  } else if (lane < 2) {  // enc: sixteen bytes from each of two lanes
    uint32_t e[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) e[i] = lane ? ence[4 + i] : ence[i];
    store_block_any(enc_out + 16 * lane, e);
  }
}

}  // namespace p3g
