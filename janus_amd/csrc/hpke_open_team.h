// Batched HPKE open of long ciphertexts on the GPU, one WAVE per report: DHKEM(X25519,
// HKDF-SHA256) (and DHKEM(P-256, HKDF-SHA256) behind the context's "hpke_gpu_p256" option, after
// hpke_dh_gpu.h's k_p256_dh) with HKDF-SHA256 / -SHA384 / -SHA512 and AES-128-GCM / AES-256-GCM /
// ChaCha20-Poly1305, RFC 9180 base mode, single shot.  What the leader does once per upload (aggregator.rs:1325-1497) with an input
// share of a hundred kilobytes, where hpke_gpu.h's lane per report would walk it alone:
//   k_hpke_open_team<KDF, AEAD>          packed inputs with offsets, as k_hpke_open takes them
//   k_hpke_open_team_shares<KDF, AEAD>   enc and payload columns in, Prio3 input-share rows out: the
//                                        InputShareAad is a byte source over the caller's rows and
//                                        the PlaintextInputShare's header is checked, not stored
// The DH is hpke_dh_gpu.h's k_x25519, one lane per report, launched before.  Four reports per
// block; the only block barrier is the one after the S-box build (reports differ in length).  How
// a wave opens its report, and what crosses its lanes, is hpke_team_wave.h's.  Only the kernels are
// here.  Included by engine_hpke_team.hip alone.
#pragma once
#include "hpke_team_wave.h"

namespace p3g {

// One wave per report over packed inputs, with k_hpke_open's arguments and contracts: report r's
// plaintext goes to pts[pt_off[r] ..] and zeros up to pt_off[r + 1]; zeros in the whole slot and
// status 4 for a tag that does not match, an all-zero DH value, a ciphertext shorter than 16 bytes,
// a slot shorter than the plaintext or offsets that do not fit.  A report whose status is non-zero
// on entry keeps it and gets zeros.
template <int KDF, int AEAD>
__global__ void __launch_bounds__(256) k_hpke_open_team(
    uint32_t n, HpkeBatchConsts bc, const uint32_t* dh, const uint8_t* encs, const uint8_t* aads,
    const uint64_t* aad_off, uint64_t aad_total, const uint8_t* cts, const uint64_t* ct_off,
    uint64_t ct_total, uint8_t* pts, const uint64_t* pt_off, uint64_t pt_total, uint8_t* status) {
  const TeamWave w = team_wave_setup<AEAD>();
  const uint32_t r = w.r, lane = w.lane;
  if (r >= n) return;
  const uint64_t a0 = aad_off[r], a1 = aad_off[r + 1], c0 = ct_off[r], c1 = ct_off[r + 1];
  const uint64_t p0 = pt_off[r], p1 = pt_off[r + 1];
  const bool pt_fits = p0 <= p1 && p1 <= pt_total;
  const uint64_t pt_cap = pt_fits ? p1 - p0 : 0;
  uint8_t* pt = pts + (pt_fits ? p0 : 0);
  const bool skip = status[r] != 0;
  const bool fits = !skip && pt_fits && a0 <= a1 && a1 <= aad_total && c0 <= c1 &&
                    c1 <= ct_total && c1 - c0 >= 16 && c1 - c0 - 16 <= pt_cap;
  if (!fits) {  // nothing to read: skip the work, not just the result
    team_zero(pt, pt_cap, lane, kTeam);
    if (!skip && lane == 0) status[r] = ST_HPKE_DECRYPT;
    return;
  }
  const uint64_t body = c1 - c0 - 16;
  PackedSink sink{pt};
  const bool ok = hpke_open_team_wave<KDF, AEAD>(w.sbox, w.tbl, bc, dh + (size_t)r * 8,
                                                 encs + (size_t)r * bc.nenc,
                                                 PackedBytes{aads + a0, a1 - a0}, cts + c0, body,
                                                 lane, sink, bc.dh_ok ? bc.dh_ok[r] : 1u);
  team_zero(pt + body, pt_cap - body, lane, kTeam);
  if (!ok && lane == 0) status[r] = ST_HPKE_DECRYPT;
}

// One wave per report over the columns of a batch of uploads to one aggregator: report r's enc is
// encs[r enc_pitch ..] (bc.nenc bytes; not read for P-256), its payload payloads[r ppitch ..], exactly 6 + slen + 16 bytes,
// its AAD the InputShareAad of (tid, rids[16 r ..], times[r], pubs[r pslen ..]), never built in
// memory.  The plaintext must be 00 00 | u32 BE slen | share: the share goes to
// out[r spitch .. + slen) and nothing else of out is written.  Zeros in the row and status 4 for
// a failed open; zeros and status 8 for an authentic plaintext with another header (extensions,
// or another length: at this ciphertext length either leaves a share of the wrong size).  A report
// whose status is non-zero on entry keeps it and gets zeros.
template <int KDF, int AEAD>
__global__ void __launch_bounds__(256) k_hpke_open_team_shares(
    uint32_t n, HpkeBatchConsts bc, ReqTaskId tid, const uint32_t* dh, const uint8_t* rids,
    const uint64_t* times, const uint8_t* pubs, uint32_t pslen, const uint8_t* encs,
    uint64_t enc_pitch, const uint8_t* payloads, uint64_t ppitch, uint32_t slen, uint8_t* out,
    uint64_t spitch, uint8_t* status) {
  const TeamWave w = team_wave_setup<AEAD>();
  const uint32_t r = w.r, lane = w.lane;
  if (r >= n) return;
  uint8_t* row = out + (uint64_t)r * spitch;
  if (status[r] != 0) {
    team_zero(row, slen, lane, kTeam);
    return;
  }
  const ReqAad aad{tid, rids + (size_t)r * 16, times[r], pslen, pubs + (size_t)r * pslen};
  ShareSink sink{row, slen, 0u};
  const bool ok = hpke_open_team_wave<KDF, AEAD>(w.sbox, w.tbl, bc, dh + (size_t)r * 8,
                                                 encs + (uint64_t)r * enc_pitch, aad,
                                                 payloads + (uint64_t)r * ppitch,
                                                 6 + (uint64_t)slen, lane, sink,
                                                 bc.dh_ok ? bc.dh_ok[r] : 1u);
  if (!ok) {
    if (lane == 0) status[r] = ST_HPKE_DECRYPT;
    return;
  }
  const uint32_t bad = (uint32_t)__shfl((int)sink.bad, 0);  // block 0 is lane 0's
  if (bad) {
    team_wipe<AEAD>(sink, 6 + (uint64_t)slen, lane);
    if (lane == 0) status[r] = ST_INVALID_MESSAGE;
  }
}

}  // namespace p3g
