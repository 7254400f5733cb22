// Batched HPKE seal on the GPU for DHKEM(X25519, HKDF-SHA256) and, behind the context's
// "hpke_gpu_p256" option, DHKEM(P-256, HKDF-SHA256) with every KDF and AEAD Janus accepts
// (KDF 1-3 x AEAD 1-3), RFC 9180 base mode, single shot: what a DAP client does once per input
// share (client/src/lib.rs:212-258, core/src/hpke.rs:158-182).  The mirror image of hpke_gpu.h's
// open, one lane per report, every report of a launch to ONE recipient key, each under its own
// ephemeral key, whose ladders (hpke_dh_gpu.h's k_x25519_eph, or k_p256_eph and k_p256_eph_kem)
// have run before:
//   k_hpke_seal<KDF, AEAD>     key schedule + AEAD encryption over packed plaintexts and AADs
//   k_hpke_seal_shares<KDF, AEAD>   the same over Prio3 input shares: the PlaintextInputShare and
//                              the InputShareAad are byte sources over the caller's rows and are
//                              never written to memory
// Only the kernels are here: the lane (hpke_seal_lane) and the two byte sources (SharePlaintext,
// ReqAad) are hpke_lane.h's, free of HIP and run by CPU tests too.  Included by
// engine_hpke_seal.hip alone.
#pragma once
#include "hpke_lane.h"

namespace p3g {

// One lane per report: hpke_seal_lane over packed plaintexts and AADs; report r's ciphertext ||
// tag goes to cts[ct_off[r] .. ct_off[r + 1]) and its enc to encs[bc.nenc r ..].  A slot shorter than
// the plaintext + 16 or offsets that do not fit: zeros and status 4.  A report whose status is
// non-zero on entry keeps it and gets zeros.  `eph` is k_x25519_eph's output (n encs, then n DH
// values) or, with bc.dh_ok set, k_p256_eph's and k_p256_eph_kem's.  Lanes have their own lengths; the only barrier is the one after the S-box is built,
// before any lane diverges (no S-box for ChaCha20-Poly1305).
template <int KDF, int AEAD>
__global__ void __launch_bounds__(256) k_hpke_seal(
    uint32_t n, HpkeBatchConsts bc, const uint32_t* eph, const uint8_t* aads,
    const uint64_t* aad_off, uint64_t aad_total, const uint8_t* pts, const uint64_t* pt_off,
    uint64_t pt_total, uint8_t* encs, uint8_t* cts, const uint64_t* ct_off, uint64_t ct_total,
    uint8_t* status) {
  const uint8_t* sbox = nullptr;
  if constexpr (AEAD != 3) {
    __shared__ uint8_t sbox_lds[256];
    aes_sbox_fill(sbox_lds, threadIdx.x, blockDim.x);
    __syncthreads();
    sbox = sbox_lds;
  }
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
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
    hpke_seal_reject(enc_out, ct, ct_cap, status + r, skip, bc.nenc);
    return;
  }
  hpke_seal_lane<KDF, AEAD>(sbox, bc, eph_enc(bc, eph, r), eph_dh(bc, eph, n, r),
                            PackedBytes{pts + p0, p1 - p0}, PackedBytes{aads + a0, a1 - a0},
                            enc_out, ct, ct_cap, status + r, bc.dh_ok ? bc.dh_ok[r] : 1u);
}

// One lane per report: hpke_seal_lane over the rows of a batch of Prio3 input shares to one
// aggregator.  Report r's plaintext is the PlaintextInputShare of shares[r spitch ..] (slen bytes),
// its AAD the InputShareAad of (tid, rids[16 r ..], times[r], pubs[r pslen ..]); neither frame
// exists in memory.  Its enc goes to encs[r enc_pitch ..] (bc.nenc bytes) and its payload, exactly
// 6 + slen + 16 bytes, to payloads[r ppitch ..]; nothing else of either buffer is written.
template <int KDF, int AEAD>
__global__ void __launch_bounds__(256) k_hpke_seal_shares(
    uint32_t n, HpkeBatchConsts bc, ReqTaskId tid, const uint32_t* eph, const uint8_t* rids,
    const uint64_t* times, const uint8_t* pubs, uint32_t pslen, const uint8_t* shares,
    uint32_t slen, uint64_t spitch, uint8_t* encs, uint64_t enc_pitch, uint8_t* payloads,
    uint64_t ppitch, uint8_t* status) {
  const uint8_t* sbox = nullptr;
  if constexpr (AEAD != 3) {
    __shared__ uint8_t sbox_lds[256];
    aes_sbox_fill(sbox_lds, threadIdx.x, blockDim.x);
    __syncthreads();
    sbox = sbox_lds;
  }
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  uint8_t* enc_out = encs + (uint64_t)r * enc_pitch;
  uint8_t* ct = payloads + (uint64_t)r * ppitch;
  const uint64_t ct_cap = 6 + (uint64_t)slen + 16;
  if (status[r] != 0) {
    hpke_seal_reject(enc_out, ct, ct_cap, status + r, true, bc.nenc);
    return;
  }
  const ReqAad aad{tid, rids + (size_t)r * 16, times[r], pslen, pubs + (size_t)r * pslen};
  hpke_seal_lane<KDF, AEAD>(sbox, bc, eph_enc(bc, eph, r), eph_dh(bc, eph, n, r),
                            SharePlaintext{shares + (uint64_t)r * spitch, slen}, aad, enc_out, ct,
                            ct_cap, status + r, bc.dh_ok ? bc.dh_ok[r] : 1u);
}

}  // namespace p3g
