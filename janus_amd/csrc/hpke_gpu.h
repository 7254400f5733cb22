// Batched HPKE open on the GPU for DHKEM(X25519, HKDF-SHA256) and, behind the context's
// "hpke_gpu_p256" option, DHKEM(P-256, HKDF-SHA256) (p256.h) with every KDF and AEAD Janus
// accepts, RFC 9180 base mode, single shot: 0x0020 / 1 / 1 is the suite Janus generates by default
// (core/src/hpke.rs:204-231) and the helper opens once per report (aggregator.rs:1634-1700); the
// other eight (KDF HKDF-SHA256 / -SHA384 / -SHA512 x AEAD AES-128-GCM / AES-256-GCM /
// ChaCha20-Poly1305) are opened when the context's "hpke_gpu_suites" option is on.
// One lane per report, every report of a launch under ONE private key, hence one suite; the DH
// (hpke_dh_gpu.h's k_x25519 or k_p256_dh) has run before:
//   k_hpke_open<KDF, AEAD>  shared_secret, key schedule, the AEAD     RFC 9180 §4.1, §5.1;
//                                                     NIST SP 800-38D (GCM); RFC 8439 (ChaCha20)
// The kernel is a thin shell around a per-lane function (hpke_lane.h's hpke_open_lane over a byte
// source for the AAD) that helper_request.h's k_hpke_open_req calls too, with the request read in
// place.  Only the kernel and the test kernel are here: everything a lane computes is in headers
// free of HIP that CPU tests run as well.  Included by engine_hpke_team.hip alone.
#pragma once
#include "hpke_lane.h"
#include "x25519.h"

namespace p3g {

// One lane per report: hpke_open_lane over packed inputs, or zeros and status 4 when there is
// nothing to open (a short ciphertext, offsets that do not fit).  A report whose status is
// non-zero on entry keeps it and gets zeros.  Lanes have their own lengths; the only barrier is
// the one after the S-box is built, before any lane diverges (no S-box for ChaCha20-Poly1305).
template <int KDF, int AEAD>
__global__ void __launch_bounds__(256) k_hpke_open(
    uint32_t n, HpkeBatchConsts bc, const uint32_t* dh, const uint8_t* encs, const uint8_t* aads,
    const uint64_t* aad_off, uint64_t aad_total, const uint8_t* cts, const uint64_t* ct_off,
    uint64_t ct_total, uint8_t* pts, const uint64_t* pt_off, uint64_t pt_total, uint8_t* status) {
  const uint8_t* sbox = nullptr;
  if constexpr (AEAD != 3) {
    __shared__ uint8_t sbox_lds[256];
    aes_sbox_fill(sbox_lds, threadIdx.x, blockDim.x);
    __syncthreads();
    sbox = sbox_lds;
  }
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const uint64_t a0 = aad_off[r], a1 = aad_off[r + 1], c0 = ct_off[r], c1 = ct_off[r + 1];
  const uint64_t p0 = pt_off[r], p1 = pt_off[r + 1];
  const bool pt_fits = p0 <= p1 && p1 <= pt_total;
  const uint64_t pt_cap = pt_fits ? p1 - p0 : 0;
  uint8_t* pt = pts + p0;
  const bool skip = status[r] != 0;
  const bool ok = !skip && pt_fits && a0 <= a1 && a1 <= aad_total && c0 <= c1 && c1 <= ct_total &&
                  c1 - c0 >= 16 && c1 - c0 - 16 <= pt_cap;
  if (!ok) {  // nothing to read: skip the work, not just the result
    hpke_open_reject(pt, pt_cap, status + r, skip);
    return;
  }
  hpke_open_lane<KDF, AEAD>(sbox, bc, dh + (size_t)r * 8, bc.dh_ok ? bc.dh_ok[r] : 1u,
                            encs + (size_t)r * bc.nenc, PackedBytes{aads + a0, a1 - a0}, cts + c0,
                            c1 - c0 - 16, pt, pt_cap, status + r);
}

// TEST ONLY (prio3gpu_test_poly1305_gpu): tags[i] = Poly1305(keys[i], msgs[off[i] .. off[i + 1])),
// one lane per message, through hpke_prims.h's poly1305_mac.
__global__ void __launch_bounds__(64) k_test_poly1305(uint32_t n, const uint8_t* keys,
                                                      const uint8_t* msgs, const uint64_t* off,
                                                      uint8_t* tags) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t k[8], tag[4];
  load_le_words8(keys + (size_t)i * 32, k);
  poly1305_mac(k, msgs + off[i], off[i + 1] - off[i], tag);
#pragma unroll
  for (int j = 0; j < 16; ++j) tags[(size_t)i * 16 + j] = (uint8_t)(tag[j >> 2] >> (8 * (j & 3)));
}

}  // namespace p3g
