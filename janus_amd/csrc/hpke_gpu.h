// Batched HPKE open on the GPU for DHKEM(X25519, HKDF-SHA256) and, behind the context's
// "hpke_gpu_p256" option, DHKEM(P-256, HKDF-SHA256) (p256.h) with every KDF and AEAD Janus
// accepts, RFC 9180 base mode, single shot: 0x0020 / 1 / 1 is the suite Janus generates by default
// (core/src/hpke.rs:204-231) and the helper opens once per report (aggregator.rs:1634-1700); the
// other eight (KDF HKDF-SHA256 / -SHA384 / -SHA512 x AEAD AES-128-GCM / AES-256-GCM /
// ChaCha20-Poly1305) are opened when the context's "hpke_gpu_suites" option is on.
// One lane per report, every report of a launch under ONE private key, hence one suite:
//   k_x25519                dh = X25519(skR, enc)                     RFC 7748 §5
//   k_p256_dh               x([skR] enc), validity flag, shared_secret RFC 9180 §4.1, §7.1
//   k_hpke_open<KDF, AEAD>  shared_secret, key schedule, the AEAD     RFC 9180 §4.1, §5.1;
//                                                     NIST SP 800-38D (GCM); RFC 8439 (ChaCha20)
// Each kernel is a thin shell around a per-lane function (x25519.h's x25519_lane, p256_kem.h's
// p256_dh_lane, hpke_lane.h's hpke_open_lane over a byte source for the AAD) that
// helper_request.h's kernels call too, with the request read in place.  Only the kernels, their
// argument structs and the test kernel are here: everything a lane computes is in headers free of
// HIP that CPU tests run as well.  Included by engine_hpke.hip.
#pragma once
#include "hpke_lane.h"
#include "p256_kem.h"
#include "x25519.h"

namespace p3g {

// out[r] = X25519(k, points[r]), one lane per point.
__global__ void __launch_bounds__(64) k_x25519(uint32_t n, X25519Scalar k, const uint8_t* points,
                                               uint32_t* out) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = r < n;
  uint32_t w[8];
  load_le_words8(points + (size_t)(live ? r : n - 1) * 32, w);
  x25519_lane(k, w);
  if (live) {
#pragma unroll
    for (int i = 0; i < 8; ++i) out[(size_t)r * 8 + i] = w[i];
  }
}

// The batch-shared inputs of the P-256 DH kernels: pkRm's coordinates and the HMAC-SHA256 pad
// states of the empty salt (the KEM half runs in the DH kernel).
struct P256DhConsts {
  P256PublicKey pk;
  uint32_t salt0_i[8], salt0_o[8];
};

// One lane of k_p256_dh / k_p256_dh_idx: p256_dh_lane over enc (65 bytes, read only if present).
// out gets 32 bytes as 8 words, zero for a refused enc: the shared_secret, or with raw set
// (prio3gpu_test_p256_gpu) the big-endian x coordinate of [k] enc itself.
DEVI bool p256_lane_out(const P256Scalar& k, const P256DhConsts& dc, uint32_t raw,
                        const uint8_t* enc, bool present, uint32_t out[8]) {
  uint32_t ss[8];
  const bool ok = p256_dh_lane(k, dc.pk, dc.salt0_i, dc.salt0_o, enc, present, raw != 0u, ss);
#pragma unroll
  for (int i = 0; i < 8; ++i) out[i] = bswap32(ss[i]);
  return ok;
}

// out[r] = the shared_secret of (k, points[r]) and ok[r] = 1, or zeros and ok[r] = 0 for an
// encoding DeserializePublicKey refuses; one lane per packed 65-byte point.  The scalar is a
// kernel argument: no device buffer ever holds the private key.
__global__ void __launch_bounds__(64) k_p256_dh(uint32_t n, P256Scalar k, P256DhConsts dc,
                                                uint32_t raw, const uint8_t* points, uint32_t* out,
                                                uint8_t* ok) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = r < n;
  uint32_t w[8];
  const bool good = p256_lane_out(k, dc, raw, points + (size_t)(live ? r : n - 1) * 65, true, w);
  if (live) {
#pragma unroll
    for (int i = 0; i < 8; ++i) out[(size_t)r * 8 + i] = w[i];
    ok[r] = good ? 1 : 0;
  }
}

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
