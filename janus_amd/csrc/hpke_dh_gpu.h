// The Diffie-Hellman kernels of the GPU HPKE paths, one lane per report (and, for a seal's two
// ladders, per point): DHKEM(X25519, HKDF-SHA256) and, behind the context's "hpke_gpu_p256" option,
// DHKEM(P-256, HKDF-SHA256).  They run before the AEAD kernels of a call and leave what those read:
//   k_x25519          dh = X25519(skR, enc), packed encs                       RFC 7748 §5
//   k_x25519_idx      the same over a key group of a request, enc read in place
//   k_p256_dh         x([skR] enc), validity flag, shared_secret                RFC 9180 §4.1, §7.1
//   k_p256_dh_idx     the same over a key group of a request, enc read in place
//   k_x25519_eph      enc = X25519(skE, 9), dh = X25519(skE, pkR)               RFC 9180 §4.1
//   k_p256_eph        enc = [skE] G, dh = x([skE] pkR), the scalar's validity   §7.1
//   k_p256_eph_kem    dh -> shared_secret (ExtractAndExpand over enc || pkR)    §4.1
// Each kernel is a thin shell around a per-lane function (x25519.h's x25519_lane, p256_kem.h's
// p256_dh_lane, p256_eph_lane and p256_eph_shared_secret), in headers free of HIP that CPU tests
// run as well.  The two ladders of a sealed report run on two lanes of one launch (blockIdx.y
// picks the point), each the unchanged lane with its own scalar: one ladder's registers per lane,
// no scratch, and twice the lanes for the latency-bound field arithmetic to hide behind.  A
// recipient's private key is a kernel argument: no device buffer ever holds it.  Included by
// engine_hpke_dh.hip alone, after include/prio3gpu.h.
#pragma once
#include "hpke_kernel_args.h"

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

// dh[idx[j]] = X25519(k, enc of report idx[j]) for the m reports of a key group.  A report whose
// encapsulated key is not 32 bytes is not read (k_hpke_open_req rejects it); its lane runs the
// ladder over zeros like an idle lane.
__global__ void __launch_bounds__(64) k_x25519_idx(uint32_t m, X25519Scalar k, const uint32_t* idx,
                                                   const uint8_t* msg, const ReqView* views,
                                                   uint32_t* dh) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = j < m;
  const uint32_t r = idx[live ? j : m - 1];
  const ReqView& v = views[r];
  uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (v.enc_len == 32) load_le_words8(msg + v.enc_off, w);
  x25519_lane(k, w);
  if (live) {
#pragma unroll
    for (int i = 0; i < 8; ++i) dh[(size_t)r * 8 + i] = w[i];
  }
}

// ss[idx[j]] = the P-256 shared_secret of (k, enc of report idx[j]) and ok[idx[j]] = 1 for the m
// reports of a key group; zeros and 0 for an enc DeserializePublicKey refuses or whose length is
// not 65 (not read: k_hpke_open_req rejects that one by its length).
__global__ void __launch_bounds__(64) k_p256_dh_idx(uint32_t m, P256Scalar k, P256DhConsts dc,
                                                    const uint32_t* idx, const uint8_t* msg,
                                                    const ReqView* views, uint32_t* ss,
                                                    uint8_t* ok) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = j < m;
  const uint32_t r = idx[live ? j : m - 1];
  const ReqView& v = views[r];
  uint32_t w[8];
  const bool good = p256_lane_out(k, dc, 0u, msg + v.enc_off, v.enc_len == 65, w);
  if (live) {
#pragma unroll
    for (int i = 0; i < 8; ++i) ss[(size_t)r * 8 + i] = w[i];
    ok[r] = good ? 1 : 0;
  }
}

// out[which n 8 + r 8 ..] = X25519(sk_es[r], which ? pkR : 9) as 8 little-endian words:
// blockIdx.y = 0 the encapsulated keys, 1 the DH values.  The scalar is clamped here
// (decodeScalar25519); its bits are read with selects inside x25519_lane, so no branch and no
// address depends on it or on a field value.
__global__ void __launch_bounds__(64) k_x25519_eph(uint32_t n, const uint8_t* sk_es,
                                                   X25519Point pk, uint32_t* out) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t which = blockIdx.y;
  const bool live = r < n;
  X25519Scalar k;
  load_le_words8(sk_es + (size_t)(live ? r : n - 1) * 32, k.w);
  k.w[0] &= ~7u;
  k.w[7] = (k.w[7] & 0x7FFFFFFFu) | 0x40000000u;
  uint32_t w[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = which ? pk.w[i] : (i ? 0u : 9u);
  x25519_lane(k, w);
  if (live) {
    uint32_t* o = out + ((size_t)which * n + r) * 8;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = w[i];
  }
}

// The P-256 counterpart of k_x25519_eph: blockIdx.y = 0 the encapsulated keys [sk_es[r]] G (both
// coordinates, and the report's validity byte), 1 the DH values x([sk_es[r]] pkR).  ONE ladder:
// the point comes from selects on blockIdx.y.  The scalar is the lane's own (p256_eph_lane): its
// bits are select masks only, no branch and no address depends on it; a scalar outside [1, n)
// runs the same instructions and leaves zeros and ok = 0.
__global__ void __launch_bounds__(64) k_p256_eph(uint32_t n, const uint8_t* sk_es,
                                                 P256EphPoints pts, uint32_t* out, uint8_t* ok) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t which = blockIdx.y;
  const bool live = r < n;
  Fp256 X, Y;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    X.v[i] = which ? pts.X[1].v[i] : pts.X[0].v[i];
    Y.v[i] = which ? pts.Y[1].v[i] : pts.Y[0].v[i];
  }
  uint32_t x[8], y[8];
  const bool good = p256_eph_lane(sk_es + (size_t)(live ? r : n - 1) * 32, X, Y, x, y);
  if (!live) return;
  if (which == 0) {
    uint32_t* o = out + (size_t)r * 16;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = bswap32(x[i]), o[8 + i] = bswap32(y[i]);
    ok[r] = good ? 1 : 0;
  } else {
    uint32_t* o = out + (size_t)n * 16 + (size_t)r * 8;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = bswap32(x[i]);
  }
}

// The KEM half after k_p256_eph, one lane per report: eph's DH value becomes the shared_secret in
// place (zeros for a report whose ok byte is 0).
__global__ void __launch_bounds__(256) k_p256_eph_kem(uint32_t n, P256DhConsts dc, uint32_t* eph,
                                                      const uint8_t* ok) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  uint32_t ex[8], ey[8], dh[8], ss[8];
  uint32_t* d = eph + (size_t)n * 16 + (size_t)r * 8;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    ex[i] = bswap32(eph[(size_t)r * 16 + i]);
    ey[i] = bswap32(eph[(size_t)r * 16 + 8 + i]);
    dh[i] = bswap32(d[i]);
  }
  p256_eph_shared_secret(dc.salt0_i, dc.salt0_o, dh, ex, ey, dc.pk, ok[r] != 0, ss);
#pragma unroll
  for (int i = 0; i < 8; ++i) d[i] = bswap32(ss[i]);
}

}  // namespace p3g
