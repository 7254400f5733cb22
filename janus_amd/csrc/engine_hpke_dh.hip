// The launches of hpke_dh_gpu.h's kernels: the ladders that run before the AEAD kernels of every
// GPU HPKE call (hpke_launch.h).  A recipient's private key becomes a kernel argument here and
// nowhere else.
#include <hip/hip_runtime.h>

#include <cstring>

#include "hpke_launch.h"
#include "hpke_dh_gpu.h"

namespace p3g::eng {

namespace {

// launch(ks) with sk clamped (decodeScalar25519): the scalar travels as a kernel argument, so no
// device buffer ever holds the private key, and its host copy is wiped after the launch.
template <class F>
int with_clamped_scalar(const uint8_t* sk, F&& launch) {
  X25519Scalar ks;
  memcpy(ks.w, sk, 32);  // little-endian host
  ks.w[0] &= ~7u;
  ks.w[7] = (ks.w[7] & 0x7FFFFFFFu) | 0x40000000u;
  launch(ks);
  wipe(&ks, sizeof ks);
  HIPCHK(hipGetLastError());
  return 0;
}

// A P-256 batch's constants: the coordinates of pk (pkRm of an open, pkR of a seal) and the empty
// salt's pad states of bc.
P256DhConsts p256_dh_consts(const uint8_t* pk, const HpkeBatchConsts& bc) {
  P256DhConsts dc;
  p256_load_be_words8(pk + 1, dc.pk.x);
  p256_load_be_words8(pk + 33, dc.pk.y);
  memcpy(dc.salt0_i, bc.salt0_i, sizeof dc.salt0_i);
  memcpy(dc.salt0_o, bc.salt0_o, sizeof dc.salt0_o);
  return dc;
}

// launch(ks, dc) with sk as a P-256 scalar (little-endian words from the 32 big-endian bytes) and
// the batch's constants.  The keypair has passed p256_keypair_valid.  The scalar's host copy is
// wiped after the launch.
template <class F>
int with_p256_scalar(const uint8_t* sk, const uint8_t* pk, const HpkeBatchConsts& bc, F&& launch) {
  P256Scalar ks;
  for (int i = 0; i < 8; ++i)
    ks.w[i] = (uint32_t)sk[31 - 4 * i] | ((uint32_t)sk[30 - 4 * i] << 8) |
              ((uint32_t)sk[29 - 4 * i] << 16) | ((uint32_t)sk[28 - 4 * i] << 24);
  const P256DhConsts dc = p256_dh_consts(pk, bc);
  launch(ks, dc);
  wipe(&ks, sizeof ks);
  HIPCHK(hipGetLastError());
  return 0;
}

}  // namespace

int launch_x25519(prio3gpu_ctx* c, const uint8_t* sk, size_t n, const uint8_t* d_points,
                  uint32_t* d_out) {
  return with_clamped_scalar(sk, [&](const X25519Scalar& ks) {
    PROF(KID_X25519);
    hipLaunchKernelGGL(k_x25519, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c->stream,
                       (uint32_t)n, ks, d_points, d_out);
  });
}

int launch_x25519_idx(prio3gpu_ctx* c, const uint8_t* sk, size_t m, const uint32_t* d_idx,
                      const uint8_t* d_msg, const ReqView* d_views, uint32_t* d_dh) {
  return with_clamped_scalar(sk, [&](const X25519Scalar& ks) {
    PROF(KID_X25519_IDX);
    hipLaunchKernelGGL(k_x25519_idx, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, c->stream,
                       (uint32_t)m, ks, d_idx, d_msg, d_views, d_dh);
  });
}

int launch_p256_dh(prio3gpu_ctx* c, const uint8_t* sk, const uint8_t* pk,
                   const HpkeBatchConsts& bc, bool raw, size_t n, const uint8_t* d_points,
                   uint32_t* d_out, uint8_t* d_ok) {
  return with_p256_scalar(sk, pk, bc, [&](const P256Scalar& ks, const P256DhConsts& dc) {
    PROF(KID_P256_DH);
    hipLaunchKernelGGL(k_p256_dh, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c->stream,
                       (uint32_t)n, ks, dc, raw ? 1u : 0u, d_points, d_out, d_ok);
  });
}

int launch_p256_dh_idx(prio3gpu_ctx* c, const uint8_t* sk, const uint8_t* pk,
                       const HpkeBatchConsts& bc, size_t m, const uint32_t* d_idx,
                       const uint8_t* d_msg, const ReqView* d_views, uint32_t* d_ss,
                       uint8_t* d_ok) {
  return with_p256_scalar(sk, pk, bc, [&](const P256Scalar& ks, const P256DhConsts& dc) {
    PROF(KID_P256_DH_IDX);
    hipLaunchKernelGGL(k_p256_dh_idx, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, c->stream,
                       (uint32_t)m, ks, dc, d_idx, d_msg, d_views, d_ss, d_ok);
  });
}

int launch_x25519_eph(prio3gpu_ctx* c, const uint8_t* pk, size_t n, const uint8_t* d_sk,
                      uint32_t* d_eph) {
  X25519Point pkw;
  memcpy(pkw.w, pk, 32);  // little-endian host
  {
    PROF(KID_X25519_EPH);
    hipLaunchKernelGGL(k_x25519_eph, dim3((unsigned)((n + 63) / 64), 2), dim3(64), 0, c->stream,
                       (uint32_t)n, d_sk, pkw, d_eph);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

int launch_p256_eph(prio3gpu_ctx* c, const uint8_t* pk, size_t n, const uint8_t* d_sk,
                    uint32_t* d_eph, uint8_t* d_ok) {
  P256EphPoints pts;
  uint32_t x[8], y[8];
  if (!p256_decode(kP256G, x, y, pts.X[0], pts.Y[0]) ||
      !p256_decode(pk, x, y, pts.X[1], pts.Y[1])) {
    set_err("HPKE seal: the public key is not a P-256 point");
    return PRIO3GPU_E_HPKE;
  }
  {
    PROF(KID_P256_EPH);
    hipLaunchKernelGGL(k_p256_eph, dim3((unsigned)((n + 63) / 64), 2), dim3(64), 0, c->stream,
                       (uint32_t)n, d_sk, pts, d_eph, d_ok);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

int launch_p256_eph_kem(prio3gpu_ctx* c, const uint8_t* pk, const HpkeBatchConsts& bc, size_t n,
                        uint32_t* d_eph, const uint8_t* d_ok) {
  const P256DhConsts dc = p256_dh_consts(pk, bc);
  {
    PROF(KID_P256_EPH_KEM);
    hipLaunchKernelGGL(k_p256_eph_kem, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       c->stream, (uint32_t)n, dc, d_eph, d_ok);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

}  // namespace p3g::eng
