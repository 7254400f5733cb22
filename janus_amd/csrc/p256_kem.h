// The KEM half of DHKEM(P-256, HKDF-SHA256) (RFC 9180 §4.1) over p256.h, one lane of the DH
// kernels (hpke_dh_gpu.h: k_p256_dh, k_p256_dh_idx) and one lane of the sender's
// (hpke_dh_gpu.h: k_p256_eph, k_p256_eph_kem).  Free of HIP like p256.h; it hashes with
// sha256.h, device code in a HIP unit and host code in a plain C++ build
// (tests/native/p256_host.cpp, tests/native/p256_eph_host.cpp).
#pragma once
#include "p256.h"
#include "sha256.h"

#if defined(__HIPCC__)
#define P3G_P256_DEV __device__ __forceinline__
#else
#define P3G_P256_DEV inline
#endif

namespace p3g {

// ------------------------------------------------------------------------------------------------
// DHKEM(P-256, HKDF-SHA256) ExtractAndExpand (RFC 9180 §4.1), suite_id = "KEM" || 0x0010.
// Messages are built as big-endian words at compile-time byte offsets, as in hpke_kdf256.h.
// ------------------------------------------------------------------------------------------------
P3G_P256_DEV void p256_msg_byte(uint32_t* w, int off, uint32_t b) {
  w[off >> 2] |= b << (24 - 8 * (off & 3));
}
template <int N>
P3G_P256_DEV void p256_msg_str(uint32_t* w, int off, const char (&s)[N]) {
#pragma unroll
  for (int i = 0; i < N - 1; ++i) p256_msg_byte(w, off + i, (uint32_t)(uint8_t)s[i]);
}
P3G_P256_DEV void p256_msg_words8(uint32_t* w, int off, const uint32_t v[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int p = off + 4 * i, sh = 8 * (p & 3), idx = p >> 2;
    if (sh == 0) {
      w[idx] |= v[i];
    } else {
      w[idx] |= v[i] >> sh;
      w[idx + 1] |= v[i] << (32 - sh);
    }
  }
}
// "HPKE-v1" || "KEM" || 0x0010 at off (12 bytes)
P3G_P256_DEV void p256_msg_kem_prefix(uint32_t* w, int off) {
  p256_msg_str(w, off, "HPKE-v1");
  p256_msg_str(w, off + 7, "KEM");
  p256_msg_byte(w, off + 11, 0x10u);
}
// HMAC-SHA256 of the padded NB-block message w (consumed) after the pad states ist / ost
template <int NB>
P3G_P256_DEV void p256_hmac_finish(const uint32_t ist[8], const uint32_t ost[8], uint32_t* w,
                                   uint32_t out[8]) {
  uint32_t st[8], o[16];
#pragma unroll
  for (int i = 0; i < 8; ++i) st[i] = ist[i];
#pragma unroll
  for (int b = 0; b < NB; ++b) sha256_compress(st, w + 16 * b);
#pragma unroll
  for (int i = 0; i < 16; ++i) o[i] = i < 8 ? st[i] : 0u;
  o[8] = 0x80000000u;
  o[15] = (64 + 32) * 8;
#pragma unroll
  for (int i = 0; i < 8; ++i) out[i] = ost[i];
  sha256_compress(out, o);
}

// The recipient's public key as the kernels take it: the coordinates of pkRm, big-endian words.
struct P256PublicKey {
  uint32_t x[8], y[8];
};

// shared_secret (8 big-endian words) from dh (the x coordinate, 8 big-endian words), the lane's
// enc = 0x04 || ex || ey and pkRm = 0x04 || pk.x || pk.y.  salt0_i / salt0_o are the HMAC-SHA256
// pad states of the empty salt (HpkeBatchConsts).  kem_context is 130 bytes, so the expand's
// message is 158 bytes: three blocks behind the pad block.  8 compressions.
P3G_P256_DEV void p256_kem_shared_secret(const uint32_t salt0_i[8], const uint32_t salt0_o[8],
                                         const uint32_t dh[8], const uint32_t ex[8],
                                         const uint32_t ey[8], const P256PublicKey& pk,
                                         uint32_t ss[8]) {
  uint32_t w[48], prk[8], ist[8], ost[8];
  // eae_prk = LabeledExtract("", "eae_prk", dh)
#pragma unroll
  for (int i = 0; i < 16; ++i) w[i] = 0;
  p256_msg_kem_prefix(w, 0);
  p256_msg_str(w, 12, "eae_prk");
  p256_msg_words8(w, 19, dh);
  p256_msg_byte(w, 51, 0x80u);
  w[15] = (64 + 51) * 8;
  p256_hmac_finish<1>(salt0_i, salt0_o, w, prk);
  // shared_secret = LabeledExpand(eae_prk, "shared_secret", enc || pkRm, 32)
#pragma unroll
  for (int i = 0; i < 16; ++i) w[i] = (i < 8 ? prk[i] : 0u) ^ 0x36363636u;
  sha256_iv(ist);
  sha256_compress(ist, w);
#pragma unroll
  for (int i = 0; i < 16; ++i) w[i] = (i < 8 ? prk[i] : 0u) ^ 0x5c5c5c5cu;
  sha256_iv(ost);
  sha256_compress(ost, w);
#pragma unroll
  for (int i = 0; i < 48; ++i) w[i] = 0;
  p256_msg_byte(w, 1, 32u);
  p256_msg_kem_prefix(w, 2);
  p256_msg_str(w, 14, "shared_secret");
  p256_msg_byte(w, 27, 0x04u);
  p256_msg_words8(w, 28, ex);
  p256_msg_words8(w, 60, ey);
  p256_msg_byte(w, 92, 0x04u);
  p256_msg_words8(w, 93, pk.x);
  p256_msg_words8(w, 125, pk.y);
  p256_msg_byte(w, 157, 1u);
  p256_msg_byte(w, 158, 0x80u);
  w[47] = (64 + 158) * 8;
  p256_hmac_finish<3>(ist, ost, w, ss);
}

// One lane of the P-256 DH kernels: decode and validate the 65-byte enc, x([k] enc), the KEM
// half.  Returns the validity flag; an invalid enc runs the same instructions over the
// recipient's own (valid) point and its shared secret is zeroed.  raw (wave-uniform; the test
// hook's) leaves the KEM half out: ss is then x([k] enc) itself.
P3G_P256_DEV bool p256_dh_lane(const P256Scalar& k, const P256PublicKey& pk,
                               const uint32_t salt0_i[8], const uint32_t salt0_o[8],
                               const uint8_t* enc, bool present, bool raw, uint32_t ss[8]) {
  uint32_t ex[8], ey[8], dh[8];
  Fp256 X, Y;
  bool claim = false, ok = false;
  if (present) {
    p256_load_be_words8(enc + 1, ex);
    p256_load_be_words8(enc + 33, ey);
    claim = enc[0] == 0x04;
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) ex[i] = pk.x[i], ey[i] = pk.y[i];
  }
  // one copy of the validation's code: the second pass runs only for a refused enc, over pkRm
  // (validated on the host, so always a point)
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    const bool on = p256_validate(ex, ey, X, Y);
    if (pass == 0) ok = on & claim;
    if (ok) break;
#pragma unroll
    for (int i = 0; i < 8; ++i) ex[i] = pk.x[i], ey[i] = pk.y[i];
  }
  p256_dh_x(k, X, Y, dh);
  if (raw) {
#pragma unroll
    for (int i = 0; i < 8; ++i) ss[i] = dh[i];
  } else {
    p256_kem_shared_secret(salt0_i, salt0_o, dh, ex, ey, pk, ss);
  }
  const uint32_t m = ok ? 0xffffffffu : 0u;
#pragma unroll
  for (int i = 0; i < 8; ++i) ss[i] &= m;
  return ok;
}

// One lane of the sender's ladders (hpke_dh_gpu.h: k_p256_eph): (x, y)([sk_e] P) as big-endian
// words for the report's own ephemeral scalar sk_e (32 big-endian bytes, any alignment) and a valid
// point P = (X, Y), the generator (the encapsulated key) or the recipient's key (the DH value).
// Returns whether sk_e is in [1, n); a scalar outside runs the same instructions over 1 and both
// coordinates are zeroed, as p256_dh_lane does for a refused enc.
P3G_P256_DEV bool p256_eph_lane(const uint8_t* sk_e, const Fp256& X, const Fp256& Y,
                                uint32_t x_be[8], uint32_t y_be[8]) {
  P256LaneScalar k;
  const bool ok = p256_lane_scalar(sk_e, k);
  p256_mul_xy(k, X, Y, x_be, y_be);
  const uint32_t m = ok ? 0xffffffffu : 0u;
#pragma unroll
  for (int i = 0; i < 8; ++i) x_be[i] &= m, y_be[i] &= m;
  return ok;
}

// The sender's KEM half for one report (k_p256_eph_kem): the shared_secret from dh = x([sk_e] pkR)
// and enc = 0x04 || ex || ey = [sk_e] G, zeroed for a report whose scalar was refused.
P3G_P256_DEV void p256_eph_shared_secret(const uint32_t salt0_i[8], const uint32_t salt0_o[8],
                                         const uint32_t dh[8], const uint32_t ex[8],
                                         const uint32_t ey[8], const P256PublicKey& pk, bool ok,
                                         uint32_t ss[8]) {
  p256_kem_shared_secret(salt0_i, salt0_o, dh, ex, ey, pk, ss);
  const uint32_t m = ok ? 0xffffffffu : 0u;
#pragma unroll
  for (int i = 0; i < 8; ++i) ss[i] &= m;
}

}  // namespace p3g
