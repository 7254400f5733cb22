// HKDF-SHA256 for one lane of the GPU HPKE open and seal: HMAC-SHA256 over fixed-layout messages
// and, on top of it, (dh, enc) -> (AEAD key, base nonce) for every suite: the DHKEM's
// ExtractAndExpand (RFC 9180 §4.1) and KeySchedule(mode_base) (§5.1).  KDF 1 (HKDF-SHA256, the
// suite Janus generates by default) is all here; KDF 2 / 3 hand the suite half to hpke_prims.h's
// hpke_kdf512_key_nonce.  Free of HIP like hpke_prims.h: the kernels and a CPU test
// (tests/native/hpke_lane_host.cpp) run the same text.
#pragma once
#include "hpke_prims.h"
#include "hpke_shared.h"
#include "sha256.h"

namespace p3g {

// ------------------------------------------------------------------------------------------------
// HMAC-SHA256 over fixed-layout messages.  A message is built in registers as big-endian words at
// compile-time byte offsets (constant bytes fold into the schedule); sha256_compress does the rest.
// ------------------------------------------------------------------------------------------------
DEVI void msg_byte(uint32_t* w, int off, uint32_t b) { w[off >> 2] |= b << (24 - 8 * (off & 3)); }

template <int N>
DEVI void msg_str(uint32_t* w, int off, const char (&s)[N]) {  // the N - 1 characters of s
#pragma unroll
  for (int i = 0; i < N - 1; ++i) msg_byte(w, off + i, (uint32_t)(uint8_t)s[i]);
}

DEVI void msg_words8(uint32_t* w, int off, const uint32_t v[8]) {  // 32 bytes as 8 BE words
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

// SHA-256 padding of a `len`-byte message that follows one 64-byte (HMAC pad) block.
DEVI void msg_pad(uint32_t* w, int len, int nblk) {
  msg_byte(w, len, 0x80u);
  w[16 * nblk - 1] = (uint32_t)(64 + len) * 8u;
}

DEVI void hmac_pads(const uint32_t key[8], uint32_t ist[8], uint32_t ost[8]) {  // 32-byte key
  uint32_t w[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) w[i] = (i < 8 ? key[i] : 0u) ^ 0x36363636u;
  sha256_iv(ist);
  sha256_compress(ist, w);
#pragma unroll
  for (int i = 0; i < 16; ++i) w[i] = (i < 8 ? key[i] : 0u) ^ 0x5c5c5c5cu;
  sha256_iv(ost);
  sha256_compress(ost, w);
}

// HMAC of the padded NB-block message w (consumed) under the key whose pad states are ist / ost.
template <int NB>
DEVI void hmac_finish(const uint32_t ist[8], const uint32_t ost[8], uint32_t* w, uint32_t out[8]) {
  uint32_t st[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) st[i] = ist[i];
#pragma unroll
  for (int b = 0; b < NB; ++b) sha256_compress(st, w + 16 * b);
  uint32_t o[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) o[i] = i < 8 ? st[i] : 0u;
  o[8] = 0x80000000u;
  o[15] = (64 + 32) * 8;
#pragma unroll
  for (int i = 0; i < 8; ++i) out[i] = ost[i];
  sha256_compress(out, o);
}

// "HPKE-v1" || suite_id("KEM" || 0x0020) at off (12 bytes)
DEVI void msg_kem_prefix(uint32_t* w, int off) {
  msg_str(w, off, "HPKE-v1");
  msg_str(w, off + 7, "KEM");
  msg_byte(w, off + 11, 0x20u);
}
// "HPKE-v1" || suite_id("HPKE" || kem || 0x0001 || aead) at off (17 bytes); kem_lo is the KEM id's
// low byte (wave-uniform)
template <int AEAD>
DEVI void msg_hpke_prefix(uint32_t* w, int off, uint32_t kem_lo) {
  msg_str(w, off, "HPKE-v1");
  msg_str(w, off + 7, "HPKE");
  msg_byte(w, off + 12, kem_lo);
  msg_byte(w, off + 14, 0x01u);
  msg_byte(w, off + 16, (uint32_t)AEAD);
}

// (dh, enc) -> the AEAD key (Nk / 4 BE words) and base nonce (3 BE words): ExtractAndExpand of
// the DHKEM (RFC 9180 §4.1; HKDF-SHA256 for every suite) and KeySchedule(mode_base) (§5.1) under
// the suite's KDF.  19 SHA-256 compressions for KDF 1; 9 and 12 SHA-512 compressions otherwise.
// With bc.dh_ok set (P-256) dh already is the shared_secret and the KEM half is skipped, on a
// wave-uniform branch.
template <int KDF, int AEAD>
DEVI void hpke_key_nonce(const HpkeBatchConsts& bc, const uint32_t dh[8], const uint32_t enc[8],
                         uint32_t* key, uint32_t nonce[3]) {
  constexpr int NK = hpke_aead_nk(AEAD);
  uint32_t w[32], ist[8], ost[8], prk[8], ss[8], secret[8], t[8];
  if (bc.dh_ok) {
#pragma unroll
    for (int i = 0; i < 8; ++i) ss[i] = dh[i];
  } else {
    // eae_prk = LabeledExtract("", "eae_prk", dh)
#pragma unroll
    for (int i = 0; i < 16; ++i) w[i] = 0;
    msg_kem_prefix(w, 0);
    msg_str(w, 12, "eae_prk");
    msg_words8(w, 19, dh);
    msg_pad(w, 51, 1);
    hmac_finish<1>(bc.salt0_i, bc.salt0_o, w, prk);
    // shared_secret = LabeledExpand(eae_prk, "shared_secret", enc || pkR, 32)
    hmac_pads(prk, ist, ost);
#pragma unroll
    for (int i = 0; i < 32; ++i) w[i] = 0;
    msg_byte(w, 1, 32u);
    msg_kem_prefix(w, 2);
    msg_str(w, 14, "shared_secret");
    msg_words8(w, 27, enc);
    msg_words8(w, 59, bc.pk);
    msg_byte(w, 91, 1u);
    msg_pad(w, 92, 2);
    hmac_finish<2>(ist, ost, w, ss);
  }
  if constexpr (KDF != 1) {
    uint64_t secret64[8];
    hpke_kdf512_key_nonce<KDF, AEAD>(ss, bc.psk_id_hash, bc.info_hash, secret64, key, nonce,
                                     bc.kem_lo);
    return;
  }
  // secret = LabeledExtract(shared_secret, "secret", psk = "")
  hmac_pads(ss, ist, ost);
#pragma unroll
  for (int i = 0; i < 16; ++i) w[i] = 0;
  msg_hpke_prefix<AEAD>(w, 0, bc.kem_lo);
  msg_str(w, 17, "secret");
  msg_pad(w, 23, 1);
  hmac_finish<1>(ist, ost, w, secret);
  // key = LabeledExpand(secret, "key", key_schedule_context, Nk);  context = mode 0 ||
  // psk_id_hash || info_hash
  hmac_pads(secret, ist, ost);
#pragma unroll
  for (int i = 0; i < 32; ++i) w[i] = 0;
  msg_byte(w, 1, (uint32_t)NK);
  msg_hpke_prefix<AEAD>(w, 2, bc.kem_lo);
  msg_str(w, 19, "key");
  msg_words8(w, 23, bc.psk_id_hash);
  msg_words8(w, 55, bc.info_hash);
  msg_byte(w, 87, 1u);
  msg_pad(w, 88, 2);
  hmac_finish<2>(ist, ost, w, t);
#pragma unroll
  for (int i = 0; i < NK / 4; ++i) key[i] = t[i];
  // base_nonce = LabeledExpand(secret, "base_nonce", key_schedule_context, 12)
#pragma unroll
  for (int i = 0; i < 32; ++i) w[i] = 0;
  msg_byte(w, 1, 12u);
  msg_hpke_prefix<AEAD>(w, 2, bc.kem_lo);
  msg_str(w, 19, "base_nonce");
  msg_words8(w, 30, bc.psk_id_hash);
  msg_words8(w, 62, bc.info_hash);
  msg_byte(w, 94, 1u);
  msg_pad(w, 95, 2);
  hmac_finish<2>(ist, ost, w, t);
#pragma unroll
  for (int i = 0; i < 3; ++i) nonce[i] = t[i];
}

}  // namespace p3g
