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
// Each kernel is a thin shell around a per-lane device function (x25519_lane, hpke_open_lane over
// a byte source for the AAD) that helper_request.h's kernels call too, with the request read in
// place.  SHA-512, ChaCha20 and Poly1305 are hpke_prims.h's (free of HIP, tested on the CPU).
// SHA-256 is sha256.h's.  Included by engine_hpke.hip.
#pragma once
#include "hpke_prims.h"
#include "hpke_shared.h"
#include "sha256.h"
#include "p256_kem.h"

namespace p3g {

constexpr uint8_t ST_HPKE_DECRYPT = 4;  // PrepareError::HpkeDecryptError

// ------------------------------------------------------------------------------------------------
// GF(2^255 - 19), ten limbs of 26 / 25 bits (value = sum v[i] 2^ceil(25.5 i)), unsigned.
// A "carried" element (output of fe_carry) has v[0], v[2..9] below 2^26 / 2^25 and v[1] below
// 2^25 + 2^18.  fe_add / fe_sub do not carry: their outputs stay below 3 * 2^26 (even limbs) and
// 3 * 2^25 (odd limbs), for which a 10-term column of fe_mul / fe_sq stays below
// 10 * 19 * 9.2 * 2^52 < 2^63 and every 32-bit premultiple (19 x, 2 x, 4 x) below 2^32.
// Products are (uint64_t)a * b + acc, i.e. one v_mad_u64_u32 each.
// ------------------------------------------------------------------------------------------------
struct Fe25 {
  uint32_t v[10];
};
struct X25519Scalar {  // clamped scalar, little-endian words; a kernel argument (SGPRs)
  uint32_t w[8];
};

DEVI void fe_carry(Fe25& h, uint64_t t[10]) {
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const int bits = (i & 1) ? 25 : 26;
    t[i] += c;
    c = t[i] >> bits;
    t[i] &= (1ull << bits) - 1;
  }
  t[0] += 19 * c;  // c < 2^39
  c = t[0] >> 26;
  t[0] &= (1ull << 26) - 1;
  t[1] += c;
#pragma unroll
  for (int i = 0; i < 10; ++i) h.v[i] = (uint32_t)t[i];
}

DEVI void fe_mul(Fe25& h, const Fe25& f, const Fe25& g) {
  uint32_t g19[10];
#pragma unroll
  for (int j = 0; j < 10; ++j) g19[j] = 19u * g.v[j];
  uint64_t t[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) t[k] = 0;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
#pragma unroll
    for (int j = 0; j < 10; ++j) {
      const int k = i + j;
      // 2^(off_i + off_j) = 2 * 2^off_(i+j) when both are odd limbs; 2^255 = 19
      const uint32_t a = ((i & 1) && (j & 1)) ? 2u * f.v[i] : f.v[i];
      const uint32_t b = k >= 10 ? g19[j] : g.v[j];
      t[k % 10] += (uint64_t)a * b;
    }
  }
  fe_carry(h, t);
}

DEVI void fe_sq(Fe25& h, const Fe25& f) {  // 55 products instead of 100
  uint32_t f19[10];
#pragma unroll
  for (int j = 0; j < 10; ++j) f19[j] = 19u * f.v[j];
  uint64_t t[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) t[k] = 0;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
#pragma unroll
    for (int j = i; j < 10; ++j) {
      const int k = i + j;
      const uint32_t m = (i < j ? 2u : 1u) * (((i & 1) && (j & 1)) ? 2u : 1u);
      const uint32_t a = m * f.v[i];
      const uint32_t b = k >= 10 ? f19[j] : f.v[j];
      t[k % 10] += (uint64_t)a * b;
    }
  }
  fe_carry(h, t);
}

DEVI void fe_mul_small(Fe25& h, const Fe25& f, uint32_t k) {  // k < 2^18
  uint64_t t[10];
#pragma unroll
  for (int i = 0; i < 10; ++i) t[i] = (uint64_t)f.v[i] * k;
  fe_carry(h, t);
}

DEVI void fe_add(Fe25& h, const Fe25& f, const Fe25& g) {  // f, g carried
#pragma unroll
  for (int i = 0; i < 10; ++i) h.v[i] = f.v[i] + g.v[i];
}

DEVI void fe_sub(Fe25& h, const Fe25& f, const Fe25& g) {  // f - g + 2p;  f, g carried
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint32_t bias = i == 0 ? 0x7FFFFDAu : ((i & 1) ? 0x3FFFFFEu : 0x7FFFFFEu);
    h.v[i] = f.v[i] + bias - g.v[i];
  }
}

DEVI void fe_cswap(Fe25& a, Fe25& b, uint32_t swap) {  // swap is wave-uniform; still a select
  const uint32_t m = 0u - swap;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint32_t t = m & (a.v[i] ^ b.v[i]);
    a.v[i] ^= t;
    b.v[i] ^= t;
  }
}

DEVI void fe_sqn(Fe25& h, const Fe25& f, int n) {
  fe_sq(h, f);
#pragma unroll 1
  for (int i = 1; i < n; ++i) fe_sq(h, h);
}

// z^(p-2): the usual addition chain (254 squarings, 11 multiplications)
DEVI void fe_invert(Fe25& out, const Fe25& z) {
  Fe25 z2, z9, z11, z_5_0, z_10_0, z_20_0, z_50_0, z_100_0, t;
  fe_sq(z2, z);
  fe_sqn(t, z2, 2);
  fe_mul(z9, t, z);
  fe_mul(z11, z9, z2);
  fe_sq(t, z11);
  fe_mul(z_5_0, t, z9);
  fe_sqn(t, z_5_0, 5);
  fe_mul(z_10_0, t, z_5_0);
  fe_sqn(t, z_10_0, 10);
  fe_mul(z_20_0, t, z_10_0);
  fe_sqn(t, z_20_0, 20);
  fe_mul(t, t, z_20_0);
  fe_sqn(t, t, 10);
  fe_mul(z_50_0, t, z_10_0);
  fe_sqn(t, z_50_0, 50);
  fe_mul(z_100_0, t, z_50_0);
  fe_sqn(t, z_100_0, 100);
  fe_mul(t, t, z_100_0);
  fe_sqn(t, t, 50);
  fe_mul(t, t, z_50_0);
  fe_sqn(t, t, 5);
  fe_mul(out, t, z11);
}

constexpr int fe_off(int i) { return (51 * i + 1) / 2; }  // 0, 26, 51, 77, ..., 230

// 32 little-endian bytes as words -> limbs; bit 255 is dropped and u >= p is accepted as it is
// (RFC 7748 §5), like the host ladders.
DEVI void fe_from_words(Fe25& h, const uint32_t w[8]) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const int off = fe_off(i), wd = off >> 5, sh = off & 31, bits = (i & 1) ? 25 : 26;
    uint32_t x = w[wd] >> sh;
    if (sh + bits > 32 && wd + 1 < 8) x |= w[wd + 1] << (32 - sh);
    h.v[i] = x & ((1u << bits) - 1);
  }
}

// carried limbs -> the canonical value (< p) as 8 little-endian words
DEVI void fe_to_words(uint32_t w[8], const Fe25& f) {
  uint32_t h[10];
#pragma unroll
  for (int i = 0; i < 10; ++i) h[i] = f.v[i];
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
      const int bits = (i & 1) ? 25 : 26;
      h[i] += c;
      c = h[i] >> bits;
      h[i] &= (1u << bits) - 1;
    }
    h[0] += 19u * c;
  }
  uint32_t q = (h[0] + 19u) >> 26;  // q = 1 iff h >= p
#pragma unroll
  for (int i = 1; i < 10; ++i) q = (h[i] + q) >> ((i & 1) ? 25 : 26);
  h[0] += 19u * q;
  uint32_t c = 0;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const int bits = (i & 1) ? 25 : 26;
    h[i] += c;
    c = h[i] >> bits;
    h[i] &= (1u << bits) - 1;  // the last carry is 2^255: dropped
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) w[k] = 0;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const int off = fe_off(i), wd = off >> 5, sh = off & 31, bits = (i & 1) ? 25 : 26;
    w[wd] |= h[i] << sh;
    if (sh + bits > 32) w[wd + 1] |= h[i] >> (32 - sh);
  }
}

// 32 bytes at p (any alignment) as little-endian words
DEVI void load_le_words8(const uint8_t* p, uint32_t w[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i)
    w[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) |
           ((uint32_t)p[4 * i + 3] << 24);
}

// w = X25519(k, w) for this lane's point (little-endian words).  The Montgomery ladder of RFC 7748
// §5; the scalar is wave-uniform, its bits are read with uniform selects and used only as swap
// masks, so no branch and no address depends on the scalar or on a field value.
DEVI void x25519_lane(const X25519Scalar& k, uint32_t w[8]) {
  Fe25 x1, x2, z2, x3, z3;
  fe_from_words(x1, w);
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    x2.v[i] = z3.v[i] = i ? 0u : 1u;
    z2.v[i] = 0u;
  }
  x3 = x1;
  uint32_t swap = 0;
#pragma unroll 1
  for (int t = 254; t >= 0; --t) {
    const int wi = t >> 5;
    uint32_t kw = k.w[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) kw = wi == i ? k.w[i] : kw;
    const uint32_t kt = (kw >> (t & 31)) & 1u;
    swap ^= kt;
    fe_cswap(x2, x3, swap);
    fe_cswap(z2, z3, swap);
    swap = kt;
    Fe25 A, AA, B, BB, E, C, D, DA, CB, t0, t1;
    fe_add(A, x2, z2);
    fe_sq(AA, A);
    fe_sub(B, x2, z2);
    fe_sq(BB, B);
    fe_sub(E, AA, BB);
    fe_add(C, x3, z3);
    fe_sub(D, x3, z3);
    fe_mul(DA, D, A);
    fe_mul(CB, C, B);
    fe_add(t0, DA, CB);
    fe_sq(x3, t0);
    fe_sub(t1, DA, CB);
    fe_sq(t1, t1);
    fe_mul(z3, x1, t1);
    fe_mul(x2, AA, BB);
    fe_mul_small(t0, E, 121665u);
    fe_add(t0, AA, t0);
    fe_mul(z2, E, t0);
  }
  fe_cswap(x2, x3, swap);
  fe_cswap(z2, z3, swap);
  Fe25 inv;
  fe_invert(inv, z2);
  fe_mul(x2, x2, inv);
  fe_to_words(w, x2);
}

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

// ------------------------------------------------------------------------------------------------
// AES-128 / AES-256 (FIPS 197; NK = 4 / 8 key words, NK + 6 rounds) with the S-box in LDS (computed
// by the block: inverse in GF(2^8) + affine map), and GHASH bit-serial (SP 800-38D §6.3): X25519
// dominates the open, so the simplest forms.
// A 16-byte block is four words, byte j at bits 8 (j & 3) of word j >> 2.
// ------------------------------------------------------------------------------------------------
DEVI uint32_t gf8_mul(uint32_t a, uint32_t b) {
  uint32_t r = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    r ^= (0u - (b & 1u)) & a;
    a = ((a << 1) ^ ((0u - (a >> 7)) & 0x11bu)) & 0xffu;
    b >>= 1;
  }
  return r;
}

DEVI void aes_sbox_init(uint8_t* sbox) {  // every thread of the block; the caller synchronises
  for (uint32_t x = threadIdx.x; x < 256u; x += blockDim.x) {
    uint32_t p = x, inv = 1u;  // x^254 = x^2 x^4 ... x^128
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      p = gf8_mul(p, p);
      inv = gf8_mul(inv, p);
    }
    if (x == 0u) inv = 0u;
    uint32_t s = inv;
#pragma unroll
    for (int i = 1; i <= 4; ++i) s ^= ((inv << i) | (inv >> (8 - i))) & 0xffu;
    sbox[x] = (uint8_t)(s ^ 0x63u);
  }
}

DEVI uint32_t aes_sub_word(const uint8_t* sbox, uint32_t x) {
  return (uint32_t)sbox[x & 0xffu] | ((uint32_t)sbox[(x >> 8) & 0xffu] << 8) |
         ((uint32_t)sbox[(x >> 16) & 0xffu] << 16) | ((uint32_t)sbox[x >> 24] << 24);
}

template <int NK>
DEVI void aes_expand(const uint8_t* sbox, const uint32_t* key_be, uint32_t* rk) {  // 4 (NK + 7)
#pragma unroll
  for (int i = 0; i < NK; ++i) rk[i] = bswap32(key_be[i]);
  uint32_t rcon = 1u;
#pragma unroll
  for (int i = NK; i < 4 * (NK + 7); ++i) {
    uint32_t t = rk[i - 1];
    if (i % NK == 0) {
      t = aes_sub_word(sbox, rotr32(t, 8)) ^ rcon;
      rcon = ((rcon << 1) ^ ((0u - (rcon >> 7)) & 0x11bu)) & 0xffu;
    } else if (NK > 6 && i % NK == 4) {
      t = aes_sub_word(sbox, t);
    }
    rk[i] = rk[i - NK] ^ t;
  }
}

template <int NK>
DEVI void aes_encrypt(const uint8_t* sbox, const uint32_t* rk, const uint32_t in[4],
                      uint32_t out[4]) {
  constexpr int NR = NK + 6;
  uint32_t s[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) s[c] = in[c] ^ rk[c];
#pragma unroll
  for (int rnd = 1; rnd <= NR; ++rnd) {
    uint32_t t[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {  // SubBytes + ShiftRows
      t[c] = (uint32_t)sbox[s[c] & 0xffu] | ((uint32_t)sbox[(s[(c + 1) & 3] >> 8) & 0xffu] << 8) |
             ((uint32_t)sbox[(s[(c + 2) & 3] >> 16) & 0xffu] << 16) |
             ((uint32_t)sbox[s[(c + 3) & 3] >> 24] << 24);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      uint32_t x = t[c];
      if (rnd < NR) {  // MixColumns: 2 b_r + 3 b_(r+1) + b_(r+2) + b_(r+3), bytewise in the word
        const uint32_t x2 = ((x & 0x7f7f7f7fu) << 1) ^ (((x >> 7) & 0x01010101u) * 0x1bu);
        x = x2 ^ rotr32(x ^ x2, 8) ^ rotr32(x, 16) ^ rotr32(x, 24);
      }
      s[c] = x ^ rk[4 * rnd + c];
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) out[c] = s[c];
}

// Y = (Y ^ X) * H in GF(2^128), GCM bit order; all as four big-endian words.
DEVI void ghash_step(uint32_t y[4], const uint32_t x[4], const uint32_t h[4]) {
  uint32_t v0 = h[0], v1 = h[1], v2 = h[2], v3 = h[3];
  uint32_t z0 = 0, z1 = 0, z2 = 0, z3 = 0;
#pragma unroll
  for (int wd = 0; wd < 4; ++wd) {
    uint32_t xb = y[wd] ^ x[wd];
#pragma unroll 4
    for (int b = 0; b < 32; ++b) {
      const uint32_t m = 0u - (xb >> 31);
      xb <<= 1;
      z0 ^= v0 & m; z1 ^= v1 & m; z2 ^= v2 & m; z3 ^= v3 & m;
      const uint32_t lsb = 0u - (v3 & 1u);
      v3 = (v3 >> 1) | (v2 << 31);
      v2 = (v2 >> 1) | (v1 << 31);
      v1 = (v1 >> 1) | (v0 << 31);
      v0 = (v0 >> 1) ^ (lsb & 0xe1000000u);
    }
  }
  y[0] = z0; y[1] = z1; y[2] = z2; y[3] = z3;
}

// GHASH the bytes of a source (hpke_prims.h: len(), block(o, d)) into y, zero-padded to whole
// blocks.
template <class Src>
DEVI void ghash_bytes(uint32_t y[4], const uint32_t h[4], const Src& src) {
  const uint64_t len = src.len();
  for (uint64_t o = 0; o < len; o += 16) {
    uint32_t d[4], x[4];
    src.block(o, d);
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = bswap32(d[i]);
    ghash_step(y, x, h);
  }
}

// A report that is not opened: its slot is zeroed; status 4 unless it was skipped on entry.
DEVI void hpke_open_reject(uint8_t* pt, uint64_t pt_cap, uint8_t* status, bool skip) {
  for (uint64_t j = 0; j < pt_cap; ++j) pt[j] = 0;
  if (!skip) *status = ST_HPKE_DECRYPT;
}

// One report, one lane: derive (key, base_nonce) from the lane's dh (8 words as k_x25519 or
// k_p256_dh wrote them) and enc (32 bytes; not read for P-256), check the AEAD's tag over aad ||
// ct[0 .. body), then write the plaintext to pt[0 .. body) and zeros up to pt_cap -- or zeros and
// status 4 when the tag does not match or the DH failed: never unauthenticated plaintext.  The DH
// failed when dh is all zero (X25519, RFC 9180 §7.1.4) or, with bc.dh_ok set (P-256), when the
// report's flag dh_flag is zero -- there an all-zero value is no marker.  ct holds body + 16
// bytes.  sbox is unused (null) for ChaCha20-Poly1305.
template <int KDF, int AEAD, class Aad>
DEVI void hpke_open_lane(const uint8_t* sbox, const HpkeBatchConsts& bc, const uint32_t* dh,
                         uint32_t dh_flag, const uint8_t* enc, const Aad& aad, const uint8_t* ct,
                         uint64_t body, uint8_t* pt, uint64_t pt_cap, uint8_t* status) {
  uint32_t dhw[8], encw[8], nz = 0;
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
  constexpr int NKW = hpke_aead_nk(AEAD) / 4;
  uint32_t key[NKW], nonce[3];
  hpke_key_nonce<KDF, AEAD>(bc, dhw, encw, key, nonce);
  if constexpr (AEAD == 3) {
    uint32_t tag[4];
#pragma unroll
    for (int i = 0; i < NKW; ++i) key[i] = bswap32(key[i]);
#pragma unroll
    for (int i = 0; i < 3; ++i) nonce[i] = bswap32(nonce[i]);
    load_block(ct + body, 16, tag);
    if (nz == 0u || !chacha20poly1305_open(key, nonce, aad, PackedBytes{ct, body}, tag, pt)) {
      hpke_open_reject(pt, pt_cap, status, false);
      return;
    }
    for (uint64_t j = body; j < pt_cap; ++j) pt[j] = 0;
    return;
  }
  uint32_t rk[4 * (NKW + 7)];
  aes_expand<NKW>(sbox, key, rk);
  const uint32_t zero[4] = {0, 0, 0, 0};
  uint32_t hle[4], h[4], ctr[4], ek[4];
  aes_encrypt<NKW>(sbox, rk, zero, hle);  // H = E(K, 0)
#pragma unroll
  for (int i = 0; i < 4; ++i) h[i] = bswap32(hle[i]);
  uint32_t y[4] = {0, 0, 0, 0};
  ghash_bytes(y, h, aad);
  ghash_bytes(y, h, PackedBytes{ct, body});
  const uint64_t abits = aad.len() * 8, cbits = body * 8;
  const uint32_t lens[4] = {(uint32_t)(abits >> 32), (uint32_t)abits, (uint32_t)(cbits >> 32),
                            (uint32_t)cbits};
  ghash_step(y, lens, h);
#pragma unroll
  for (int i = 0; i < 3; ++i) ctr[i] = bswap32(nonce[i]);
  ctr[3] = bswap32(1u);  // J0 = nonce || 1 (seq 0: the nonce is base_nonce)
  aes_encrypt<NKW>(sbox, rk, ctr, ek);
  uint32_t tag[4], diff = 0;
  load_block(ct + body, 16, tag);
#pragma unroll
  for (int i = 0; i < 4; ++i) diff |= (bswap32(y[i]) ^ ek[i]) ^ tag[i];  // no early exit
  if (diff != 0u || nz == 0u) {
    hpke_open_reject(pt, pt_cap, status, false);
    return;
  }
  for (uint64_t o = 0; o < body; o += 16) {  // CTR from counter 2
    uint32_t d[4];
    load_block(ct + o, body - o, d);
    ctr[3] = bswap32((uint32_t)(o >> 4) + 2u);
    aes_encrypt<NKW>(sbox, rk, ctr, ek);
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (o + j < body) pt[o + j] = (uint8_t)((d[j >> 2] ^ ek[j >> 2]) >> (8 * (j & 3)));
  }
  for (uint64_t j = body; j < pt_cap; ++j) pt[j] = 0;
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
    aes_sbox_init(sbox_lds);
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
