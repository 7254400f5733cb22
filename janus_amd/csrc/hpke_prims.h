// The primitives of the GPU HPKE open and seal (hpke_lane.h) beyond HKDF-SHA256 (hpke_kdf256.h) and
// AES-GCM (aes_gcm.h), free of HIP so the device kernels and a CPU test
// (tests/native/hpke_prims_host.cpp) run the same code:
//   sha512_compress, sha384_iv / sha512_iv      FIPS 180-4, 64-bit big-endian words
//   msg64_* / hmac512_pads / hmac512_finish     HMAC over fixed-layout messages, 128-byte block
//   hpke_kdf512_key_nonce                       RFC 9180 §5.1 KeySchedule(mode_base) for
//                                               HKDF-SHA384 (KDF 2) and HKDF-SHA512 (KDF 3)
//   chacha20_block, Poly1305                    RFC 8439 §2.3, §2.5
//   chacha20poly1305_open                       RFC 8439 §2.8 over GHASH's byte-source interface
//   chacha20poly1305_seal                       its mirror for the GPU seal
//   load_block / PackedBytes                    that interface's contiguous source
//   store_block / mask_block                    a block's bytes out; zeros past a short block's end
// Nothing here indexes memory or branches by key material: rotations are plain shifts, Poly1305's
// final subtraction is a select, the tag comparison has no early exit.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define P3G_HP __host__ __device__ __forceinline__
#else
#define P3G_HP inline
#endif

namespace p3g {

P3G_HP uint64_t hp_rotr64(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }
P3G_HP uint32_t hp_rotl32(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }
P3G_HP uint32_t hp_bswap32(uint32_t x) {
  return (x >> 24) | ((x >> 8) & 0xff00u) | ((x << 8) & 0xff0000u) | (x << 24);
}

// up to 16 bytes at p (rem of them exist; the rest read as zero) -> block words, byte j at bits
// 8 (j & 3) of word j >> 2
P3G_HP void load_block(const uint8_t* p, uint64_t rem, uint32_t d[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) d[i] = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const uint32_t b = (uint64_t)j < rem ? (uint32_t)p[j] : 0u;
    d[j >> 2] |= b << (8 * (j & 3));
  }
}

// A byte source for GHASH / Poly1305: len() bytes, block(o, d) = the 16 bytes at offset o (a
// multiple of 16) as block words, zero past the end.  PackedBytes is the contiguous one.
struct PackedBytes {
  const uint8_t* p;
  uint64_t n;
  P3G_HP uint64_t len() const { return n; }
  P3G_HP void block(uint64_t o, uint32_t d[4]) const { load_block(p + o, n - o, d); }
  // block(o, d) where all sixteen bytes exist (o + 16 <= n): one 16-byte load
  P3G_HP void whole(uint64_t o, uint32_t d[4]) const { __builtin_memcpy(d, p + o, 16); }
};

// ------------------------------------------------------------------------------------------------
// SHA-384 / SHA-512
// ------------------------------------------------------------------------------------------------
P3G_HP void sha512_iv(uint64_t h[8]) {
  h[0] = 0x6a09e667f3bcc908ull; h[1] = 0xbb67ae8584caa73bull; h[2] = 0x3c6ef372fe94f82bull;
  h[3] = 0xa54ff53a5f1d36f1ull; h[4] = 0x510e527fade682d1ull; h[5] = 0x9b05688c2b3e6c1full;
  h[6] = 0x1f83d9abfb41bd6bull; h[7] = 0x5be0cd19137e2179ull;
}
P3G_HP void sha384_iv(uint64_t h[8]) {
  h[0] = 0xcbbb9d5dc1059ed8ull; h[1] = 0x629a292a367cd507ull; h[2] = 0x9159015a3070dd17ull;
  h[3] = 0x152fecd8f70e5939ull; h[4] = 0x67332667ffc00b31ull; h[5] = 0x8eb44a8768581511ull;
  h[6] = 0xdb0c2e0d64f98fa7ull; h[7] = 0x47b5481dbefa4fa4ull;
}

constexpr uint64_t kSha512K[80] = {
    0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull,
    0x3956c25bf348b538ull, 0x59f111f1b605d019ull, 0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull,
    0xd807aa98a3030242ull, 0x12835b0145706fbeull, 0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull,
    0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull, 0xc19bf174cf692694ull,
    0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull, 0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull,
    0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull,
    0x983e5152ee66dfabull, 0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull,
    0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull, 0x06ca6351e003826full, 0x142929670a0e6e70ull,
    0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull, 0x53380d139d95b3dfull,
    0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull,
    0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull, 0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull,
    0xd192e819d6ef5218ull, 0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull,
    0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull, 0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull,
    0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull, 0x5b9cca4f7763e373ull, 0x682e6ff3d6b2b8a3ull,
    0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
    0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull,
    0xca273eceea26619cull, 0xd186b8c721c0c207ull, 0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull,
    0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull, 0x113f9804bef90daeull, 0x1b710b35131c471bull,
    0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull, 0x431d67c49c100d4cull,
    0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull, 0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull};

// One compression: h (8 state words) absorbs the 128-byte block given as 16 big-endian words (w
// is consumed as the message schedule).  Five passes of 16 unrolled rounds; the passes stay a
// loop (an HPKE open runs 12 compressions per lane, and unrolled they cost the AES-256 kernels
// their registers and the build minutes), so the round constants are read from the table.
P3G_HP void sha512_compress(uint64_t h[8], uint64_t w[16]) {
  const uint64_t iv[8] = {h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7]};
  uint64_t a = iv[0], b = iv[1], c = iv[2], d = iv[3], e = iv[4], f = iv[5], g = iv[6], hh = iv[7];
#pragma unroll 1
  for (int t0 = 0; t0 < 80; t0 += 16) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const uint64_t S1 = hp_rotr64(e, 14) ^ hp_rotr64(e, 18) ^ hp_rotr64(e, 41);
      const uint64_t ch = (e & f) ^ (~e & g);
      const uint64_t t1 = hh + S1 + ch + kSha512K[t0 + j] + w[j];
      const uint64_t S0 = hp_rotr64(a, 28) ^ hp_rotr64(a, 34) ^ hp_rotr64(a, 39);
      const uint64_t mj = (a & b) ^ (a & c) ^ (b & c);
      const uint64_t t2 = S0 + mj;
      hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {  // the schedule of the next pass, in place (unused after the last)
      const uint64_t w15 = w[(j + 1) & 15], w2 = w[(j + 14) & 15];
      const uint64_t s0 = hp_rotr64(w15, 1) ^ hp_rotr64(w15, 8) ^ (w15 >> 7);
      const uint64_t s1 = hp_rotr64(w2, 19) ^ hp_rotr64(w2, 61) ^ (w2 >> 6);
      w[j] = w[j] + s0 + w[(j + 9) & 15] + s1;
    }
  }
  h[0] = iv[0] + a; h[1] = iv[1] + b; h[2] = iv[2] + c; h[3] = iv[3] + d;
  h[4] = iv[4] + e; h[5] = iv[5] + f; h[6] = iv[6] + g; h[7] = iv[7] + hh;
}

// ------------------------------------------------------------------------------------------------
// HMAC-SHA384 / HMAC-SHA512 over fixed-layout messages: the counterpart of hpke_kdf256.h's msg_* /
// hmac_* for a 128-byte block.  KDF is the HPKE KDF id: 2 (SHA-384, Nh = 48) or 3 (SHA-512,
// Nh = 64).  A message is built as big-endian 64-bit words at byte offsets that are compile-time
// constants in the kernels (constant bytes fold into the schedule).
// ------------------------------------------------------------------------------------------------
template <int KDF>
struct Kdf512 {
  static_assert(KDF == 2 || KDF == 3, "HKDF-SHA384 or HKDF-SHA512");
  static constexpr int NH = KDF == 2 ? 48 : 64;  // output bytes
  static constexpr int NHW = NH / 8;             // ... as 64-bit words
};

P3G_HP void msg64_byte(uint64_t* w, int off, uint64_t b) {
  w[off >> 3] |= b << (56 - 8 * (off & 7));
}

template <int N>
P3G_HP void msg64_str(uint64_t* w, int off, const char (&s)[N]) {  // the N - 1 characters of s
#pragma unroll
  for (int i = 0; i < N - 1; ++i) msg64_byte(w, off + i, (uint64_t)(uint8_t)s[i]);
}

// 4 n bytes given as n big-endian 32-bit words
P3G_HP void msg64_words32(uint64_t* w, int off, const uint32_t* v, int n) {
#pragma unroll
  for (int i = 0; i < n; ++i) {
    const int p = off + 4 * i, sh = 8 * (p & 7), idx = p >> 3;
    if (sh <= 32) {
      w[idx] |= (uint64_t)v[i] << (32 - sh);
    } else {
      w[idx] |= (uint64_t)v[i] >> (sh - 32);
      w[idx + 1] |= (uint64_t)v[i] << (96 - sh);
    }
  }
}

// SHA-512 padding of a `len`-byte message in nblk blocks that follows `before` hashed bytes
// (128 after an HMAC pad block, 0 for a plain hash).
P3G_HP void msg64_pad(uint64_t* w, int len, int nblk, int before) {
  msg64_byte(w, len, 0x80u);
  w[16 * nblk - 1] = (uint64_t)(before + len) * 8u;
}

// the pad states of an nk-word key (8 nk <= 128 bytes; zero-padded to the block)
template <int KDF>
P3G_HP void hmac512_pads(const uint64_t* key, int nk, uint64_t ist[8], uint64_t ost[8]) {
  uint64_t w[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) w[i] = (i < nk ? key[i] : 0ull) ^ 0x3636363636363636ull;
  if (KDF == 2) sha384_iv(ist); else sha512_iv(ist);
  sha512_compress(ist, w);
#pragma unroll
  for (int i = 0; i < 16; ++i) w[i] = (i < nk ? key[i] : 0ull) ^ 0x5c5c5c5c5c5c5c5cull;
  if (KDF == 2) sha384_iv(ost); else sha512_iv(ost);
  sha512_compress(ost, w);
}

// HMAC of the padded NB-block message w (consumed) under the key whose pad states are ist / ost;
// the first Nh / 8 words of out are the MAC.
template <int KDF, int NB>
P3G_HP void hmac512_finish(const uint64_t ist[8], const uint64_t ost[8], uint64_t* w,
                           uint64_t out[8]) {
  constexpr int NHW = Kdf512<KDF>::NHW;
  uint64_t st[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) st[i] = ist[i];
#pragma unroll
  for (int b = 0; b < NB; ++b) sha512_compress(st, w + 16 * b);
  uint64_t o[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) o[i] = i < NHW ? st[i] : 0ull;
  o[NHW] = 0x8000000000000000ull;
  o[15] = (uint64_t)(128 + 8 * NHW) * 8u;
#pragma unroll
  for (int i = 0; i < 8; ++i) out[i] = ost[i];
  sha512_compress(out, o);
}

constexpr int hpke_aead_nk(int aead) { return aead == 1 ? 16 : 32; }  // AEAD key bytes (Nk)

// "HPKE-v1" || suite_id("HPKE" || kem || kdf || aead) at off (17 bytes); kem_lo is the KEM id's low
// byte (0x20 X25519, 0x10 P-256; the high byte is zero)
template <int KDF, int AEAD>
P3G_HP void msg64_hpke_prefix(uint64_t* w, int off, uint32_t kem_lo) {
  msg64_str(w, off, "HPKE-v1");
  msg64_str(w, off + 7, "HPKE");
  msg64_byte(w, off + 12, (uint64_t)kem_lo);
  msg64_byte(w, off + 14, (uint64_t)KDF);
  msg64_byte(w, off + 16, (uint64_t)AEAD);
}

// The suite-KDF half of KeySchedule(mode_base) (RFC 9180 §5.1) for KDF 2 / 3: shared_secret (8
// big-endian 32-bit words), psk_id_hash and info_hash (Nh bytes each as big-endian 32-bit words)
// -> secret (Nh / 8 64-bit words), key (Nk / 4 big-endian 32-bit words) and base_nonce (3).
// L <= Nh for both expands, so each is one HKDF block.  12 SHA-512 compressions.
template <int KDF, int AEAD>
P3G_HP void hpke_kdf512_key_nonce(const uint32_t ss[8], const uint32_t* psk_id_hash,
                                  const uint32_t* info_hash, uint64_t secret[8], uint32_t* key,
                                  uint32_t nonce[3], uint32_t kem_lo = 0x20u) {
  constexpr int NH = Kdf512<KDF>::NH, NHW = Kdf512<KDF>::NHW, NK = hpke_aead_nk(AEAD);
  uint64_t w[32], ist[8], ost[8], t[8], ssw[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) ssw[i] = ((uint64_t)ss[2 * i] << 32) | ss[2 * i + 1];
  // secret = LabeledExtract(shared_secret, "secret", psk = "")
  hmac512_pads<KDF>(ssw, 4, ist, ost);
#pragma unroll
  for (int i = 0; i < 16; ++i) w[i] = 0;
  msg64_hpke_prefix<KDF, AEAD>(w, 0, kem_lo);
  msg64_str(w, 17, "secret");
  msg64_pad(w, 23, 1, 128);
  hmac512_finish<KDF, 1>(ist, ost, w, secret);
  // key = LabeledExpand(secret, "key", key_schedule_context, Nk);  context = mode 0 ||
  // psk_id_hash || info_hash
  hmac512_pads<KDF>(secret, NHW, ist, ost);
#pragma unroll
  for (int i = 0; i < 32; ++i) w[i] = 0;
  msg64_byte(w, 1, (uint64_t)NK);
  msg64_hpke_prefix<KDF, AEAD>(w, 2, kem_lo);
  msg64_str(w, 19, "key");
  msg64_words32(w, 23, psk_id_hash, NH / 4);
  msg64_words32(w, 23 + NH, info_hash, NH / 4);
  msg64_byte(w, 23 + 2 * NH, 1u);
  msg64_pad(w, 24 + 2 * NH, 2, 128);
  hmac512_finish<KDF, 2>(ist, ost, w, t);
#pragma unroll
  for (int i = 0; i < NK / 4; ++i) key[i] = (uint32_t)(t[i >> 1] >> ((i & 1) ? 0 : 32));
  // base_nonce = LabeledExpand(secret, "base_nonce", key_schedule_context, 12)
#pragma unroll
  for (int i = 0; i < 32; ++i) w[i] = 0;
  msg64_byte(w, 1, 12u);
  msg64_hpke_prefix<KDF, AEAD>(w, 2, kem_lo);
  msg64_str(w, 19, "base_nonce");
  msg64_words32(w, 30, psk_id_hash, NH / 4);
  msg64_words32(w, 30 + NH, info_hash, NH / 4);
  msg64_byte(w, 30 + 2 * NH, 1u);
  msg64_pad(w, 31 + 2 * NH, 2, 128);
  hmac512_finish<KDF, 2>(ist, ost, w, t);
#pragma unroll
  for (int i = 0; i < 3; ++i) nonce[i] = (uint32_t)(t[i >> 1] >> ((i & 1) ? 0 : 32));
}

// ------------------------------------------------------------------------------------------------
// ChaCha20 (RFC 8439 §2.3): key 8, nonce 3 little-endian words; out = the 64-byte block as 16
// little-endian words.
// ------------------------------------------------------------------------------------------------
P3G_HP void chacha20_qr(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d) {
  a += b; d ^= a; d = hp_rotl32(d, 16);
  c += d; b ^= c; b = hp_rotl32(b, 12);
  a += b; d ^= a; d = hp_rotl32(d, 8);
  c += d; b ^= c; b = hp_rotl32(b, 7);
}

P3G_HP void chacha20_block(const uint32_t key[8], uint32_t counter, const uint32_t nonce[3],
                           uint32_t out[16]) {
  uint32_t in[16], x[16];
  in[0] = 0x61707865u; in[1] = 0x3320646eu; in[2] = 0x79622d32u; in[3] = 0x6b206574u;
#pragma unroll
  for (int i = 0; i < 8; ++i) in[4 + i] = key[i];
  in[12] = counter;
#pragma unroll
  for (int i = 0; i < 3; ++i) in[13 + i] = nonce[i];
#pragma unroll
  for (int i = 0; i < 16; ++i) x[i] = in[i];
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    chacha20_qr(x[0], x[4], x[8], x[12]);
    chacha20_qr(x[1], x[5], x[9], x[13]);
    chacha20_qr(x[2], x[6], x[10], x[14]);
    chacha20_qr(x[3], x[7], x[11], x[15]);
    chacha20_qr(x[0], x[5], x[10], x[15]);
    chacha20_qr(x[1], x[6], x[11], x[12]);
    chacha20_qr(x[2], x[7], x[8], x[13]);
    chacha20_qr(x[3], x[4], x[9], x[14]);
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) out[i] = x[i] + in[i];
}

// ------------------------------------------------------------------------------------------------
// Poly1305 (RFC 8439 §2.5), five 26-bit limbs.  After a block h[0], h[2..4] are below 2^26 and
// h[1] below 2^26 + 2^10; with a block added every limb stays below 2^27 + 2^10, r[i] < 2^26 and
// 5 r[i] < 2^29, so a five-term column stays below 5 * 2^57 < 2^60.  Products are
// (uint64_t)a * b + acc, i.e. one v_mad_u64_u32 each on the GPU.
// ------------------------------------------------------------------------------------------------
struct Poly1305 {
  uint32_t r[5], h[5], s[4];
};

// k = r || s as 8 little-endian words; r is clamped here
P3G_HP void poly1305_init(Poly1305& p, const uint32_t k[8]) {
  p.r[0] = k[0] & 0x3ffffffu;
  p.r[1] = ((k[0] >> 26) | (k[1] << 6)) & 0x3ffff03u;
  p.r[2] = ((k[1] >> 20) | (k[2] << 12)) & 0x3ffc0ffu;
  p.r[3] = ((k[2] >> 14) | (k[3] << 18)) & 0x3f03fffu;
  p.r[4] = (k[3] >> 8) & 0x00fffffu;
#pragma unroll
  for (int i = 0; i < 5; ++i) p.h[i] = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) p.s[i] = k[4 + i];
}

// h = (h + m + hibit 2^104 limb-wise) r mod 2^130 - 5;  m = 16 bytes as block words, hibit =
// 1 << 24 for a whole block (the 2^128 bit), 0 for a last block that carries its own 0x01 byte
P3G_HP void poly1305_block(Poly1305& p, const uint32_t m[4], uint32_t hibit) {
  constexpr uint32_t M = 0x3ffffffu;
  const uint32_t r0 = p.r[0], r1 = p.r[1], r2 = p.r[2], r3 = p.r[3], r4 = p.r[4];
  const uint32_t s1 = 5u * r1, s2 = 5u * r2, s3 = 5u * r3, s4 = 5u * r4;
  const uint32_t h0 = p.h[0] + (m[0] & M);
  const uint32_t h1 = p.h[1] + (((m[0] >> 26) | (m[1] << 6)) & M);
  const uint32_t h2 = p.h[2] + (((m[1] >> 20) | (m[2] << 12)) & M);
  const uint32_t h3 = p.h[3] + (((m[2] >> 14) | (m[3] << 18)) & M);
  const uint32_t h4 = p.h[4] + ((m[3] >> 8) | hibit);
  uint64_t d0 = (uint64_t)h0 * r0;
  d0 = (uint64_t)h1 * s4 + d0; d0 = (uint64_t)h2 * s3 + d0;
  d0 = (uint64_t)h3 * s2 + d0; d0 = (uint64_t)h4 * s1 + d0;
  uint64_t d1 = (uint64_t)h0 * r1;
  d1 = (uint64_t)h1 * r0 + d1; d1 = (uint64_t)h2 * s4 + d1;
  d1 = (uint64_t)h3 * s3 + d1; d1 = (uint64_t)h4 * s2 + d1;
  uint64_t d2 = (uint64_t)h0 * r2;
  d2 = (uint64_t)h1 * r1 + d2; d2 = (uint64_t)h2 * r0 + d2;
  d2 = (uint64_t)h3 * s4 + d2; d2 = (uint64_t)h4 * s3 + d2;
  uint64_t d3 = (uint64_t)h0 * r3;
  d3 = (uint64_t)h1 * r2 + d3; d3 = (uint64_t)h2 * r1 + d3;
  d3 = (uint64_t)h3 * r0 + d3; d3 = (uint64_t)h4 * s4 + d3;
  uint64_t d4 = (uint64_t)h0 * r4;
  d4 = (uint64_t)h1 * r3 + d4; d4 = (uint64_t)h2 * r2 + d4;
  d4 = (uint64_t)h3 * r1 + d4; d4 = (uint64_t)h4 * r0 + d4;
  uint64_t c = d0 >> 26;
  p.h[0] = (uint32_t)d0 & M;
  d1 += c; c = d1 >> 26; p.h[1] = (uint32_t)d1 & M;
  d2 += c; c = d2 >> 26; p.h[2] = (uint32_t)d2 & M;
  d3 += c; c = d3 >> 26; p.h[3] = (uint32_t)d3 & M;
  d4 += c; c = d4 >> 26; p.h[4] = (uint32_t)d4 & M;
  const uint64_t e = (uint64_t)p.h[0] + c * 5u;  // c < 2^34
  p.h[0] = (uint32_t)e & M;
  p.h[1] += (uint32_t)(e >> 26);  // < 2^10
}

// tag = ((h mod 2^130 - 5) + s) mod 2^128 as 4 little-endian words
P3G_HP void poly1305_finish(const Poly1305& p, uint32_t tag[4]) {
  constexpr uint32_t M = 0x3ffffffu;
  uint32_t h[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) h[i] = p.h[i];
  // two carry passes: after the first h[0] < 2^26 + 5 and h[1..4] < 2^26; after the second every
  // limb is below 2^26 (a carry out of h[4] in the second pass leaves h[1..4] zero and h[0] tiny)
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      h[i] += c;
      c = h[i] >> 26;
      h[i] &= M;
    }
    h[0] += 5u * c;
  }
  // g = h + 5 - 2^130: its sign says whether h >= p; the subtraction is a select
  uint32_t g[5], c = 5u;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    g[i] = h[i] + c;
    c = g[i] >> 26;
    g[i] &= M;
  }
  const uint32_t take = 0u - c;  // c = 1 iff h + 5 >= 2^130, i.e. h >= p
#pragma unroll
  for (int i = 0; i < 5; ++i) h[i] = (h[i] & ~take) | (g[i] & take);
  const uint32_t w0 = h[0] | (h[1] << 26);
  const uint32_t w1 = (h[1] >> 6) | (h[2] << 20);
  const uint32_t w2 = (h[2] >> 12) | (h[3] << 14);
  const uint32_t w3 = (h[3] >> 18) | (h[4] << 8);
  uint64_t f = (uint64_t)w0 + p.s[0];
  tag[0] = (uint32_t)f;
  f = (uint64_t)w1 + p.s[1] + (f >> 32);
  tag[1] = (uint32_t)f;
  f = (uint64_t)w2 + p.s[2] + (f >> 32);
  tag[2] = (uint32_t)f;
  f = (uint64_t)w3 + p.s[3] + (f >> 32);
  tag[3] = (uint32_t)f;
}

// The MAC of a whole message (RFC 8439 §2.5.1): 16-byte blocks with the 2^128 bit, a shorter last
// block with a 0x01 byte after its end.
P3G_HP void poly1305_mac(const uint32_t k[8], const uint8_t* msg, uint64_t len, uint32_t tag[4]) {
  Poly1305 p;
  poly1305_init(p, k);
  for (uint64_t o = 0; o < len; o += 16) {
    const uint64_t rem = len - o;
    uint32_t d[4];
    load_block(msg + o, rem, d);
#pragma unroll
    for (int i = 0; i < 4; ++i)  // rem < 16: the 0x01 byte after the end
      d[i] |= (rem < 16 && (uint64_t)i == (rem >> 2)) ? 1u << (8 * (rem & 3)) : 0u;
    poly1305_block(p, d, rem < 16 ? 0u : 1u << 24);
  }
  poly1305_finish(p, tag);
}

// ------------------------------------------------------------------------------------------------
// AEAD_CHACHA20_POLY1305 open (RFC 8439 §2.8).  key 8 and nonce 3 little-endian words; aad and ct
// are byte sources (len(), block(o, d)); tag = 16 bytes as block words.  The one-time Poly1305 key
// is the first half of the block with counter 0; the MAC covers pad16(aad) || pad16(ct) ||
// len(aad) || len(ct), both lengths LE64 (a source's block() is zero past its end, which is the
// padding).  The tag is compared with no early exit before any byte is decrypted; on a mismatch
// pt[0 .. ct.len()) is zeroed and false returned, otherwise the plaintext (counter 1 onwards)
// is written there.
// ------------------------------------------------------------------------------------------------
template <class Aad, class Ct>
P3G_HP bool chacha20poly1305_open(const uint32_t key[8], const uint32_t nonce[3], const Aad& aad,
                                  const Ct& ct, const uint32_t tag[4], uint8_t* pt) {
  uint32_t ks[16], d[4], t[4];
  chacha20_block(key, 0u, nonce, ks);
  Poly1305 mac;
  poly1305_init(mac, ks);
  const uint64_t alen = aad.len(), clen = ct.len();
  for (uint64_t o = 0; o < alen; o += 16) {
    aad.block(o, d);
    poly1305_block(mac, d, 1u << 24);
  }
  for (uint64_t o = 0; o < clen; o += 16) {
    ct.block(o, d);
    poly1305_block(mac, d, 1u << 24);
  }
  d[0] = (uint32_t)alen; d[1] = (uint32_t)(alen >> 32);
  d[2] = (uint32_t)clen; d[3] = (uint32_t)(clen >> 32);
  poly1305_block(mac, d, 1u << 24);
  poly1305_finish(mac, t);
  uint32_t diff = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) diff |= t[i] ^ tag[i];  // no early exit
  if (diff != 0u) {
    for (uint64_t j = 0; j < clen; ++j) pt[j] = 0;
    return false;
  }
  for (uint64_t o = 0; o < clen; o += 64) {
    chacha20_block(key, (uint32_t)(o >> 6) + 1u, nonce, ks);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint64_t oo = o + 16 * q;
      if (oo < clen) {
        ct.block(oo, d);
#pragma unroll
        for (int j = 0; j < 16; ++j)
          if (oo + j < clen)
            pt[oo + j] = (uint8_t)((d[j >> 2] ^ ks[4 * q + (j >> 2)]) >> (8 * (j & 3)));
      }
    }
  }
  return true;
}

// The first min(rem, 16) bytes of block words c to p: four word stores where p is word-aligned and
// the block whole, byte stores otherwise (the choice depends on the address and the length only).
P3G_HP void store_block(uint8_t* p, uint64_t rem, const uint32_t c[4]) {
  if (rem >= 16 && ((uintptr_t)p & 3u) == 0) {
    __builtin_memcpy(__builtin_assume_aligned(p, 4), c, 16);
    return;
  }
#pragma unroll
  for (int j = 0; j < 16; ++j)
    if ((uint64_t)j < rem) p[j] = (uint8_t)(c[j >> 2] >> (8 * (j & 3)));
}

// c &= the first min(rem, 16) bytes: what enters a MAC of a short last block is zero past its end
P3G_HP void mask_block(uint32_t c[4], uint64_t rem) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint64_t lo = 4u * (uint64_t)i;
    c[i] &= rem >= lo + 4 ? 0xffffffffu : rem <= lo ? 0u : (1u << (8 * (uint32_t)(rem - lo))) - 1u;
  }
}

// ------------------------------------------------------------------------------------------------
// AEAD_CHACHA20_POLY1305 seal (RFC 8439 §2.8), the mirror of the open: key 8 and nonce 3
// little-endian words; aad and pt are byte sources.  ct gets pt.len() ciphertext bytes and the
// 16-byte tag.  One pass over the plaintext: each 16-byte piece is XORed with the keystream
// (counter 1 onwards), stored, and absorbed by the MAC (zero past the end of a short last piece);
// the MAC covers pad16(aad) || pad16(ct) || len(aad) || len(ct) under the one-time key of block 0.
// ------------------------------------------------------------------------------------------------
template <class Aad, class Pt>
P3G_HP void chacha20poly1305_seal(const uint32_t key[8], const uint32_t nonce[3], const Aad& aad,
                                  const Pt& pt, uint8_t* ct) {
  uint32_t ks[16], d[4], t[4];
  chacha20_block(key, 0u, nonce, ks);
  Poly1305 mac;
  poly1305_init(mac, ks);
  const uint64_t alen = aad.len(), plen = pt.len();
  for (uint64_t o = 0; o < alen; o += 16) {
    aad.block(o, d);
    poly1305_block(mac, d, 1u << 24);
  }
  for (uint64_t o = 0; o < plen; o += 64) {
    chacha20_block(key, (uint32_t)(o >> 6) + 1u, nonce, ks);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint64_t oo = o + 16 * q;
      if (oo < plen) {
        pt.block(oo, d);
#pragma unroll
        for (int i = 0; i < 4; ++i) d[i] ^= ks[4 * q + i];
        mask_block(d, plen - oo);
        store_block(ct + oo, plen - oo, d);
        poly1305_block(mac, d, 1u << 24);
      }
    }
  }
  d[0] = (uint32_t)alen; d[1] = (uint32_t)(alen >> 32);
  d[2] = (uint32_t)plen; d[3] = (uint32_t)(plen >> 32);
  poly1305_block(mac, d, 1u << 24);
  poly1305_finish(mac, t);
  store_block(ct + plen, 16, t);
}

}  // namespace p3g
