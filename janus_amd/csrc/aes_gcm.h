// AES-128-GCM / AES-256-GCM for one lane of the GPU HPKE open and seal (FIPS 197; NIST SP 800-38D):
//   aes_sbox_fill                     the S-box, computed (inverse in GF(2^8) + affine map)
//   aes_expand, aes_encrypt           key schedule and one block, S-box lookups only
//   ghash_step, ghash_bytes           GHASH, bit-serial, over hpke_prims.h's byte-source interface
//   aes_gcm_open, aes_gcm_seal        the AEAD, with the contracts of chacha20poly1305_open / _seal
// Free of HIP like hpke_prims.h: the kernels and a CPU test (tests/native/hpke_lane_host.cpp) run
// the same text.  rotr32, bswap32 and DEVI are sha256.h's.
#pragma once
#include "hpke_prims.h"
#include "sha256.h"

namespace p3g {

// ------------------------------------------------------------------------------------------------
// AES-128 / AES-256 (FIPS 197; NK = 4 / 8 key words, NK + 6 rounds) with the S-box in memory the
// caller provides (LDS in the kernels, computed by the block: inverse in GF(2^8) + affine map), and
// GHASH bit-serial (SP 800-38D §6.3): X25519 dominates the open, so the simplest forms.
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

// sbox[x] for x = first, first + step, ...: a block's threads fill it together, each passing
// (threadIdx.x, blockDim.x), and synchronise afterwards; (0, 1) fills all of it.
DEVI void aes_sbox_fill(uint8_t* sbox, uint32_t first, uint32_t step) {
  for (uint32_t x = first; x < 256u; x += step) {
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

// ------------------------------------------------------------------------------------------------
// AES-GCM with a 96-bit nonce (SP 800-38D §7).  key_be NK and nonce_be 3 big-endian words (as the
// key schedule gives them); aad, ct and pt are byte sources (len(), block(o, d)); a tag is 16 bytes
// as block words.  What the open and the seal share is written once: aes_gcm_start (round keys,
// H = E(K, 0), the GHASH of the AAD, the counter block's nonce) and aes_gcm_tag (the length block
// and the J0 mask).  The text is encrypted from counter 2 (J0 = nonce || 1 masks the tag).
// ------------------------------------------------------------------------------------------------
template <int NK, class Aad>
DEVI void aes_gcm_start(const uint8_t* sbox, const uint32_t* key_be, const uint32_t nonce_be[3],
                        const Aad& aad, uint32_t* rk, uint32_t h[4], uint32_t y[4],
                        uint32_t ctr[4]) {
  aes_expand<NK>(sbox, key_be, rk);
  const uint32_t zero[4] = {0, 0, 0, 0};
  uint32_t hle[4];
  aes_encrypt<NK>(sbox, rk, zero, hle);  // H = E(K, 0)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    h[i] = bswap32(hle[i]);
    y[i] = 0;
  }
  ghash_bytes(y, h, aad);
#pragma unroll
  for (int i = 0; i < 3; ++i) ctr[i] = bswap32(nonce_be[i]);
  ctr[3] = 0;
}

// tag = GHASH(pad16(aad) || pad16(ct) || len(aad) || len(ct)) ^ E(K, J0), y holding the GHASH so far
template <int NK>
DEVI void aes_gcm_tag(const uint8_t* sbox, const uint32_t* rk, const uint32_t h[4], uint32_t y[4],
                      uint32_t ctr[4], uint64_t alen, uint64_t clen, uint32_t tag[4]) {
  const uint64_t abits = alen * 8, cbits = clen * 8;
  const uint32_t lens[4] = {(uint32_t)(abits >> 32), (uint32_t)abits, (uint32_t)(cbits >> 32),
                            (uint32_t)cbits};
  ghash_step(y, lens, h);
  uint32_t ek[4];
  ctr[3] = bswap32(1u);  // J0 = nonce || 1
  aes_encrypt<NK>(sbox, rk, ctr, ek);
#pragma unroll
  for (int i = 0; i < 4; ++i) tag[i] = bswap32(y[i]) ^ ek[i];
}

// The open: the tag is compared with no early exit before any byte is decrypted; on a mismatch
// pt[0 .. ct.len()) is zeroed and false returned, otherwise the plaintext is written there.
template <int NK, class Aad, class Ct>
DEVI bool aes_gcm_open(const uint8_t* sbox, const uint32_t* key_be, const uint32_t nonce_be[3],
                       const Aad& aad, const Ct& ct, const uint32_t tag[4], uint8_t* pt) {
  uint32_t rk[4 * (NK + 7)], h[4], y[4], ctr[4], t[4];
  aes_gcm_start<NK>(sbox, key_be, nonce_be, aad, rk, h, y, ctr);
  ghash_bytes(y, h, ct);
  const uint64_t clen = ct.len();
  aes_gcm_tag<NK>(sbox, rk, h, y, ctr, aad.len(), clen, t);
  uint32_t diff = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) diff |= t[i] ^ tag[i];  // no early exit
  if (diff != 0u) {
    for (uint64_t j = 0; j < clen; ++j) pt[j] = 0;
    return false;
  }
  for (uint64_t o = 0; o < clen; o += 16) {
    uint32_t d[4], ek[4];
    ct.block(o, d);
    ctr[3] = bswap32((uint32_t)(o >> 4) + 2u);
    aes_encrypt<NK>(sbox, rk, ctr, ek);
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (o + j < clen) pt[o + j] = (uint8_t)((d[j >> 2] ^ ek[j >> 2]) >> (8 * (j & 3)));
  }
  return true;
}

// The seal: ct gets pt.len() ciphertext bytes and the 16-byte tag.  One pass over the plaintext:
// each 16-byte piece is XORed with the keystream, masked past the end of a short last piece,
// stored, and absorbed by GHASH.
template <int NK, class Aad, class Pt>
DEVI void aes_gcm_seal(const uint8_t* sbox, const uint32_t* key_be, const uint32_t nonce_be[3],
                       const Aad& aad, const Pt& pt, uint8_t* ct) {
  uint32_t rk[4 * (NK + 7)], h[4], y[4], ctr[4], t[4];
  aes_gcm_start<NK>(sbox, key_be, nonce_be, aad, rk, h, y, ctr);
  const uint64_t plen = pt.len();
  for (uint64_t o = 0; o < plen; o += 16) {
    uint32_t d[4], ek[4], x[4];
    pt.block(o, d);
    ctr[3] = bswap32((uint32_t)(o >> 4) + 2u);
    aes_encrypt<NK>(sbox, rk, ctr, ek);
#pragma unroll
    for (int i = 0; i < 4; ++i) d[i] ^= ek[i];
    mask_block(d, plen - o);
    store_block(ct + o, plen - o, d);
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = bswap32(d[i]);
    ghash_step(y, x, h);
  }
  aes_gcm_tag<NK>(sbox, rk, h, y, ctr, aad.len(), plen, t);
  store_block(ct + plen, 16, t);
}

}  // namespace p3g
