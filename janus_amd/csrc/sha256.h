// SHA-256 (FIPS 180-4), one compression at a time: the report-ID checksum of prio3_kernels.h and
// the HKDF-SHA256 / HMAC of hpke_kdf256.h and p256_kem.h chain it.  Device code under hipcc; a plain
// C++ compiler gets the same functions as host code (DEVI is `inline`, the round constants a
// constexpr table, the rotation two shifts), so the per-lane HPKE headers built on it (x25519.h,
// hpke_kdf256.h, aes_gcm.h, hpke_lane.h, p256_kem.h) run in CPU tests too.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#ifndef DEVI
#define DEVI __device__ __forceinline__
#endif
#else
#define DEVI inline
#endif

namespace p3g {

// An inline variable: every translation unit that hashes carries the table in its own code
// object, and the host side gets no shadow of it.  Not `static`: the compiler then folds the 64
// words into the hashing kernels as literals, which changes their registers and spills.
#if defined(__HIPCC__)
inline __constant__ uint32_t kSha256K[64] = {
#else
constexpr uint32_t kSha256K[64] = {
#endif
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
    0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
    0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
    0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
    0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
    0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
    0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
    0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};

#if defined(__HIPCC__)
DEVI uint32_t rotr32(uint32_t x, uint32_t n) { return __builtin_amdgcn_alignbit(x, x, n); }
#else
DEVI uint32_t rotr32(uint32_t x, uint32_t n) { return (x >> n) | (x << (32 - n)); }  // 0 < n < 32
#endif
DEVI uint32_t bswap32(uint32_t x) { return __builtin_bswap32(x); }

DEVI void sha256_iv(uint32_t h[8]) {
  h[0] = 0x6a09e667; h[1] = 0xbb67ae85; h[2] = 0x3c6ef372; h[3] = 0xa54ff53a;
  h[4] = 0x510e527f; h[5] = 0x9b05688c; h[6] = 0x1f83d9ab; h[7] = 0x5be0cd19;
}

// One SHA-256 compression: h (8 big-endian state words) absorbs the 64-byte block given as 16
// big-endian words (w is consumed as the message schedule).  Multi-block messages and HMAC
// (hpke_kdf256.h) chain it; fully unrolled, so constant block words fold away.
DEVI void sha256_compress(uint32_t h[8], uint32_t w[16]) {
  const uint32_t iv[8] = {h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7]};
  uint32_t a = iv[0], b = iv[1], c = iv[2], d = iv[3], e = iv[4], f = iv[5], g = iv[6], hh = iv[7];
#pragma unroll
  for (int t = 0; t < 64; ++t) {
    uint32_t wt;
    if (t < 16) {
      wt = w[t];
    } else {
      const uint32_t w15 = w[(t + 1) & 15], w2 = w[(t + 14) & 15];
      const uint32_t s0 = rotr32(w15, 7) ^ rotr32(w15, 18) ^ (w15 >> 3);
      const uint32_t s1 = rotr32(w2, 17) ^ rotr32(w2, 19) ^ (w2 >> 10);
      wt = w[t & 15] = w[t & 15] + s0 + w[(t + 9) & 15] + s1;
    }
    const uint32_t S1 = rotr32(e, 6) ^ rotr32(e, 11) ^ rotr32(e, 25);
    const uint32_t ch = (e & f) ^ (~e & g);
    const uint32_t t1 = hh + S1 + ch + kSha256K[t] + wt;
    const uint32_t S0 = rotr32(a, 2) ^ rotr32(a, 13) ^ rotr32(a, 22);
    const uint32_t mj = (a & b) ^ (a & c) ^ (b & c);
    const uint32_t t2 = S0 + mj;
    hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
  }
  h[0] = iv[0] + a; h[1] = iv[1] + b; h[2] = iv[2] + c; h[3] = iv[3] + d;
  h[4] = iv[4] + e; h[5] = iv[5] + f; h[6] = iv[6] + g; h[7] = iv[7] + hh;
}

// SHA-256 of a 16-byte message (one padded block): h = digest as 8 big-endian state words.
DEVI void sha256_16(const uint8_t* m, uint32_t h[8]) {
  uint32_t w[16];
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = bswap32(*reinterpret_cast<const uint32_t*>(m + 4 * i));
  w[4] = 0x80000000u;
#pragma unroll
  for (int i = 5; i < 15; ++i) w[i] = 0u;
  w[15] = 128u;  // message length in bits
  sha256_iv(h);
  sha256_compress(h, w);
}

}  // namespace p3g
