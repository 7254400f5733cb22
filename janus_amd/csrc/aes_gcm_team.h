// AES-GCM opened by a team of lanes (one wave per report in hpke_open_team.h's kernels), for
// ciphertexts far longer than one lane should walk: the leader's input shares at upload.  CTR is
// parallel over blocks and GHASH is parallel over blocks through powers of H (NIST SP 800-38D
// §6.4), so lane l of a team of T takes blocks l, l + T, ... -- a stripe of T consecutive 16-byte
// blocks is one contiguous load per lane.
//   gf128_mul                         a product in GF(2^128), GCM bit order, bit-serial
//   gf128_powers_step                 the table H^1 .. H^T by doubling, log2 T products per lane
//   gcm_team_power, gcm_team_stripe   one lane's share of GHASH and of the CTR decryption
//   gcm_team_join                     the GHASH of the whole ciphertext from the lanes' XOR
//   gcm_team_stripe_range, gcm_team_seal_stripe_range, gf128_pow, gcm_split_join
//                                     the same over a sub-range of the blocks, and the GHASH of a
//                                     text from its segments' sums (several waves per report)
//   gcm_team_wipe, team_zero          zeros where a report failed, and in a slot's tail
//   PackedSink, ShareSink             where the plaintext goes: a packed slot, or a share row with
//                                     the PlaintextInputShare header checked and dropped
//   gcm_team_seal_stripe              the seal's stripe (hpke_seal_team.h's kernels): a plaintext
//                                     source encrypted, stored and then absorbed by GHASH
//   store_block_any, CtSink           where the ciphertext goes: a slot at any alignment
// Written per lane, with the lane index and the team size as parameters.  What crosses lanes is the
// caller's: the table lives in memory the team shares (LDS; ordered between steps by the caller),
// the lanes' accumulators are XORed by the caller, and every lane then computes the same tag.
// Round keys, H, the AAD's GHASH and the tag mask are aes_gcm.h's aes_gcm_start / aes_gcm_tag,
// unchanged, computed alike by every lane.  Free of HIP like aes_gcm.h: the kernels and a CPU test
// (tests/native/aes_gcm_team_host.cpp, 64 lanes in a loop) run the same text.
// No branch and no global-memory address depends on a key-derived value: the table is indexed by
// block counts only, and the products are the masked bit-serial form of ghash_step.
#pragma once
#include "aes_gcm.h"

namespace p3g {

// out = a * b in GF(2^128), GCM bit order; all as four big-endian words (ghash_step(y, x, h) is
// gf128_mul(y ^ x, h)).  out may be a or b.
DEVI void gf128_mul(const uint32_t a[4], const uint32_t b[4], uint32_t out[4]) {
  uint32_t v0 = b[0], v1 = b[1], v2 = b[2], v3 = b[3];
  uint32_t z0 = 0, z1 = 0, z2 = 0, z3 = 0;
#pragma unroll
  for (int wd = 0; wd < 4; ++wd) {
    uint32_t xb = a[wd];
#pragma unroll 4
    for (int bit = 0; bit < 32; ++bit) {
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
  out[0] = z0; out[1] = z1; out[2] = z2; out[3] = z3;
}

// The table of powers, tbl[4 e .. 4 e + 4) = H^(e + 1) for e < team (a power of two): entry 0 is H,
// and the step `half` = 1, 2, 4, ..., team / 2 fills entries half .. 2 half - 1 from the entries
// below: lane l in that range sets entry l = entry (l - half) * entry (half - 1).  Every lane
// multiplies; a step reads entries below `half` only and writes entries from `half` up, and the
// caller orders each step's writes before the next step's reads.
DEVI void gf128_powers_step(uint32_t* tbl, uint32_t lane, uint32_t half) {
  const bool mine = lane >= half && lane < 2 * half;
  uint32_t p[4];
  gf128_mul(tbl + 4 * (mine ? lane - half : 0u), tbl + 4 * (half - 1), p);
  if (mine) {
#pragma unroll
    for (int i = 0; i < 4; ++i) tbl[4 * lane + i] = p[i];
  }
}

// The power a lane multiplies by once it has absorbed block b of nb: H^team while a later block of
// its own follows, else H^(nb - b), which carries its sum to the end of the ciphertext.
DEVI const uint32_t* gcm_team_power(const uint32_t* tbl, uint64_t b, uint64_t nb, uint32_t team) {
  const uint64_t d = nb - b;
  return tbl + 4 * ((d > team ? (uint64_t)team : d) - 1);
}

// 16 bytes at p (any alignment) as block words
DEVI void load_block16(const uint8_t* p, uint32_t d[4]) { __builtin_memcpy(d, p, 16); }

// One lane's stripe of the blocks [b0, b1) of a ciphertext of clen bytes (nb = ceil(clen / 16)
// blocks, the last one zero-padded; b1 <= nb): blocks b0 + lane, b0 + lane + team, ...  Block
// indices are the ciphertext's own, so the counter, the offsets and the padding are those of the
// whole text.  With GHASH, acc (zero on entry) absorbs them as acc = (acc ^ X_b) * power(b), the
// power carrying to b1; block 0 also takes y0, the GHASH of the AAD, so the XOR of all lanes' acc
// is sum_b X_b H^(b1 - b): for [0, nb) the GHASH of pad16(aad) || pad16(ct).  With CTR, block b is
// XORed with E(K, nonce || b + 2) (ctr is aes_gcm_start's; its last word is not read) and handed
// to sink.put(b, words, bytes): all sixteen bytes, or the partial last block's.  The counter is 32
// bits wide: a text of more than 2^32 - 2 blocks would wrap it, which no caller can reach (the
// share rows' length is a u32 of bytes, the packed slots' far below).
template <int NK, bool GHASH, bool CTR, class Sink>
DEVI void gcm_team_stripe_range(const uint8_t* sbox, const uint32_t* rk, const uint32_t ctr[4],
                                const uint32_t* tbl, const uint32_t y0[4], const uint8_t* ct,
                                uint64_t clen, uint64_t b0, uint64_t b1, uint32_t lane,
                                uint32_t team, uint32_t acc[4], Sink& sink) {
  for (uint64_t b = b0 + lane; b < b1; b += team) {
    const uint64_t o = 16 * b, rem = clen - o;
    uint32_t d[4];
    if (rem >= 16) load_block16(ct + o, d);
    else load_block(ct + o, rem, d);
    if constexpr (GHASH) {
      uint32_t x[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) x[i] = bswap32(d[i]) ^ acc[i] ^ (b == 0 ? y0[i] : 0u);
      gf128_mul(x, gcm_team_power(tbl, b, b1, team), acc);
    }
    if constexpr (CTR) {
      const uint32_t c[4] = {ctr[0], ctr[1], ctr[2], bswap32((uint32_t)b + 2u)};
      uint32_t ek[4];
      aes_encrypt<NK>(sbox, rk, c, ek);
#pragma unroll
      for (int i = 0; i < 4; ++i) d[i] ^= ek[i];
      sink.put(b, d, rem < 16 ? (uint32_t)rem : 16u);
    }
  }
}

// The whole ciphertext: gcm_team_stripe_range over [0, nb).
template <int NK, bool GHASH, bool CTR, class Sink>
DEVI void gcm_team_stripe(const uint8_t* sbox, const uint32_t* rk, const uint32_t ctr[4],
                          const uint32_t* tbl, const uint32_t y0[4], const uint8_t* ct,
                          uint64_t clen, uint32_t lane, uint32_t team, uint32_t acc[4],
                          Sink& sink) {
  gcm_team_stripe_range<NK, GHASH, CTR>(sbox, rk, ctr, tbl, y0, ct, clen, 0, (clen + 15) / 16,
                                        lane, team, acc, sink);
}

// The sixteen bytes at offset o of a byte source, all of which exist: the source's own whole-block
// form where it has one (whole(o, d): one 16-byte load), else block(o, d).
template <class Src>
DEVI auto src_whole_block(const Src& s, uint64_t o, uint32_t d[4], int) -> decltype(s.whole(o, d)) {
  s.whole(o, d);
}
template <class Src>
DEVI void src_whole_block(const Src& s, uint64_t o, uint32_t d[4], long) {
  s.block(o, d);
}

// The seal's mirror of gcm_team_stripe_range: one lane's stripe of the blocks [b0, b1) of a
// plaintext, a byte source (len(), block(o, d)) of nb = ceil(len / 16) blocks (b1 <= nb).  Block
// b = b0 + lane, b0 + lane + team, ... is XORed with E(K, nonce || b + 2), zeroed past the end of
// a partial last block, handed to sink.put(b, words, bytes) and then absorbed:
// acc = (acc ^ C_b [^ y0 when b == 0]) * power(b), so the XOR of all lanes' acc (zero on entry) is
// sum_b C_b H^(b1 - b): for [0, nb) the GHASH of pad16(aad) || pad16(ciphertext).
template <int NK, class Src, class Sink>
DEVI void gcm_team_seal_stripe_range(const uint8_t* sbox, const uint32_t* rk,
                                     const uint32_t ctr[4], const uint32_t* tbl,
                                     const uint32_t y0[4], const Src& pt, uint64_t b0, uint64_t b1,
                                     uint32_t lane, uint32_t team, uint32_t acc[4], Sink& sink) {
  const uint64_t plen = pt.len();
  for (uint64_t b = b0 + lane; b < b1; b += team) {
    const uint64_t o = 16 * b, rem = plen - o;
    uint32_t d[4], ek[4], x[4];
    if (rem >= 16) src_whole_block(pt, o, d, 0);
    else pt.block(o, d);
    const uint32_t c[4] = {ctr[0], ctr[1], ctr[2], bswap32((uint32_t)b + 2u)};
    aes_encrypt<NK>(sbox, rk, c, ek);
#pragma unroll
    for (int i = 0; i < 4; ++i) d[i] ^= ek[i];
    mask_block(d, rem);
    sink.put(b, d, rem < 16 ? (uint32_t)rem : 16u);
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = bswap32(d[i]) ^ acc[i] ^ (b == 0 ? y0[i] : 0u);
    gf128_mul(x, gcm_team_power(tbl, b, b1, team), acc);
  }
}

// The whole plaintext: gcm_team_seal_stripe_range over [0, nb).
template <int NK, class Src, class Sink>
DEVI void gcm_team_seal_stripe(const uint8_t* sbox, const uint32_t* rk, const uint32_t ctr[4],
                               const uint32_t* tbl, const uint32_t y0[4], const Src& pt,
                               uint32_t lane, uint32_t team, uint32_t acc[4], Sink& sink) {
  gcm_team_seal_stripe_range<NK>(sbox, rk, ctr, tbl, y0, pt, 0, (pt.len() + 15) / 16, lane, team,
                                 acc, sink);
}

// y = the GHASH so far, given sum = the XOR of every lane's acc: sum itself, or y0 when there was
// no block to carry it.
DEVI void gcm_team_join(uint32_t y[4], const uint32_t sum[4], const uint32_t y0[4], uint64_t clen) {
#pragma unroll
  for (int i = 0; i < 4; ++i) y[i] = clen ? sum[i] : y0[i];
}

// out = a^e in GF(2^128) for a public exponent e (e = 0 gives 1, the block 80 00 .. 00):
// square-and-multiply from bit 31 down with the multiplication selected, not branched on --
// sixty-four products whatever e is.  The exponents are block counts.
DEVI void gf128_pow(const uint32_t a[4], uint32_t e, uint32_t out[4]) {
  uint32_t acc[4] = {0x80000000u, 0u, 0u, 0u};
#pragma unroll 1
  for (int bit = 31; bit >= 0; --bit) {
    uint32_t t[4];
    gf128_mul(acc, acc, acc);
    gf128_mul(acc, a, t);
    const uint32_t m = 0u - ((e >> bit) & 1u);
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = (acc[i] & ~m) | (t[i] & m);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) out[i] = acc[i];
}

// A text of nb blocks cut into S >= 2 segments of L blocks (the last one shorter: plan_hpke.h's
// team_split_plan), each segment's sum P_s = sum_b X_b H^(end_s - b) carried to its own end
// (gcm_team_stripe_range's XOR over the lanes, y0 inside P_0) at parts[pitch s ..]: y = the GHASH
// so far of the whole text, by Horner over the segments,
//   y = (..((P_0 H^L ^ P_1) H^L ^ P_2)..) H^(nb - (S - 1) L) ^ P_(S-1),
// two exponentiations and S - 1 products.  L and nb are below 2^32 (gcm_team_stripe_range).
DEVI void gcm_split_join(const uint32_t h[4], const uint32_t* parts, uint32_t pitch, uint32_t S,
                         uint64_t L, uint64_t nb, uint32_t y[4]) {
  uint32_t hl[4], hlast[4];
  gf128_pow(h, (uint32_t)L, hl);
  gf128_pow(h, (uint32_t)(nb - (uint64_t)(S - 1) * L), hlast);
#pragma unroll
  for (int i = 0; i < 4; ++i) y[i] = parts[i];
  for (uint32_t s = 1; s < S; ++s) {
    uint32_t pw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) pw[i] = s + 1 == S ? hlast[i] : hl[i];
    gf128_mul(y, pw, y);
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] ^= parts[(size_t)pitch * s + i];
  }
}

// An AAD that only the first segment of a split text absorbs: the source itself there, an empty
// one (y0 = 0, which no later segment's blocks take) elsewhere.  len() is the absorbed length; the
// tag's length block takes the source's own.
template <class Aad>
struct FirstSegmentAad {
  const Aad& aad;
  bool first;
  DEVI uint64_t len() const { return first ? aad.len() : 0; }
  DEVI void block(uint64_t o, uint32_t d[4]) const { aad.block(o, d); }
};

// Zeros over what the lane's stripe wrote (sink.store with the stripe's own block-to-lane map, so
// a lane overwrites its own stores).
template <class Sink>
DEVI void gcm_team_wipe(Sink& sink, uint64_t clen, uint32_t lane, uint32_t team) {
  const uint32_t zero[4] = {0, 0, 0, 0};
  for (uint64_t o = 16 * (uint64_t)lane; o < clen; o += 16 * (uint64_t)team)
    sink.store(o >> 4, zero, clen - o < 16 ? (uint32_t)(clen - o) : 16u);
}

// p[0 .. n) = 0, by the whole team: sixteen bytes per lane and round.
DEVI void team_zero(uint8_t* p, uint64_t n, uint32_t lane, uint32_t team) {
  const uint32_t zero[4] = {0, 0, 0, 0};
  for (uint64_t o = 16 * (uint64_t)lane; o < n; o += 16 * (uint64_t)team)
    store_block(p + o, n - o, zero);
}

// The plaintext to a packed slot: block b at pt + 16 b.
struct PackedSink {
  uint8_t* pt;
  DEVI void store(uint64_t b, const uint32_t d[4], uint32_t n) { store_block(pt + 16 * b, n, d); }
  DEVI void put(uint64_t b, const uint32_t d[4], uint32_t n) { store(b, d, n); }
};

// The plaintext of a PlaintextInputShare to a share row: 00 00 | u32 BE slen | share.  The six
// header bytes (block 0's first) are compared, never stored, and bad set on the lane that holds
// them when they differ; plaintext byte p >= 6 goes to row[p - 6].  A block's sixteen bytes start
// ten bytes into a sixteen-byte piece of the row, so on a row aligned to 16 they leave as
// naturally aligned pieces of 2, 4, 8 and 2 bytes (block 0: 8 and 2); bytes otherwise.
struct ShareSink {
  uint8_t* row;
  uint32_t slen;
  uint32_t bad;
  DEVI void store(uint64_t b, const uint32_t d[4], uint32_t n) {
    if (n == 16 && ((uintptr_t)row & 15u) == 0) {
      uint8_t* q = row + 16 * b;  // the row piece that takes bytes 6 .. 15
      const uint32_t w1 = (d[0] >> 16) | (d[1] << 16);
      const uint32_t w2[2] = {(d[1] >> 16) | (d[2] << 16), (d[2] >> 16) | (d[3] << 16)};
      const uint16_t h0 = (uint16_t)d[0], h3 = (uint16_t)(d[3] >> 16);
      if (b) {
        __builtin_memcpy(__builtin_assume_aligned(q - 6, 2), &h0, 2);
        __builtin_memcpy(__builtin_assume_aligned(q - 4, 4), &w1, 4);
      }
      __builtin_memcpy(__builtin_assume_aligned(q, 8), w2, 8);
      __builtin_memcpy(__builtin_assume_aligned(q + 8, 2), &h3, 2);
      return;
    }
#pragma unroll
    for (uint32_t j = 0; j < 16; ++j) {
      const uint64_t p = 16 * b + j;
      if (j < n && p >= 6) row[p - 6] = (uint8_t)(d[j >> 2] >> (8 * (j & 3)));
    }
  }
  DEVI void put(uint64_t b, const uint32_t d[4], uint32_t n) {
    if (b == 0) {
      const uint32_t be = bswap32(slen);  // SharePlaintext's header words
      bad |= (d[0] ^ (be << 16)) | ((d[1] ^ (be >> 16)) & 0xffffu);
    }
    store(b, d, n);
  }
};

// The eight bytes from byte p (< 16) of a block on, as a little-endian value (zeros past byte 15).
DEVI uint64_t block_bytes_from(const uint32_t d[4], uint32_t p) {
  const uint64_t lo = d[0] | ((uint64_t)d[1] << 32), hi = d[2] | ((uint64_t)d[3] << 32);
  const uint32_t s = 8 * (p & 7u);
  const uint64_t mid = (lo >> s) | (s ? hi << (64 - s) : 0);  // p < 8
  return p < 8 ? mid : hi >> s;
}

// A block's sixteen bytes to a (any alignment) as the widest naturally aligned pieces the address
// allows: one 16-byte store on a 16-byte boundary; otherwise 1, 2, 4 and 8 bytes, those that
// 16 - (a mod 16) is made of, which end on the boundary, then from the boundary on 8, 4, 2 and 1
// bytes, those that a mod 16 is made of -- five stores at the most.
DEVI void store_block_any(uint8_t* a, const uint32_t d[4]) {
  const uint32_t k = (uint32_t)((uintptr_t)a & 15u);
  if (k == 0) {
    __builtin_memcpy(__builtin_assume_aligned(a, 16), d, 16);
    return;
  }
  uint32_t p = 0;
  if (k & 1u) {
    a[0] = (uint8_t)d[0];
    p = 1;
  }
  if ((k + p) & 2u) {
    const uint16_t v = (uint16_t)block_bytes_from(d, p);
    __builtin_memcpy(__builtin_assume_aligned(a + p, 2), &v, 2);
    p += 2;
  }
  if ((k + p) & 4u) {
    const uint32_t v = (uint32_t)block_bytes_from(d, p);
    __builtin_memcpy(__builtin_assume_aligned(a + p, 4), &v, 4);
    p += 4;
  }
  if ((k + p) & 8u) {
    const uint64_t v = block_bytes_from(d, p);
    __builtin_memcpy(__builtin_assume_aligned(a + p, 8), &v, 8);
    p += 8;
  }
  // a + p is the boundary and p = 16 - k: k bytes are left
  if (k & 8u) {
    const uint64_t v = block_bytes_from(d, p);
    __builtin_memcpy(__builtin_assume_aligned(a + p, 8), &v, 8);
    p += 8;
  }
  if (k & 4u) {
    const uint32_t v = (uint32_t)block_bytes_from(d, p);
    __builtin_memcpy(__builtin_assume_aligned(a + p, 4), &v, 4);
    p += 4;
  }
  if (k & 2u) {
    const uint16_t v = (uint16_t)block_bytes_from(d, p);
    __builtin_memcpy(__builtin_assume_aligned(a + p, 2), &v, 2);
    p += 2;
  }
  if (k & 1u) a[15] = (uint8_t)(d[3] >> 24);
}

// The ciphertext to a slot at any alignment (a packed slot at a byte offset, the payload column of
// a report matrix): block b at ct + 16 b, a whole block as store_block_any's pieces, the partial
// last block bytewise.  Only ct[16 b .. 16 b + n) is written.
struct CtSink {
  uint8_t* ct;
  DEVI void put(uint64_t b, const uint32_t d[4], uint32_t n) {
    uint8_t* a = ct + 16 * b;
    if (n == 16) {
      store_block_any(a, d);
      return;
    }
#pragma unroll
    for (uint32_t j = 0; j < 16; ++j)
      if (j < n) a[j] = (uint8_t)(d[j >> 2] >> (8 * (j & 3)));
  }
};

}  // namespace p3g
