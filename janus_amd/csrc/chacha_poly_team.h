// ChaCha20-Poly1305 (RFC 8439 §2.8) opened and sealed by a team of lanes (one wave per report in
// hpke_open_team.h's and hpke_seal_team.h's kernels), the third AEAD beside aes_gcm_team.h's.
// ChaCha20 is parallel over its 64-byte blocks and Poly1305 over its 16-byte blocks through powers
// of r, so lane l of a team of T takes the 64-byte chunks l, l + T, ... of the body (block counter
// = chunk index + 1): one chacha20_block per lane and trip, 64 contiguous bytes per lane.  (A
// 16-byte stripe as in the GCM team would have four lanes compute the same keystream block.)
//   poly1305_mul, poly1305_carry      a general product mod 2^130 - 5 and one carry pass
//   poly1305_pow                      r^e for a public e < 512: nine squarings, selects
//   poly_team_start                   a lane's MAC state: r, s, the AAD's hash, r^(4T - 3), r^d
//   poly_team_absorb                  one ciphertext block into the lane's sum
//   chacha_team_start                 the one-time key from block 0, then poly_team_start
//   chacha_team_stripe<SEAL>          one lane's chunks: load, [absorb,] XOR, store[, absorb]
//   poly_team_tag                     the tag from the joined sum, on every lane alike
//   poly_team_start_range, chacha_team_stripe_range, poly1305_pow64, poly_split_join
//                                     the same over a sub-range of the chunks, and the sum of a
//                                     body from its segments' sums (several waves per report)
//   chacha_team_wipe                  zeros over what the lane's stripe stored
// The MAC across lanes.  With h_a the state after the padded AAD, c_0 .. c_(nb-1) the zero-padded
// ciphertext blocks (each with the 2^128 bit: the AEAD pads to 16) and L the length block, the
// serial MAC is h = ((h_a r^nb + sum_b c_b r^(nb - b)) + L) r.  Lane 0 starts from h_a, the others
// from 0; after absorbing block b a lane multiplies by r^g, g the distance to the next block it
// absorbs or nb - b after its last: 1 inside a chunk, 4T - 3 from a chunk's last block to the
// lane's next chunk, and one d in [1, 4T - 3] per lane at its end.  The lanes' sums add up (mod
// 2^130 - 5) to T = h_a r^nb + sum_b c_b r^(nb - b); for nb = 0 that is lane 0's h_a.  Every lane
// then computes (T + L) r and poly1305_finish, unchanged.
// The exponents depend on lengths only, so the square-and-multiply (selects, no branch on its
// bits) is constant-time in the key; r, s, the powers, the key and the nonce stay in registers,
// and there is no table to zero.  What crosses lanes is the caller's: the sum of the lanes' limbs,
// which does not fit 32 bits (64 limbs below 2^26 + 2^10), so the caller adds eight lanes, runs
// poly1305_carry, adds the eight sums and carries again (poly1305_carry's comment has the bounds).
// Sinks and sources are aes_gcm_team.h's and hpke_lane.h's, unchanged.  Free of HIP: the kernels
// and a CPU test (tests/native/chacha_poly_team_host.cpp, 64 lanes in a loop) run the same text.
#pragma once
#include "aes_gcm_team.h"

namespace p3g {

// out = a b mod 2^130 - 5 on five 26-bit limbs, partly reduced.  Limb bounds: every limb of a and
// of b is below B = 2^27 + 2^10 (a sum of two values this function or poly1305_block returns, or
// such a value plus a message block).  Then 5 b[i] < 2^29.33 fits 32 bits, a product a[i] (5 b[j])
// is below 5 B^2 < 2^56.33 and a five-term column below 2^58.66; the carry out of a column is
// below 2^32.66, five times the last one below 2^35, so what returns to limb 1 is below 2^9.
// Result: out[0], out[2..4] < 2^26 and out[1] < 2^26 + 2^10, as after poly1305_block.  Products are
// (uint64_t)x * y + acc, one v_mad_u64_u32 each.  out may be a or b.
DEVI void poly1305_mul(const uint32_t a[5], const uint32_t b[5], uint32_t out[5]) {
  constexpr uint32_t M = 0x3ffffffu;
  const uint32_t a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], a4 = a[4];
  const uint32_t b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3], b4 = b[4];
  const uint32_t s1 = 5u * b1, s2 = 5u * b2, s3 = 5u * b3, s4 = 5u * b4;
  uint64_t d0 = (uint64_t)a0 * b0;
  d0 = (uint64_t)a1 * s4 + d0; d0 = (uint64_t)a2 * s3 + d0;
  d0 = (uint64_t)a3 * s2 + d0; d0 = (uint64_t)a4 * s1 + d0;
  uint64_t d1 = (uint64_t)a0 * b1;
  d1 = (uint64_t)a1 * b0 + d1; d1 = (uint64_t)a2 * s4 + d1;
  d1 = (uint64_t)a3 * s3 + d1; d1 = (uint64_t)a4 * s2 + d1;
  uint64_t d2 = (uint64_t)a0 * b2;
  d2 = (uint64_t)a1 * b1 + d2; d2 = (uint64_t)a2 * b0 + d2;
  d2 = (uint64_t)a3 * s4 + d2; d2 = (uint64_t)a4 * s3 + d2;
  uint64_t d3 = (uint64_t)a0 * b3;
  d3 = (uint64_t)a1 * b2 + d3; d3 = (uint64_t)a2 * b1 + d3;
  d3 = (uint64_t)a3 * b0 + d3; d3 = (uint64_t)a4 * s4 + d3;
  uint64_t d4 = (uint64_t)a0 * b4;
  d4 = (uint64_t)a1 * b3 + d4; d4 = (uint64_t)a2 * b2 + d4;
  d4 = (uint64_t)a3 * b1 + d4; d4 = (uint64_t)a4 * b0 + d4;
  uint64_t c = d0 >> 26;
  out[0] = (uint32_t)d0 & M;
  d1 += c; c = d1 >> 26; out[1] = (uint32_t)d1 & M;
  d2 += c; c = d2 >> 26; out[2] = (uint32_t)d2 & M;
  d3 += c; c = d3 >> 26; out[3] = (uint32_t)d3 & M;
  d4 += c; c = d4 >> 26; out[4] = (uint32_t)d4 & M;
  const uint64_t e = (uint64_t)out[0] + c * 5u;  // c < 2^33
  out[0] = (uint32_t)e & M;
  out[1] += (uint32_t)(e >> 26);  // < 2^9
}

// One carry pass over limbs that fit 32 bits: afterwards h[1..4] < 2^26 and h[0] < 2^26 + 2^9
// (the carry out of limb 4 is at most 2^6).  The lane join uses it twice: eight lanes' limbs, each
// below 2^26 + 2^10, sum to less than 2^29 + 2^13; carried, eight such sums add to less than
// 2^29 + 2^12; carried again, T's limbs are below 2^26 + 2^9 and T plus a length block is within
// poly1305_block's bound.  (Sixty-four limbs added without the carry between would pass 2^32.)
DEVI void poly1305_carry(uint32_t h[5]) {
  constexpr uint32_t M = 0x3ffffffu;
  uint32_t c = 0;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    h[i] += c;
    c = h[i] >> 26;
    h[i] &= M;
  }
  h[0] += 5u * c;
}

// out = r^e mod 2^130 - 5 for e < 512 (r's limbs within poly1305_mul's bound; e = 0 gives 1).
// Square-and-multiply from bit 8 down with the multiplication selected, not branched on: eighteen
// products whatever e is, so lanes with different exponents stay together.
DEVI void poly1305_pow(const uint32_t r[5], uint32_t e, uint32_t out[5]) {
  uint32_t acc[5] = {1u, 0u, 0u, 0u, 0u};
#pragma unroll 1
  for (int bit = 8; bit >= 0; --bit) {
    uint32_t t[5];
    poly1305_mul(acc, acc, acc);
    poly1305_mul(acc, r, t);
    const uint32_t m = 0u - ((e >> bit) & 1u);
#pragma unroll
    for (int i = 0; i < 5; ++i) acc[i] = (acc[i] & ~m) | (t[i] & m);
  }
#pragma unroll
  for (int i = 0; i < 5; ++i) out[i] = acc[i];
}

// out = r^e mod 2^130 - 5 for any public 64-bit e: poly1305_pow's square-and-multiply from bit 63
// down, 128 products whatever e is.  For the segments' join (poly_split_join), whose exponents are
// block counts.
DEVI void poly1305_pow64(const uint32_t r[5], uint64_t e, uint32_t out[5]) {
  uint32_t acc[5] = {1u, 0u, 0u, 0u, 0u};
#pragma unroll 1
  for (int bit = 63; bit >= 0; --bit) {
    uint32_t t[5];
    poly1305_mul(acc, acc, acc);
    poly1305_mul(acc, r, t);
    const uint32_t m = 0u - (uint32_t)((e >> bit) & 1u);
#pragma unroll
    for (int i = 0; i < 5; ++i) acc[i] = (acc[i] & ~m) | (t[i] & m);
  }
#pragma unroll
  for (int i = 0; i < 5; ++i) out[i] = acc[i];
}

// A lane's share of the MAC: mac.r and mac.s the one-time key, mac.h the lane's running sum, rs =
// r^(4 team - 3) (from a chunk's last block to the lane's next chunk) and rd = r^d, d = nb - b
// for the last block b of the lane's last chunk where that chunk is whole.
struct PolyTeam {
  Poly1305 mac;
  uint32_t rs[5], rd[5];
};

// The lane's state before its stripe of the chunks [c0, c1) of a body, whose blocks end at block
// b1 (c1 = ceil(b1 / 4); the whole body: c0 = 0 and b1 = nb), from the one-time key otk (r || s, 8
// little-endian words; r is clamped here) and the AAD.  With `first` (the range starts the body)
// every lane absorbs the padded AAD and lane 0 keeps that state as its sum; every other sum starts
// from zero, and a later range does not read the AAD.  The powers carry to b1, so the lanes' sums
// add up to [h_a r^b1 +] sum_b c_b r^(b1 - b) over the range's blocks.  team <= 64 (the exponents
// fit poly1305_pow); rs is computed only where some lane has a second chunk, and a lane without a
// whole last chunk gets rd = r (never used).  Both choices depend on lengths, lane and team only.
template <class Aad>
DEVI void poly_team_start_range(PolyTeam& t, const uint32_t otk[8], const Aad& aad, bool first,
                                uint64_t c0, uint64_t c1, uint64_t b1, uint32_t lane,
                                uint32_t team) {
  poly1305_init(t.mac, otk);
  if (first) {
    const uint64_t alen = aad.len();
    for (uint64_t o = 0; o < alen; o += 16) {
      uint32_t d[4];
      aad.block(o, d);
      poly1305_block(t.mac, d, 1u << 24);
    }
  }
#pragma unroll
  for (int i = 0; i < 5; ++i) t.mac.h[i] = first && lane == 0 ? t.mac.h[i] : 0u;
#pragma unroll
  for (int i = 0; i < 5; ++i) t.rs[i] = t.mac.r[i];
  if (c1 - c0 > team) poly1305_pow(t.mac.r, 4u * team - 3u, t.rs);
  uint32_t d = 1;
  if (c0 + lane < c1) {
    const uint64_t k0 = c0 + lane;
    const uint64_t last = k0 + team * ((c1 - 1 - k0) / team);    // the lane's last chunk
    if (4 * last + 3 < b1) d = (uint32_t)(b1 - (4 * last + 3));  // <= 4 team - 3
  }
  poly1305_pow(t.mac.r, d, t.rd);
}

// The whole body of `len` bytes: poly_team_start_range over every chunk.
template <class Aad>
DEVI void poly_team_start(PolyTeam& t, const uint32_t otk[8], const Aad& aad, uint64_t len,
                          uint32_t lane, uint32_t team) {
  poly_team_start_range(t, otk, aad, true, 0, (len + 63) / 64, (len + 15) / 16, lane, team);
}

// h += the sixteen bytes m as a number, with the 2^128 bit
DEVI void poly1305_add_block(uint32_t h[5], const uint32_t m[4]) {
  constexpr uint32_t M = 0x3ffffffu;
  h[0] += m[0] & M;
  h[1] += ((m[0] >> 26) | (m[1] << 6)) & M;
  h[2] += ((m[1] >> 20) | (m[2] << 12)) & M;
  h[3] += ((m[2] >> 14) | (m[3] << 18)) & M;
  h[4] += (m[3] >> 8) | (1u << 24);
}

// The lane's sum absorbs ciphertext block m (zero past the body's end), the q-th of its chunk:
// times r inside the chunk, and after the chunk's fourth block times rs when a later chunk of the
// lane's follows (`more`), else times rd.  A short last chunk ends with a block of q < 3 and so
// with r, which is r^(nb - b) there.
DEVI void poly_team_absorb(PolyTeam& t, const uint32_t m[4], int q, bool more) {
  if (q < 3) {
    poly1305_block(t.mac, m, 1u << 24);
    return;
  }
  uint32_t pw[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) pw[i] = more ? t.rs[i] : t.rd[i];
  poly1305_add_block(t.mac.h, m);
  poly1305_mul(t.mac.h, pw, t.mac.h);
}

// tag = the MAC of pad16(aad) || pad16(body) || LE64 alen || LE64 len, given sum = the lanes' sums
// added and carried (limbs below 2^26 + 2^9): (sum + L) r, then poly1305_finish.
DEVI void poly_team_tag(PolyTeam& t, const uint32_t sum[5], uint64_t alen, uint64_t len,
                        uint32_t tag[4]) {
#pragma unroll
  for (int i = 0; i < 5; ++i) t.mac.h[i] = sum[i];
  const uint32_t l[4] = {(uint32_t)alen, (uint32_t)(alen >> 32), (uint32_t)len,
                         (uint32_t)(len >> 32)};
  poly1305_block(t.mac, l, 1u << 24);
  poly1305_finish(t.mac, tag);
}

// poly_team_start under the one-time key of (key, nonce): the first half of the ChaCha20 block
// with counter 0.  key 8 and nonce 3 little-endian words.
template <class Aad>
DEVI void chacha_team_start(PolyTeam& t, const uint32_t key[8], const uint32_t nonce[3],
                            const Aad& aad, uint64_t len, uint32_t lane, uint32_t team) {
  uint32_t ks[16];
  chacha20_block(key, 0u, nonce, ks);
  poly_team_start(t, ks, aad, len, lane, team);
}

// One lane's stripe of the chunks [c0, c1) of a body, a byte source (len(), block(o, d),
// whole(o, d) where it has one): chunks c0 + lane, c0 + lane + team, ... of 64 bytes, c1 at most
// the body's chunk count.  Chunk and block indices are the body's own, so the counter, the offsets
// and the padding are those of the whole body.  A chunk's (up to) four blocks are loaded, the
// keystream block with counter chunk + 1 is computed, and block b = 4 chunk + q is
//   open (SEAL false): absorbed as it came, XORed, and handed to sink.put(b, words, bytes);
//   seal:              XORed, zeroed past the end of a partial last block, handed to sink.put and
//                      then absorbed.
// t is the lane's poly_team_start_range state for the same range; afterwards t.mac.h is the
// lane's sum.  (The counter is 32 bits wide, as RFC 8439's: 2^32 chunks are 256 GiB.)
template <bool SEAL, class Src, class Sink>
DEVI void chacha_team_stripe_range(PolyTeam& t, const uint32_t key[8], const uint32_t nonce[3],
                                   const Src& src, uint64_t c0, uint64_t c1, uint32_t lane,
                                   uint32_t team, Sink& sink) {
  const uint64_t len = src.len();
  for (uint64_t k = c0 + lane; k < c1; k += team) {
    uint32_t d[4][4], ks[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint64_t o = 64 * k + 16 * q;
      if (o + 16 <= len) {
        src_whole_block(src, o, d[q], 0);
      } else if (o < len) {
        src.block(o, d[q]);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) d[q][i] = 0;
      }
    }
    chacha20_block(key, (uint32_t)k + 1u, nonce, ks);
    const bool more = k + team < c1;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint64_t o = 64 * k + 16 * q;
      if (o < len) {
        const uint64_t rem = len - o;
        if constexpr (!SEAL) poly_team_absorb(t, d[q], q, more);
#pragma unroll
        for (int i = 0; i < 4; ++i) d[q][i] ^= ks[4 * q + i];
        if constexpr (SEAL) mask_block(d[q], rem);
        sink.put(o >> 4, d[q], rem < 16 ? (uint32_t)rem : 16u);
        if constexpr (SEAL) poly_team_absorb(t, d[q], q, more);
      }
    }
  }
}

// The whole body: chacha_team_stripe_range over every chunk, after poly_team_start.
template <bool SEAL, class Src, class Sink>
DEVI void chacha_team_stripe(PolyTeam& t, const uint32_t key[8], const uint32_t nonce[3],
                             const Src& src, uint32_t lane, uint32_t team, Sink& sink) {
  chacha_team_stripe_range<SEAL>(t, key, nonce, src, 0, (src.len() + 63) / 64, lane, team, sink);
}

// A body of nb blocks cut into S >= 2 segments of L blocks (L a multiple of 4 team; the last one
// shorter: plan_hpke.h's team_split_plan), each segment's sum P_s = [h_a r^L +] sum_b c_b
// r^(end_s - b) carried to its own end (the lanes' sums added and carried, limbs below
// 2^26 + 2^9) at parts[pitch s ..]: sum = h_a r^nb + sum_b c_b r^(nb - b), what poly_team_tag
// takes, by Horner over the segments,
//   sum = (..((P_0 r^L + P_1) r^L + P_2)..) r^(nb - (S - 1) L) + P_(S-1),
// two exponentiations and S - 1 products.  A product's limbs (below 2^26 + 2^10) plus a sum's
// stay within poly1305_carry's 32 bits; carried, they are within poly1305_mul's bound again and,
// at the end, within poly_team_tag's.
DEVI void poly_split_join(const uint32_t r[5], const uint32_t* parts, uint32_t pitch, uint32_t S,
                          uint64_t L, uint64_t nb, uint32_t sum[5]) {
  uint32_t rl[5], rlast[5];
  poly1305_pow64(r, L, rl);
  poly1305_pow64(r, nb - (uint64_t)(S - 1) * L, rlast);
#pragma unroll
  for (int i = 0; i < 5; ++i) sum[i] = parts[i];
  for (uint32_t s = 1; s < S; ++s) {
    uint32_t pw[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) pw[i] = s + 1 == S ? rlast[i] : rl[i];
    poly1305_mul(sum, pw, sum);
#pragma unroll
    for (int i = 0; i < 5; ++i) sum[i] += parts[(size_t)pitch * s + i];
    poly1305_carry(sum);
  }
}

// Zeros over what the lane's stripe stored (sink.store with the stripe's own block-to-lane map, so
// a lane overwrites its own stores: gcm_team_wipe's contract).
template <class Sink>
DEVI void chacha_team_wipe(Sink& sink, uint64_t len, uint32_t lane, uint32_t team) {
  const uint32_t zero[4] = {0, 0, 0, 0};
  for (uint64_t c = 64 * (uint64_t)lane; c < len; c += 64 * (uint64_t)team) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint64_t o = c + 16 * q;
      if (o < len) sink.store(o >> 4, zero, len - o < 16 ? (uint32_t)(len - o) : 16u);
    }
  }
}

}  // namespace p3g
