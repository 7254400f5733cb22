// Driver of tests/test_team_split.py: several waves per report (janus_amd/csrc/hpke_team_split.h's
// kernels) built for the host from the same text -- plan_hpke.h's team_split_plan, and the
// sub-range stripes, segment sums and joins of aes_gcm_team.h and chacha_poly_team.h.  A segment's
// 64 lanes are simulated in a loop, and what the kernel shells do across lanes and kernels (the XOR
// or the butterfly sum of the lanes' sums, the segment's sum to a scratch row, the join's verdict,
// the wipe of a failed row) is done here.  A text protocol on stdin / stdout, one answer line per
// command; byte strings are hex, "-" when empty, and every input is used from a heap block of
// exactly its length and every output written to one of exactly its length, so a sanitizer build
// sees any access past either.  A is the AEAD: 1 AES-128-GCM, 2 AES-256-GCM, 3 ChaCha20-Poly1305;
// L the segment length in blocks (S = ceil(nb / L) segments):
//   plan <n> <body> <unit> <cap> <min_blocks> <wave_slots>  -> "<S> <L>" of team_split_plan
//   pow64 <r: 16 bytes> <e>              -> the five limbs of poly1305_pow64(clamp(r), e), decimal
//   gfpow <h: 16 bytes> <k>              -> "<gf128_pow(h, 64 k)> <h multiplied 64 k times>"
//   sseal <A> <key> <nonce> <aad> <pt> <L>        -> ct || tag by segments and join
//   tseal <A> <key> <nonce> <aad> <pt>            -> ct || tag by one team (the one-wave kernels)
//   lseal <A> <key> <nonce> <aad> <pt>            -> ct || tag by aes_gcm_seal / chacha20poly1305_seal
//   sopen <A> <key> <nonce> <aad> <ct || tag> <L> -> "<1 | 0> <plaintext>" by segments and join,
//                                                    zeros when the verdict is 0
//   topen <A> <key> <nonce> <aad> <ct || tag>     -> the same by one team
//   sshare <A> <key> <nonce> <aad> <ct || tag> <slen> <L>
//                                        -> "<1 | 0> <mask> <row>": the segments through ShareSink
//                                           into a row of slen bytes (preset 0xaa); bit s of mask
//                                           is set when a sink of segment s saw another header;
//                                           the row is zeros when the verdict is 0 or the mask not
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../janus_amd/csrc/chacha_poly_team.h"
#include "../../janus_amd/csrc/plan_hpke.h"

using namespace p3g;
typedef std::vector<uint8_t> Bytes;
static const uint32_t kLanes = 64;
static const uint32_t kPitch = 8;  // words between two segments' sums, as the kernels keep them

static int nib(char c) {
  if (c >= '0' && c <= '9') return c - '0';
  if (c >= 'a' && c <= 'f') return c - 'a' + 10;
  return -1;
}

static bool unhex(std::string hex, Bytes* out) {
  if (hex == "-") hex.clear();
  out->clear();
  out->shrink_to_fit();
  if (hex.empty() || hex.size() % 2) return hex.empty();
  out->resize(hex.size() / 2);
  out->shrink_to_fit();
  for (size_t i = 0; i < out->size(); ++i) {
    const int h = nib(hex[2 * i]), l = nib(hex[2 * i + 1]);
    if (h < 0 || l < 0) return false;
    (*out)[i] = (uint8_t)(h * 16 + l);
  }
  return true;
}

static std::string hex(const uint8_t* p, size_t n) {
  static const char* d = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; ++i) {
    s += d[p[i] >> 4];
    s += d[p[i] & 15];
  }
  return s.empty() ? "-" : s;
}

static void be32_words(const Bytes& b, uint32_t* w) {  // b.size() is a multiple of 4
  for (size_t i = 0; i < b.size() / 4; ++i)
    w[i] = (uint32_t)b[4 * i] << 24 | (uint32_t)b[4 * i + 1] << 16 | (uint32_t)b[4 * i + 2] << 8 |
           b[4 * i + 3];
}

static void le32_words(const Bytes& b, uint32_t* w) {
  for (size_t i = 0; i < b.size() / 4; ++i)
    w[i] = (uint32_t)b[4 * i] | (uint32_t)b[4 * i + 1] << 8 | (uint32_t)b[4 * i + 2] << 16 |
           (uint32_t)b[4 * i + 3] << 24;
}

static std::string hex_be(const uint32_t* w, size_t n) {
  Bytes b(4 * n);
  for (size_t i = 0; i < 4 * n; ++i) b[i] = (uint8_t)(w[i >> 2] >> (24 - 8 * (i & 3)));
  return hex(b.data(), b.size());
}

static Bytes block(size_t n) {  // exactly n bytes, preset
  Bytes b(n, 0xaa);
  b.shrink_to_fit();
  return b;
}

static Bytes body_of(const Bytes& ct) {  // the body alone: a read past it is past the block
  Bytes text(ct.begin(), ct.end() - 16);
  text.shrink_to_fit();
  return text;
}

static void powers(const uint32_t h[4], uint32_t* tbl) {  // the shell's order: step by step
  for (int i = 0; i < 4; ++i) tbl[i] = h[i];
  for (uint32_t half = 1; half < kLanes; half *= 2)
    for (uint32_t lane = 0; lane < kLanes; ++lane) gf128_powers_step(tbl, lane, half);
}

// hpke_team_wave.h's poly_team_sum: the butterfly's steps 1, 2, 4, a carry pass, 8, 16, 32, a
// carry pass, in 32 bits.  false if the lanes do not end alike.
static bool team_sum(std::vector<PolyTeam>& t, uint32_t sum[5]) {
  uint32_t h[kLanes][5], g[kLanes][5];
  for (uint32_t l = 0; l < kLanes; ++l)
    for (int i = 0; i < 5; ++i) h[l][i] = t[l].mac.h[i];
  for (uint32_t m = 1; m < kLanes; m *= 2) {
    for (uint32_t l = 0; l < kLanes; ++l)
      for (int i = 0; i < 5; ++i) g[l][i] = h[l][i] + h[l ^ m][i];
    for (uint32_t l = 0; l < kLanes; ++l) {
      for (int i = 0; i < 5; ++i) h[l][i] = g[l][i];
      if (m == 4 || m == kLanes / 2) poly1305_carry(h[l]);
    }
  }
  bool same = true;
  for (uint32_t l = 0; l < kLanes; ++l)
    for (int i = 0; i < 5; ++i) same &= h[l][i] == h[0][i];
  for (int i = 0; i < 5; ++i) sum[i] = h[0][i];
  return same;
}

struct Segments {
  uint64_t nb, L;
  uint32_t S;
  Segments(uint64_t body, uint64_t l) : nb((body + 15) / 16), L(l) {
    S = (uint32_t)((nb + L - 1) / L);
    if (S == 0) S = 1;
  }
  uint64_t b0(uint32_t s) const { return s * L; }
  uint64_t b1(uint32_t s) const { return b0(s) + L < nb ? b0(s) + L : nb; }
};

// ---- AES-GCM ----------------------------------------------------------------------------------
// The tag from the segments' sums, as k_hpke_*_team_join computes it: the key's start over an
// empty AAD, the fold, the length block.
template <int NK>
static void gcm_join_tag(const uint8_t* sbox, const uint32_t* kw, const uint32_t* nw,
                         const std::vector<uint32_t>& parts, const Segments& g, size_t alen,
                         size_t body, uint32_t t[4]) {
  uint32_t rk[4 * (NK + 7)], h[4], y0[4], ctr[4], y[4];
  aes_gcm_start<NK>(sbox, kw, nw, PackedBytes{nullptr, 0}, rk, h, y0, ctr);
  gcm_split_join(h, parts.data(), kPitch, g.S, g.L, g.nb, y);
  aes_gcm_tag<NK>(sbox, rk, h, y, ctr, alen, body, t);
}

// One segment as k_hpke_*_team_split's wave runs it; sinks: one per lane.
template <int NK, bool SEAL, class Sink>
static void gcm_segment(const uint8_t* sbox, const uint32_t* kw, const uint32_t* nw,
                        const PackedBytes& aad, const PackedBytes& text, const Segments& g,
                        uint32_t s, std::vector<Sink>& sinks, uint32_t* part) {
  uint32_t rk[4 * (NK + 7)], h[4], y0[4], ctr[4], tbl[4 * kLanes], sum[4] = {0, 0, 0, 0};
  const FirstSegmentAad<PackedBytes> seg_aad{aad, s == 0};
  aes_gcm_start<NK>(sbox, kw, nw, seg_aad, rk, h, y0, ctr);
  powers(h, tbl);
  for (uint32_t lane = 0; lane < kLanes; ++lane) {
    uint32_t acc[4] = {0, 0, 0, 0};
    if constexpr (SEAL)
      gcm_team_seal_stripe_range<NK>(sbox, rk, ctr, tbl, y0, text, g.b0(s), g.b1(s), lane, kLanes,
                                     acc, sinks[lane]);
    else
      gcm_team_stripe_range<NK, true, true>(sbox, rk, ctr, tbl, y0, text.p, text.n, g.b0(s),
                                            g.b1(s), lane, kLanes, acc, sinks[lane]);
    for (int i = 0; i < 4; ++i) sum[i] ^= acc[i];
  }
  for (int i = 0; i < 4; ++i) part[i] = sum[i];
}

template <int NK>
struct Gcm {
  uint8_t sbox[256];
  uint32_t kw[NK], nw[3];
  Gcm(const Bytes& key, const Bytes& nonce) {
    aes_sbox_fill(sbox, 0, 1);
    be32_words(key, kw);
    be32_words(nonce, nw);
  }
  Bytes split_seal(const Bytes& aad, const Bytes& pt, uint64_t L) {
    const Segments g(pt.size(), L);
    Bytes ct = block(pt.size() + 16);
    std::vector<uint32_t> parts(kPitch * g.S, 0xaaaaaaaau);
    std::vector<CtSink> sinks(kLanes, CtSink{ct.data()});
    for (uint32_t s = 0; s < g.S; ++s)
      gcm_segment<NK, true>(sbox, kw, nw, PackedBytes{aad.data(), aad.size()},
                            PackedBytes{pt.data(), pt.size()}, g, s, sinks, &parts[kPitch * s]);
    uint32_t t[4];
    gcm_join_tag<NK>(sbox, kw, nw, parts, g, aad.size(), pt.size(), t);
    store_block_any(ct.data() + pt.size(), t);
    return ct;
  }
  // sinks[s]: one sink per lane of segment s
  template <class Sink>
  bool split_open(const Bytes& aad, const Bytes& ct, uint64_t L,
                  std::vector<std::vector<Sink>>& sinks) {
    const Bytes text = body_of(ct);
    const Segments g(text.size(), L);
    std::vector<uint32_t> parts(kPitch * g.S, 0xaaaaaaaau);
    for (uint32_t s = 0; s < g.S; ++s)
      gcm_segment<NK, false>(sbox, kw, nw, PackedBytes{aad.data(), aad.size()},
                             PackedBytes{text.data(), text.size()}, g, s, sinks[s],
                             &parts[kPitch * s]);
    uint32_t t[4], tag[4], diff = 0;
    gcm_join_tag<NK>(sbox, kw, nw, parts, g, aad.size(), text.size(), t);
    load_block(ct.data() + text.size(), 16, tag);
    for (int i = 0; i < 4; ++i) diff |= t[i] ^ tag[i];
    return diff == 0;
  }
  Bytes team_seal(const Bytes& aad, const Bytes& pt) {
    uint32_t rk[4 * (NK + 7)], h[4], y0[4], ctr[4], tbl[4 * kLanes], sum[4] = {0, 0, 0, 0};
    uint32_t y[4], t[4];
    Bytes ct = block(pt.size() + 16);
    aes_gcm_start<NK>(sbox, kw, nw, PackedBytes{aad.data(), aad.size()}, rk, h, y0, ctr);
    powers(h, tbl);
    CtSink sink{ct.data()};
    for (uint32_t lane = 0; lane < kLanes; ++lane) {
      uint32_t acc[4] = {0, 0, 0, 0};
      gcm_team_seal_stripe<NK>(sbox, rk, ctr, tbl, y0, PackedBytes{pt.data(), pt.size()}, lane,
                               kLanes, acc, sink);
      for (int i = 0; i < 4; ++i) sum[i] ^= acc[i];
    }
    gcm_team_join(y, sum, y0, pt.size());
    aes_gcm_tag<NK>(sbox, rk, h, y, ctr, aad.size(), pt.size(), t);
    store_block_any(ct.data() + pt.size(), t);
    return ct;
  }
  bool team_open(const Bytes& aad, const Bytes& ct, Bytes* pt) {
    uint32_t rk[4 * (NK + 7)], h[4], y0[4], ctr[4], tbl[4 * kLanes], sum[4] = {0, 0, 0, 0};
    uint32_t y[4], t[4], tag[4], diff = 0;
    const Bytes text = body_of(ct);
    *pt = block(text.size());
    aes_gcm_start<NK>(sbox, kw, nw, PackedBytes{aad.data(), aad.size()}, rk, h, y0, ctr);
    powers(h, tbl);
    PackedSink sink{pt->data()};
    for (uint32_t lane = 0; lane < kLanes; ++lane) {
      uint32_t acc[4] = {0, 0, 0, 0};
      gcm_team_stripe<NK, true, true>(sbox, rk, ctr, tbl, y0, text.data(), text.size(), lane,
                                      kLanes, acc, sink);
      for (int i = 0; i < 4; ++i) sum[i] ^= acc[i];
    }
    gcm_team_join(y, sum, y0, text.size());
    aes_gcm_tag<NK>(sbox, rk, h, y, ctr, aad.size(), text.size(), t);
    load_block(ct.data() + text.size(), 16, tag);
    for (int i = 0; i < 4; ++i) diff |= t[i] ^ tag[i];
    if (diff)
      for (uint32_t lane = 0; lane < kLanes; ++lane) gcm_team_wipe(sink, text.size(), lane, kLanes);
    return diff == 0;
  }
  Bytes lane_seal(const Bytes& aad, const Bytes& pt) {
    Bytes ct = block(pt.size() + 16);
    aes_gcm_seal<NK>(sbox, kw, nw, PackedBytes{aad.data(), aad.size()},
                     PackedBytes{pt.data(), pt.size()}, ct.data());
    return ct;
  }
};

// ---- ChaCha20-Poly1305 ------------------------------------------------------------------------
struct Chacha {
  uint32_t kw[8], nw[3], otk[16];
  Chacha(const Bytes& key, const Bytes& nonce) {
    le32_words(key, kw);
    le32_words(nonce, nw);
    chacha20_block(kw, 0u, nw, otk);
  }
  template <bool SEAL, class Sink>
  bool segment(const PackedBytes& aad, const PackedBytes& text, const Segments& g, uint32_t s,
               std::vector<Sink>& sinks, uint32_t* part) {
    const uint64_t c0 = g.b0(s) / 4, c1 = (g.b1(s) + 3) / 4;
    std::vector<PolyTeam> lanes(kLanes);
    for (uint32_t lane = 0; lane < kLanes; ++lane) {
      poly_team_start_range(lanes[lane], otk, aad, s == 0, c0, c1, g.b1(s), lane, kLanes);
      chacha_team_stripe_range<SEAL>(lanes[lane], kw, nw, text, c0, c1, lane, kLanes, sinks[lane]);
    }
    uint32_t sum[5];
    const bool same = team_sum(lanes, sum);
    for (int i = 0; i < 5; ++i) part[i] = sum[i];
    return same;
  }
  void join_tag(const std::vector<uint32_t>& parts, const Segments& g, size_t alen, size_t body,
                uint32_t t[4]) {
    uint32_t sum[5];
    PolyTeam pt;
    poly1305_init(pt.mac, otk);
    poly_split_join(pt.mac.r, parts.data(), kPitch, g.S, g.L, g.nb, sum);
    poly_team_tag(pt, sum, alen, body, t);
  }
  Bytes split_seal(const Bytes& aad, const Bytes& pt, uint64_t L) {
    const Segments g(pt.size(), L);
    Bytes ct = block(pt.size() + 16);
    std::vector<uint32_t> parts(kPitch * g.S, 0xaaaaaaaau);
    std::vector<CtSink> sinks(kLanes, CtSink{ct.data()});
    bool same = true;
    for (uint32_t s = 0; s < g.S; ++s)
      same &= segment<true>(PackedBytes{aad.data(), aad.size()}, PackedBytes{pt.data(), pt.size()},
                            g, s, sinks, &parts[kPitch * s]);
    if (!same) return Bytes();
    uint32_t t[4];
    join_tag(parts, g, aad.size(), pt.size(), t);
    store_block_any(ct.data() + pt.size(), t);
    return ct;
  }
  template <class Sink>
  bool split_open(const Bytes& aad, const Bytes& ct, uint64_t L,
                  std::vector<std::vector<Sink>>& sinks) {
    const Bytes text = body_of(ct);
    const Segments g(text.size(), L);
    std::vector<uint32_t> parts(kPitch * g.S, 0xaaaaaaaau);
    bool same = true;
    for (uint32_t s = 0; s < g.S; ++s)
      same &= segment<false>(PackedBytes{aad.data(), aad.size()},
                             PackedBytes{text.data(), text.size()}, g, s, sinks[s],
                             &parts[kPitch * s]);
    uint32_t t[4], tag[4], diff = 0;
    join_tag(parts, g, aad.size(), text.size(), t);
    load_block(ct.data() + text.size(), 16, tag);
    for (int i = 0; i < 4; ++i) diff |= t[i] ^ tag[i];
    return same && diff == 0;
  }
  Bytes team_seal(const Bytes& aad, const Bytes& pt) {
    Bytes ct = block(pt.size() + 16);
    uint32_t t[4], sum[5];
    const PackedBytes a{aad.data(), aad.size()}, src{pt.data(), pt.size()};
    std::vector<PolyTeam> lanes(kLanes);
    CtSink sink{ct.data()};
    for (uint32_t lane = 0; lane < kLanes; ++lane) {
      chacha_team_start(lanes[lane], kw, nw, a, pt.size(), lane, kLanes);
      chacha_team_stripe<true>(lanes[lane], kw, nw, src, lane, kLanes, sink);
    }
    if (!team_sum(lanes, sum)) return Bytes();
    poly_team_tag(lanes[0], sum, aad.size(), pt.size(), t);
    store_block_any(ct.data() + pt.size(), t);
    return ct;
  }
  bool team_open(const Bytes& aad, const Bytes& ct, Bytes* pt) {
    const Bytes text = body_of(ct);
    *pt = block(text.size());
    uint32_t t[4], tag[4], sum[5], diff = 0;
    const PackedBytes a{aad.data(), aad.size()}, src{text.data(), text.size()};
    std::vector<PolyTeam> lanes(kLanes);
    PackedSink sink{pt->data()};
    for (uint32_t lane = 0; lane < kLanes; ++lane) {
      chacha_team_start(lanes[lane], kw, nw, a, text.size(), lane, kLanes);
      chacha_team_stripe<false>(lanes[lane], kw, nw, src, lane, kLanes, sink);
    }
    bool ok = team_sum(lanes, sum);
    poly_team_tag(lanes[0], sum, aad.size(), text.size(), t);
    load_block(ct.data() + text.size(), 16, tag);
    for (int i = 0; i < 4; ++i) diff |= t[i] ^ tag[i];
    ok &= diff == 0;
    if (!ok)
      for (uint32_t lane = 0; lane < kLanes; ++lane)
        chacha_team_wipe(sink, text.size(), lane, kLanes);
    return ok;
  }
  Bytes lane_seal(const Bytes& aad, const Bytes& pt) {
    Bytes ct = block(pt.size() + 16);
    chacha20poly1305_seal(kw, nw, PackedBytes{aad.data(), aad.size()},
                          PackedBytes{pt.data(), pt.size()}, ct.data());
    return ct;
  }
};

// ---- the commands, for either AEAD ------------------------------------------------------------
template <class A>
static std::string run_aead(A& a, const std::string& cmd, const Bytes& aad, const Bytes& text,
                            uint32_t slen, uint64_t L) {
  if (cmd == "sseal" || cmd == "tseal" || cmd == "lseal") {
    const Bytes ct = cmd == "sseal" ? a.split_seal(aad, text, L)
                     : cmd == "tseal" ? a.team_seal(aad, text) : a.lane_seal(aad, text);
    return ct.empty() ? "err the lanes' sums differ" : hex(ct.data(), ct.size());
  }
  const size_t body = text.size() - 16;
  const Segments g(body, L ? L : 1);
  if (cmd == "topen") {
    Bytes pt;
    const bool ok = a.team_open(aad, text, &pt);
    return std::string(ok ? "1 " : "0 ") + hex(pt.data(), pt.size());
  }
  if (cmd == "sopen") {
    Bytes pt = block(body);
    std::vector<std::vector<PackedSink>> sinks(
        g.S, std::vector<PackedSink>(kLanes, PackedSink{pt.data()}));
    const bool ok = a.split_open(aad, text, L, sinks);
    if (!ok && body) memset(pt.data(), 0, body);  // k_hpke_team_wipe
    return std::string(ok ? "1 " : "0 ") + hex(pt.data(), pt.size());
  }
  // sshare
  Bytes row = block(slen);
  std::vector<std::vector<ShareSink>> sinks(
      g.S, std::vector<ShareSink>(kLanes, ShareSink{row.data(), slen, 0u}));
  const bool ok = a.split_open(aad, text, L, sinks);
  uint64_t mask = 0;
  for (uint32_t s = 0; s < g.S; ++s)
    for (uint32_t lane = 0; lane < kLanes; ++lane)
      if (sinks[s][lane].bad) mask |= 1ull << s;
  if ((!ok || mask) && slen) memset(row.data(), 0, slen);
  return std::string(ok ? "1 " : "0 ") + std::to_string(mask) + " " + hex(row.data(), row.size());
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd, a, b, c, d;
    in >> cmd;
    Bytes x, y, z, u;
    if (cmd == "plan") {
      uint64_t n, body, unit, cap, minb, slots;
      in >> n >> body >> unit >> cap >> minb >> slots;
      if (!in) {
        std::printf("err bad arguments\n");
        continue;
      }
      const TeamSplit t = team_split_plan(n, body, (uint32_t)unit, (uint32_t)cap, minb, slots);
      std::printf("%u %llu\n", t.S, (unsigned long long)t.L);
    } else if (cmd == "pow64") {
      uint64_t e = 0;
      in >> a >> e;
      if (!in || !unhex(a, &x) || x.size() != 16) {
        std::printf("err bad arguments\n");
        continue;
      }
      uint32_t k[8] = {0, 0, 0, 0, 0, 0, 0, 0}, p[5];
      le32_words(x, k);
      Poly1305 mac;
      poly1305_init(mac, k);
      poly1305_pow64(mac.r, e, p);
      std::printf("%u %u %u %u %u\n", p[0], p[1], p[2], p[3], p[4]);
    } else if (cmd == "gfpow") {
      uint32_t k = 0;
      in >> a >> k;
      if (!in || !unhex(a, &x) || x.size() != 16 || k > 1024) {
        std::printf("err bad arguments\n");
        continue;
      }
      uint32_t h[4], p[4], q[4] = {0x80000000u, 0, 0, 0};
      be32_words(x, h);
      gf128_pow(h, 64 * k, p);
      for (uint32_t i = 0; i < 64 * k; ++i) gf128_mul(q, h, q);
      std::printf("%s %s\n", hex_be(p, 4).c_str(), hex_be(q, 4).c_str());
    } else if (cmd == "sseal" || cmd == "tseal" || cmd == "lseal" || cmd == "sopen" ||
               cmd == "topen" || cmd == "sshare") {
      int aead = 0;
      uint32_t slen = 0;
      uint64_t L = 0;
      in >> aead >> a >> b >> c >> d;
      if (cmd == "sshare") in >> slen;
      if (cmd == "sseal" || cmd == "sopen" || cmd == "sshare") in >> L;
      const bool seal = cmd == "sseal" || cmd == "tseal" || cmd == "lseal";
      const bool split = cmd == "sseal" || cmd == "sopen" || cmd == "sshare";
      if (!in || aead < 1 || aead > 3 || !unhex(a, &x) || !unhex(b, &y) || !unhex(c, &z) ||
          !unhex(d, &u) || x.size() != (aead == 1 ? 16u : 32u) || y.size() != 12 ||
          (!seal && u.size() < 16) || (split && (L == 0 || L % (aead == 3 ? 256 : 64))) ||
          (split && u.size() <= (seal ? 0u : 16u)) ||
          (cmd == "sshare" && u.size() != 6 + (size_t)slen + 16)) {
        std::printf("err bad arguments\n");
        continue;
      }
      std::string out;
      if (aead == 1) {
        Gcm<4> g(x, y);
        out = run_aead(g, cmd, z, u, slen, L);
      } else if (aead == 2) {
        Gcm<8> g(x, y);
        out = run_aead(g, cmd, z, u, slen, L);
      } else {
        Chacha g(x, y);
        out = run_aead(g, cmd, z, u, slen, L);
      }
      std::printf("%s\n", out.c_str());
    } else if (!cmd.empty()) {
      std::printf("err unknown command\n");
    }
  }
  return 0;
}
