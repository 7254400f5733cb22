// Driver of tests/test_chacha_poly_team.py: the team ChaCha20-Poly1305 of
// janus_amd/csrc/chacha_poly_team.h (what a wave of hpke_open_team.h's and hpke_seal_team.h's
// kernels runs per report under AEAD 3) built for the host, the 64 lanes simulated in a loop and
// what the kernel shell does across lanes (the butterfly sum of the lanes' limbs in 32 bits with a
// carry pass between its halves, one verdict, lane 0's tag store) done here.  A text protocol on
// stdin / stdout, one answer line per command; byte strings are hex, "-" when empty, and every
// input is used from a heap block of exactly its length and every output written to one of exactly
// its length, so a sanitizer build sees any access past either:
//   mul <a0 .. a4> <b0 .. b4>            -> the five limbs of poly1305_mul(a, b), decimal
//   pow <r: 16 bytes> <e>                -> the five limbs of poly1305_pow(clamp(r), e)
//   tmac <r || s: 32 bytes> <aad> <body> -> "<striped tag> <poly1305_mac tag>" over pad16(aad) ||
//                                           pad16(body) || LE64 lengths under that one-time key
//   seal <key> <nonce> <aad> <pt>        -> ct || tag of chacha20poly1305_seal
//   open <key> <nonce> <aad> <ct || tag> -> "<1 | 0> <plaintext>" of chacha20poly1305_open (preset
//                                           0xaa)
//   tseal <key> <nonce> <aad> <pt> <off> -> ct || tag of the team seal through CtSink into a slot
//                                           that starts `off` bytes past a 16-byte boundary
//   topen <key> <nonce> <aad> <ct || tag>
//                                        -> "<1 | 0> <plaintext>" of the team open into a packed
//                                           slot
//   tshare <key> <nonce> <aad> <ct || tag> <slen> <shift>
//                                        -> "<1 | 0> <header bad: 1 | 0> <row>" of the team open
//                                           through ShareSink into a row of slen bytes (preset
//                                           0xaa) that starts `shift` bytes past a 16-byte boundary;
//                                           the row is zeroed again when the header is bad, as the
//                                           kernel does
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../janus_amd/csrc/chacha_poly_team.h"

using namespace p3g;
typedef std::vector<uint8_t> Bytes;
static const uint32_t kLanes = 64;

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

static void le32_words(const Bytes& b, uint32_t* w) {  // b.size() is a multiple of 4
  for (size_t i = 0; i < b.size() / 4; ++i)
    w[i] = (uint32_t)b[4 * i] | (uint32_t)b[4 * i + 1] << 8 | (uint32_t)b[4 * i + 2] << 16 |
           (uint32_t)b[4 * i + 3] << 24;
}

static std::string hex_le(const uint32_t* w, size_t n) {
  Bytes b(4 * n);
  for (size_t i = 0; i < 4 * n; ++i) b[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
  return hex(b.data(), b.size());
}

static Bytes block(size_t n) {  // exactly n bytes, preset
  Bytes b(n, 0xaa);
  b.shrink_to_fit();
  return b;
}

struct NoSink {
  void store(uint64_t, const uint32_t*, uint32_t) {}
  void put(uint64_t, const uint32_t*, uint32_t) {}
};

// The shell's sum of the lanes' limbs, in its order and in 32 bits: the butterfly's steps 1, 2, 4,
// a carry pass, the steps 8, 16, 32, a carry pass.  false if the lanes do not end alike.
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

// The wave's open as hpke_open_team_wave_chacha orders it: every lane's start and stripe, the sum,
// the tag on every lane, and every lane's wipe on a mismatch.  sinks: one per lane.
template <class Sink>
static bool team_open(const Bytes& key, const Bytes& nonce, const Bytes& aad, const Bytes& ct,
                      std::vector<Sink>& sinks) {
  uint32_t kw[8], nw[3], tag[4], t[4], sum[5];
  le32_words(key, kw);
  le32_words(nonce, nw);
  const size_t body = ct.size() - 16;
  Bytes text(ct.begin(), ct.begin() + body);  // the body alone: a read past it is past the block
  text.shrink_to_fit();
  const PackedBytes a{aad.data(), aad.size()}, src{text.data(), text.size()};
  std::vector<PolyTeam> lanes(kLanes);
  for (uint32_t lane = 0; lane < kLanes; ++lane) {
    chacha_team_start(lanes[lane], kw, nw, a, body, lane, kLanes);
    chacha_team_stripe<false>(lanes[lane], kw, nw, src, lane, kLanes, sinks[lane]);
  }
  bool ok = team_sum(lanes, sum);
  load_block(ct.data() + body, 16, tag);
  for (uint32_t lane = 0; lane < kLanes; ++lane) {
    poly_team_tag(lanes[lane], sum, aad.size(), body, t);
    uint32_t diff = 0;
    for (int i = 0; i < 4; ++i) diff |= t[i] ^ tag[i];
    ok &= diff == 0;
  }
  if (!ok)
    for (uint32_t lane = 0; lane < kLanes; ++lane) chacha_team_wipe(sinks[lane], body, lane, kLanes);
  return ok;
}

// The wave's seal as hpke_seal_team_wave orders it; the slot is ct[0 .. pt.size() + 16).
static bool team_seal(const Bytes& key, const Bytes& nonce, const Bytes& aad, const Bytes& pt,
                      uint8_t* ct) {
  uint32_t kw[8], nw[3], t[4], sum[5];
  le32_words(key, kw);
  le32_words(nonce, nw);
  const PackedBytes a{aad.data(), aad.size()}, src{pt.data(), pt.size()};
  std::vector<PolyTeam> lanes(kLanes);
  for (uint32_t lane = 0; lane < kLanes; ++lane) {
    CtSink sink{ct};
    chacha_team_start(lanes[lane], kw, nw, a, pt.size(), lane, kLanes);
    chacha_team_stripe<true>(lanes[lane], kw, nw, src, lane, kLanes, sink);
  }
  if (!team_sum(lanes, sum)) return false;
  poly_team_tag(lanes[0], sum, aad.size(), pt.size(), t);
  store_block_any(ct + pt.size(), t);
  return true;
}

static std::string team_mac(const Bytes& otk, const Bytes& aad, const Bytes& body) {
  uint32_t kw[8], zero[8] = {0, 0, 0, 0, 0, 0, 0, 0}, sum[5], t[4], want[4];
  le32_words(otk, kw);
  const PackedBytes a{aad.data(), aad.size()}, src{body.data(), body.size()};
  std::vector<PolyTeam> lanes(kLanes);
  NoSink none;
  for (uint32_t lane = 0; lane < kLanes; ++lane) {
    poly_team_start(lanes[lane], kw, a, body.size(), lane, kLanes);
    chacha_team_stripe<false>(lanes[lane], zero, zero, src, lane, kLanes, none);
  }
  if (!team_sum(lanes, sum)) return "err the lanes' sums differ";
  poly_team_tag(lanes[kLanes - 1], sum, aad.size(), body.size(), t);
  // the serial MAC over the message as RFC 8439 §2.8 lays it out
  const size_t pa = (aad.size() + 15) / 16 * 16, pb = (body.size() + 15) / 16 * 16;
  Bytes msg(pa + pb + 16, 0);
  msg.shrink_to_fit();
  for (size_t i = 0; i < aad.size(); ++i) msg[i] = aad[i];
  for (size_t i = 0; i < body.size(); ++i) msg[pa + i] = body[i];
  for (int i = 0; i < 8; ++i) {
    msg[pa + pb + i] = (uint8_t)((uint64_t)aad.size() >> (8 * i));
    msg[pa + pb + 8 + i] = (uint8_t)((uint64_t)body.size() >> (8 * i));
  }
  poly1305_mac(kw, msg.data(), msg.size(), want);
  return hex_le(t, 4) + " " + hex_le(want, 4);
}

static std::string team_share(const Bytes& key, const Bytes& nonce, const Bytes& aad,
                              const Bytes& ct, uint32_t slen, uint32_t shift) {
  // a block of exactly shift + slen bytes on a 16-byte boundary: the row is its last slen bytes
  void* mem = nullptr;
  if (posix_memalign(&mem, 16, shift + slen ? shift + slen : 1)) return "err allocation";
  uint8_t* base = static_cast<uint8_t*>(mem);
  for (uint32_t i = 0; i < shift + slen; ++i) base[i] = 0xaa;
  uint8_t* row = base + shift;
  std::vector<ShareSink> sinks(kLanes, ShareSink{row, slen, 0u});
  const bool ok = team_open(key, nonce, aad, ct, sinks);
  const bool bad = ok && sinks[0].bad != 0;  // block 0 is in chunk 0, lane 0's
  if (bad)
    for (uint32_t lane = 0; lane < kLanes; ++lane)
      chacha_team_wipe(sinks[lane], ct.size() - 16, lane, kLanes);
  bool guard = true;
  for (uint32_t i = 0; i < shift; ++i) guard &= base[i] == 0xaa;
  std::string out = std::string(ok ? "1 " : "0 ") + (bad ? "1 " : "0 ") + hex(row, slen);
  free(mem);
  return guard ? out : "err bytes before the row were written";
}

static std::string team_seal_at(const Bytes& key, const Bytes& nonce, const Bytes& aad,
                                const Bytes& pt, uint32_t off) {
  // a block of exactly off + pt.size() + 16 bytes on a 16-byte boundary: the slot is its end
  const size_t n = pt.size() + 16;
  void* mem = nullptr;
  if (posix_memalign(&mem, 16, off + n)) return "err allocation";
  uint8_t* base = static_cast<uint8_t*>(mem);
  for (size_t i = 0; i < off + n; ++i) base[i] = 0xaa;
  const bool ok = team_seal(key, nonce, aad, pt, base + off);
  bool guard = true;
  for (uint32_t i = 0; i < off; ++i) guard &= base[i] == 0xaa;
  std::string out = hex(base + off, n);
  free(mem);
  if (!ok) return "err the lanes' sums differ";
  return guard ? out : "err bytes before the slot were written";
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd, a, b, c, d;
    in >> cmd;
    Bytes x, y, z, u;
    if (cmd == "mul") {
      uint32_t v[10], p[5];
      for (int i = 0; i < 10; ++i) in >> v[i];
      if (!in) {
        std::printf("err bad arguments\n");
        continue;
      }
      poly1305_mul(v, v + 5, p);
      std::printf("%u %u %u %u %u\n", p[0], p[1], p[2], p[3], p[4]);
    } else if (cmd == "pow") {
      uint32_t e = 0;
      in >> a >> e;
      if (!in || !unhex(a, &x) || x.size() != 16 || e >= 512) {
        std::printf("err bad arguments\n");
        continue;
      }
      uint32_t k[8] = {0, 0, 0, 0, 0, 0, 0, 0}, p[5];
      le32_words(x, k);
      Poly1305 mac;
      poly1305_init(mac, k);
      poly1305_pow(mac.r, e, p);
      std::printf("%u %u %u %u %u\n", p[0], p[1], p[2], p[3], p[4]);
    } else if (cmd == "tmac") {
      in >> a >> b >> c;
      if (!in || !unhex(a, &x) || !unhex(b, &y) || !unhex(c, &z) || x.size() != 32) {
        std::printf("err bad arguments\n");
        continue;
      }
      std::printf("%s\n", team_mac(x, y, z).c_str());
    } else if (cmd == "seal" || cmd == "open" || cmd == "topen" || cmd == "tshare" ||
               cmd == "tseal") {
      uint32_t slen = 0, shift = 0, off = 0;
      in >> a >> b >> c >> d;
      if (cmd == "tshare") in >> slen >> shift;
      if (cmd == "tseal") in >> off;
      const bool seal = cmd == "seal" || cmd == "tseal";
      if (!in || !unhex(a, &x) || !unhex(b, &y) || !unhex(c, &z) || !unhex(d, &u) ||
          x.size() != 32 || y.size() != 12 || (!seal && u.size() < 16) || off > 15 ||
          (cmd == "tshare" && (u.size() != 6 + (size_t)slen + 16 || shift > 15))) {
        std::printf("err bad arguments\n");
        continue;
      }
      uint32_t kw[8], nw[3];
      le32_words(x, kw);
      le32_words(y, nw);
      if (cmd == "seal") {
        Bytes ct = block(u.size() + 16);
        chacha20poly1305_seal(kw, nw, PackedBytes{z.data(), z.size()},
                              PackedBytes{u.data(), u.size()}, ct.data());
        std::printf("%s\n", hex(ct.data(), ct.size()).c_str());
      } else if (cmd == "tseal") {
        std::printf("%s\n", team_seal_at(x, y, z, u, off).c_str());
      } else if (cmd == "open") {
        const size_t body = u.size() - 16;
        uint32_t tag[4];
        load_block(u.data() + body, 16, tag);
        Bytes text(u.begin(), u.begin() + body);
        text.shrink_to_fit();
        Bytes pt = block(body);
        const bool ok = chacha20poly1305_open(kw, nw, PackedBytes{z.data(), z.size()},
                                              PackedBytes{text.data(), text.size()}, tag,
                                              pt.data());
        std::printf("%d %s\n", ok ? 1 : 0, hex(pt.data(), pt.size()).c_str());
      } else if (cmd == "topen") {
        Bytes pt = block(u.size() - 16);
        std::vector<PackedSink> sinks(kLanes, PackedSink{pt.data()});
        const bool ok = team_open(x, y, z, u, sinks);
        std::printf("%d %s\n", ok ? 1 : 0, hex(pt.data(), pt.size()).c_str());
      } else {
        std::printf("%s\n", team_share(x, y, z, u, slen, shift).c_str());
      }
    } else if (!cmd.empty()) {
      std::printf("err unknown command\n");
    }
  }
  return 0;
}
