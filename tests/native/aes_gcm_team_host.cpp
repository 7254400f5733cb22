// Driver of tests/test_aes_gcm_team.py: the team AES-GCM of janus_amd/csrc/aes_gcm_team.h (what a
// wave of hpke_open_team.h's kernels runs per report) built for the host, the 64 lanes simulated in
// a loop and what the kernel shell does across lanes (the table's steps in order, the XOR of the
// lanes' sums, one verdict) done here.  A text protocol on stdin / stdout, one answer line per
// command; byte strings are hex, "-" when empty, and every input is used from a heap block of
// exactly its length and every output written to one of exactly its length, so a sanitizer build
// sees any access past either:
//   mul <a> <b>                          -> gf128_mul(a, b)
//   step <y> <x> <h>                     -> "<gf128_mul(y ^ x, h)> <ghash_step(y, x, h)>"
//   powers <h>                           -> H^1 .. H^64 from gf128_powers_step, 1024 bytes
//   tghash <h> <y0> <bytes>              -> "<striped GHASH> <ghash_bytes>" from the state y0
//   tctr <key> <nonce> <text>            -> text XOR the team's keystream (blocks from counter 2)
//   seal <key> <nonce> <aad> <pt>        -> ct || tag of aes_gcm_seal
//   open <key> <nonce> <aad> <ct || tag> -> "<1 | 0> <plaintext>" of aes_gcm_open (preset 0xaa)
//   topen <key> <nonce> <aad> <ct || tag>
//                                        -> the same from the team open into a packed slot
//   tshare <key> <nonce> <aad> <ct || tag> <slen> <shift>
//                                        -> "<1 | 0> <header bad: 1 | 0> <row>" of the team open
//                                           through ShareSink into a row of slen bytes (preset
//                                           0xaa) that starts `shift` bytes past a 16-byte boundary;
//                                           the row is zeroed again when the header is bad, as the
//                                           kernel does
// Field elements are 16 bytes in GCM's order (four big-endian words).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../janus_amd/csrc/aes_gcm_team.h"

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

static void powers(const uint32_t h[4], uint32_t* tbl) {  // the shell's order: step by step
  for (int i = 0; i < 4; ++i) tbl[i] = h[i];
  for (uint32_t half = 1; half < kLanes; half *= 2)
    for (uint32_t lane = 0; lane < kLanes; ++lane) gf128_powers_step(tbl, lane, half);
}

struct NoSink {
  void store(uint64_t, const uint32_t*, uint32_t) {}
  void put(uint64_t, const uint32_t*, uint32_t) {}
};

// The wave's open as hpke_open_team_wave orders it: start, table, every lane's stripe, the XOR,
// the tag, and every lane's wipe on a mismatch.  sinks: one per lane.
template <int NK, class Sink>
static bool team_open(const Bytes& key, const Bytes& nonce, const Bytes& aad, const Bytes& ct,
                      std::vector<Sink>& sinks) {
  uint8_t sbox[256];
  uint32_t kw[NK], nw[3], rk[4 * (NK + 7)], h[4], y0[4], ctr[4], tag[4], t[4], y[4];
  uint32_t tbl[4 * kLanes], sum[4] = {0, 0, 0, 0};
  aes_sbox_fill(sbox, 0, 1);
  be32_words(key, kw);
  be32_words(nonce, nw);
  const size_t body = ct.size() - 16;
  Bytes text(ct.begin(), ct.begin() + body);  // the body alone: a read past it is past the block
  text.shrink_to_fit();
  aes_gcm_start<NK>(sbox, kw, nw, PackedBytes{aad.data(), aad.size()}, rk, h, y0, ctr);
  powers(h, tbl);
  for (uint32_t lane = 0; lane < kLanes; ++lane) {
    uint32_t acc[4] = {0, 0, 0, 0};
    gcm_team_stripe<NK, true, true>(sbox, rk, ctr, tbl, y0, text.data(), body, lane, kLanes, acc,
                                    sinks[lane]);
    for (int i = 0; i < 4; ++i) sum[i] ^= acc[i];
  }
  gcm_team_join(y, sum, y0, body);
  aes_gcm_tag<NK>(sbox, rk, h, y, ctr, aad.size(), body, t);
  load_block(ct.data() + body, 16, tag);
  uint32_t diff = 0;
  for (int i = 0; i < 4; ++i) diff |= t[i] ^ tag[i];
  if (diff)
    for (uint32_t lane = 0; lane < kLanes; ++lane) gcm_team_wipe(sinks[lane], body, lane, kLanes);
  return diff == 0;
}

template <int NK>
static Bytes team_ctr(const Bytes& key, const Bytes& nonce, const Bytes& text) {
  uint8_t sbox[256];
  uint32_t kw[NK], nw[3], rk[4 * (NK + 7)], h[4], y0[4], ctr[4], acc[4] = {0, 0, 0, 0};
  aes_sbox_fill(sbox, 0, 1);
  be32_words(key, kw);
  be32_words(nonce, nw);
  aes_gcm_start<NK>(sbox, kw, nw, PackedBytes{nullptr, 0}, rk, h, y0, ctr);
  Bytes out = block(text.size());
  PackedSink sink{out.data()};
  for (uint32_t lane = 0; lane < kLanes; ++lane)
    gcm_team_stripe<NK, false, true>(sbox, rk, ctr, nullptr, y0, text.data(), text.size(), lane,
                                     kLanes, acc, sink);
  return out;
}

template <int NK>
static Bytes lane_seal(const Bytes& key, const Bytes& nonce, const Bytes& aad, const Bytes& pt) {
  uint8_t sbox[256];
  uint32_t kw[NK], nw[3];
  aes_sbox_fill(sbox, 0, 1);
  be32_words(key, kw);
  be32_words(nonce, nw);
  Bytes ct = block(pt.size() + 16);
  aes_gcm_seal<NK>(sbox, kw, nw, PackedBytes{aad.data(), aad.size()},
                   PackedBytes{pt.data(), pt.size()}, ct.data());
  return ct;
}

template <int NK>
static bool lane_open(const Bytes& key, const Bytes& nonce, const Bytes& aad, const Bytes& ct,
                      Bytes* pt) {
  uint8_t sbox[256];
  uint32_t kw[NK], nw[3], tag[4];
  aes_sbox_fill(sbox, 0, 1);
  be32_words(key, kw);
  be32_words(nonce, nw);
  const size_t body = ct.size() - 16;
  load_block(ct.data() + body, 16, tag);
  Bytes text(ct.begin(), ct.begin() + body);
  text.shrink_to_fit();
  *pt = block(body);
  return aes_gcm_open<NK>(sbox, kw, nw, PackedBytes{aad.data(), aad.size()},
                          PackedBytes{text.data(), text.size()}, tag, pt->data());
}

template <int NK>
static std::string team_share(const Bytes& key, const Bytes& nonce, const Bytes& aad,
                              const Bytes& ct, uint32_t slen, uint32_t shift) {
  // a block of exactly shift + slen bytes on a 16-byte boundary: the row is its last slen bytes
  void* mem = nullptr;
  if (posix_memalign(&mem, 16, shift + slen ? shift + slen : 1)) return "err allocation";
  uint8_t* base = static_cast<uint8_t*>(mem);
  for (uint32_t i = 0; i < shift + slen; ++i) base[i] = 0xaa;
  uint8_t* row = base + shift;
  std::vector<ShareSink> sinks(kLanes, ShareSink{row, slen, 0u});
  const bool ok = team_open<NK>(key, nonce, aad, ct, sinks);
  const bool bad = ok && sinks[0].bad != 0;  // block 0 is lane 0's
  if (bad)
    for (uint32_t lane = 0; lane < kLanes; ++lane)
      gcm_team_wipe(sinks[lane], ct.size() - 16, lane, kLanes);
  bool guard = true;
  for (uint32_t i = 0; i < shift; ++i) guard &= base[i] == 0xaa;
  std::string out = std::string(ok ? "1 " : "0 ") + (bad ? "1 " : "0 ") + hex(row, slen);
  free(mem);
  return guard ? out : "err bytes before the row were written";
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd, a, b, c, d;
    in >> cmd;
    Bytes x, y, z, u;
    if (cmd == "mul" || cmd == "step") {
      const bool step = cmd == "step";
      in >> a >> b;
      if (step) in >> c;
      if (!unhex(a, &x) || !unhex(b, &y) || x.size() != 16 || y.size() != 16 ||
          (step && (!unhex(c, &z) || z.size() != 16))) {
        std::printf("err bad arguments\n");
        continue;
      }
      uint32_t xw[4], yw[4], zw[4], p[4];
      be32_words(x, xw);
      be32_words(y, yw);
      if (!step) {
        gf128_mul(xw, yw, p);
        std::printf("%s\n", hex_be(p, 4).c_str());
      } else {
        be32_words(z, zw);
        uint32_t s[4];
        for (int i = 0; i < 4; ++i) s[i] = xw[i] ^ yw[i];
        gf128_mul(s, zw, p);
        ghash_step(xw, yw, zw);
        std::printf("%s %s\n", hex_be(p, 4).c_str(), hex_be(xw, 4).c_str());
      }
    } else if (cmd == "powers") {
      in >> a;
      if (!unhex(a, &x) || x.size() != 16) {
        std::printf("err bad arguments\n");
        continue;
      }
      uint32_t hw[4], tbl[4 * kLanes];
      be32_words(x, hw);
      powers(hw, tbl);
      std::printf("%s\n", hex_be(tbl, 4 * kLanes).c_str());
    } else if (cmd == "tghash") {
      in >> a >> b >> c;
      if (!unhex(a, &x) || !unhex(b, &y) || !unhex(c, &z) || x.size() != 16 || y.size() != 16) {
        std::printf("err bad arguments\n");
        continue;
      }
      uint32_t hw[4], y0[4], tbl[4 * kLanes], sum[4] = {0, 0, 0, 0}, yt[4], yl[4];
      be32_words(x, hw);
      be32_words(y, y0);
      powers(hw, tbl);
      NoSink none;
      for (uint32_t lane = 0; lane < kLanes; ++lane) {
        uint32_t acc[4] = {0, 0, 0, 0};
        gcm_team_stripe<4, true, false>(nullptr, nullptr, nullptr, tbl, y0, z.data(), z.size(),
                                        lane, kLanes, acc, none);
        for (int i = 0; i < 4; ++i) sum[i] ^= acc[i];
      }
      gcm_team_join(yt, sum, y0, z.size());
      for (int i = 0; i < 4; ++i) yl[i] = y0[i];
      ghash_bytes(yl, hw, PackedBytes{z.data(), z.size()});
      std::printf("%s %s\n", hex_be(yt, 4).c_str(), hex_be(yl, 4).c_str());
    } else if (cmd == "tctr") {
      in >> a >> b >> c;
      if (!unhex(a, &x) || !unhex(b, &y) || !unhex(c, &z) || (x.size() != 16 && x.size() != 32) ||
          y.size() != 12) {
        std::printf("err bad arguments\n");
        continue;
      }
      const Bytes o = x.size() == 16 ? team_ctr<4>(x, y, z) : team_ctr<8>(x, y, z);
      std::printf("%s\n", hex(o.data(), o.size()).c_str());
    } else if (cmd == "seal" || cmd == "open" || cmd == "topen" || cmd == "tshare") {
      uint32_t slen = 0, shift = 0;
      in >> a >> b >> c >> d;
      if (cmd == "tshare") in >> slen >> shift;
      const bool seal = cmd == "seal";
      if (!in || !unhex(a, &x) || !unhex(b, &y) || !unhex(c, &z) || !unhex(d, &u) ||
          (x.size() != 16 && x.size() != 32) || y.size() != 12 || (!seal && u.size() < 16) ||
          (cmd == "tshare" && (u.size() != 6 + (size_t)slen + 16 || shift > 15))) {
        std::printf("err bad arguments\n");
        continue;
      }
      const bool k16 = x.size() == 16;
      if (seal) {
        const Bytes ct = k16 ? lane_seal<4>(x, y, z, u) : lane_seal<8>(x, y, z, u);
        std::printf("%s\n", hex(ct.data(), ct.size()).c_str());
      } else if (cmd == "open") {
        Bytes pt;
        const bool ok = k16 ? lane_open<4>(x, y, z, u, &pt) : lane_open<8>(x, y, z, u, &pt);
        std::printf("%d %s\n", ok ? 1 : 0, hex(pt.data(), pt.size()).c_str());
      } else if (cmd == "topen") {
        Bytes pt = block(u.size() - 16);
        std::vector<PackedSink> sinks(kLanes, PackedSink{pt.data()});
        const bool ok = k16 ? team_open<4>(x, y, z, u, sinks) : team_open<8>(x, y, z, u, sinks);
        std::printf("%d %s\n", ok ? 1 : 0, hex(pt.data(), pt.size()).c_str());
      } else {
        std::printf("%s\n", (k16 ? team_share<4>(x, y, z, u, slen, shift)
                                 : team_share<8>(x, y, z, u, slen, shift)).c_str());
      }
    } else if (!cmd.empty()) {
      std::printf("err unknown command\n");
    }
  }
  return 0;
}
