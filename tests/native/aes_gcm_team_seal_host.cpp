// Driver of tests/test_aes_gcm_team_seal.py: the team AES-GCM seal of
// janus_amd/csrc/aes_gcm_team.h (what a wave of hpke_seal_team.h's kernels runs per report) built
// for the host, the 64 lanes simulated in a loop and what the kernel shell does across lanes (the
// table's steps in order, the XOR of the lanes' sums, one lane's tag store) done here.  A text
// protocol on stdin / stdout, one answer line per command; byte strings are hex, "-" when empty.
// Every input is used from a heap block of exactly its length.  The ciphertext slot starts `shift`
// bytes past a 16-byte boundary of a heap block of exactly shift + len + 16 + tail bytes filled
// with 0xa5; the answer is "err ..." when a byte before or after the slot has changed, and a
// sanitizer build sees any access past the block:
//   seal <key> <nonce> <aad> <pt>                  -> ct || tag of aes_gcm_seal
//   tseal <key> <nonce> <aad> <pt> <shift> <tail>  -> ct || tag of the team seal over a packed
//                                                     plaintext (PackedBytes)
//   tshare <key> <nonce> <aad> <share> <shift> <tail>
//                                                  -> the same over the PlaintextInputShare of a
//                                                     share row (SharePlaintext), never built
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../janus_amd/csrc/aes_gcm_team.h"
#include "../../janus_amd/csrc/hpke_lane.h"

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

template <int NK>
static std::string lane_seal(const Bytes& key, const Bytes& nonce, const Bytes& aad,
                             const Bytes& pt) {
  uint8_t sbox[256];
  uint32_t kw[NK], nw[3];
  aes_sbox_fill(sbox, 0, 1);
  be32_words(key, kw);
  be32_words(nonce, nw);
  Bytes ct(pt.size() + 16, 0xaa);
  ct.shrink_to_fit();
  aes_gcm_seal<NK>(sbox, kw, nw, PackedBytes{aad.data(), aad.size()},
                   PackedBytes{pt.data(), pt.size()}, ct.data());
  return hex(ct.data(), ct.size());
}

// The wave's seal as hpke_seal_team_wave orders it: start, table, every lane's stripe, the XOR, the
// tag from one lane.
template <int NK, class Src>
static std::string team_seal(const Bytes& key, const Bytes& nonce, const Bytes& aad, const Src& pt,
                             uint32_t shift, uint32_t tail) {
  uint8_t sbox[256];
  uint32_t kw[NK], nw[3], rk[4 * (NK + 7)], h[4], y0[4], ctr[4], t[4], y[4];
  uint32_t tbl[4 * kLanes], sum[4] = {0, 0, 0, 0};
  aes_sbox_fill(sbox, 0, 1);
  be32_words(key, kw);
  be32_words(nonce, nw);
  const size_t plen = pt.len(), clen = plen + 16, total = shift + clen + tail;
  void* mem = nullptr;
  if (posix_memalign(&mem, 16, total)) return "err allocation";
  uint8_t* base = static_cast<uint8_t*>(mem);
  for (size_t i = 0; i < total; ++i) base[i] = 0xa5;
  uint8_t* ct = base + shift;
  aes_gcm_start<NK>(sbox, kw, nw, PackedBytes{aad.data(), aad.size()}, rk, h, y0, ctr);
  for (int i = 0; i < 4; ++i) tbl[i] = h[i];
  for (uint32_t half = 1; half < kLanes; half *= 2)
    for (uint32_t lane = 0; lane < kLanes; ++lane) gf128_powers_step(tbl, lane, half);
  for (uint32_t lane = 0; lane < kLanes; ++lane) {
    uint32_t acc[4] = {0, 0, 0, 0};
    CtSink sink{ct};
    gcm_team_seal_stripe<NK>(sbox, rk, ctr, tbl, y0, pt, lane, kLanes, acc, sink);
    for (int i = 0; i < 4; ++i) sum[i] ^= acc[i];
  }
  gcm_team_join(y, sum, y0, plen);
  aes_gcm_tag<NK>(sbox, rk, h, y, ctr, aad.size(), plen, t);
  store_block_any(ct + plen, t);
  bool guard = true;
  for (size_t i = 0; i < shift; ++i) guard &= base[i] == 0xa5;
  for (size_t i = shift + clen; i < total; ++i) guard &= base[i] == 0xa5;
  const std::string out = hex(ct, clen);
  free(mem);
  return guard ? out : "err bytes outside the slot were written";
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd, a, b, c, d;
    in >> cmd;
    if (cmd.empty()) continue;
    Bytes x, y, z, u;
    uint32_t shift = 0, tail = 0;
    in >> a >> b >> c >> d;
    if (cmd != "seal") in >> shift >> tail;
    if ((cmd != "seal" && cmd != "tseal" && cmd != "tshare") || !in || !unhex(a, &x) ||
        !unhex(b, &y) || !unhex(c, &z) || !unhex(d, &u) || (x.size() != 16 && x.size() != 32) ||
        y.size() != 12 || shift > 15 || tail > 64) {
      std::printf("err bad arguments\n");
      continue;
    }
    const bool k16 = x.size() == 16;
    std::string out;
    if (cmd == "seal") {
      out = k16 ? lane_seal<4>(x, y, z, u) : lane_seal<8>(x, y, z, u);
    } else if (cmd == "tseal") {
      const PackedBytes pt{u.data(), u.size()};
      out = k16 ? team_seal<4>(x, y, z, pt, shift, tail) : team_seal<8>(x, y, z, pt, shift, tail);
    } else {
      const SharePlaintext pt{u.data(), (uint32_t)u.size()};
      out = k16 ? team_seal<4>(x, y, z, pt, shift, tail) : team_seal<8>(x, y, z, pt, shift, tail);
    }
    std::printf("%s\n", out.c_str());
  }
  return 0;
}
