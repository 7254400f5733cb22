// Driver of tests/test_hpke_seal_prims.py: the ChaCha20-Poly1305 seal of
// janus_amd/csrc/hpke_prims.h (what the GPU kernels of hpke_seal_gpu.h run for AEAD 3) built for
// the host.  A text protocol on stdin / stdout, one answer line per command; byte strings are
// hex, "-" when empty, and every input is used from a heap block of exactly its length and every
// output written to one of exactly its length, so a sanitizer build sees any access past either:
//   seal <key> <nonce> <aad> <pt>        -> ct || tag of chacha20poly1305_seal
//   rt <key> <nonce> <aad> <pt>          -> "<1 | 0> <plaintext>": chacha20poly1305_open of that
//                                           seal (the plaintext block is preset to 0xaa)
//   hseal <kdf> <shared_secret> <psk_id_hash> <info_hash> <aad> <pt>
//                                        -> ct || tag under the key and base nonce of
//                                           hpke_kdf512_key_nonce<kdf, 3> (kdf 2 or 3)
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../janus_amd/csrc/hpke_prims.h"

using namespace p3g;
typedef std::vector<uint8_t> Bytes;

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

static void le32_words(const Bytes& b, uint32_t* w) {
  for (size_t i = 0; i < b.size() / 4; ++i)
    w[i] = (uint32_t)b[4 * i] | (uint32_t)b[4 * i + 1] << 8 | (uint32_t)b[4 * i + 2] << 16 |
           (uint32_t)b[4 * i + 3] << 24;
}

// ct || tag in a block of exactly pt.size() + 16 bytes
static Bytes do_seal(const uint32_t key[8], const uint32_t nonce[3], const Bytes& aad,
                     const Bytes& pt) {
  Bytes ct(pt.size() + 16, 0xaa);
  ct.shrink_to_fit();
  chacha20poly1305_seal(key, nonce, PackedBytes{aad.data(), aad.size()},
                        PackedBytes{pt.data(), pt.size()}, ct.data());
  return ct;
}

template <int KDF>
static void kdf_key_nonce(const Bytes& ss, const Bytes& psk, const Bytes& info, uint32_t key[8],
                          uint32_t nonce[3]) {
  uint32_t ssw[8], pw[16], iw[16];
  uint64_t secret[8];
  be32_words(ss, ssw);
  be32_words(psk, pw);
  be32_words(info, iw);
  hpke_kdf512_key_nonce<KDF, 3>(ssw, pw, iw, secret, key, nonce);
  for (int i = 0; i < 8; ++i) key[i] = hp_bswap32(key[i]);  // big-endian words -> ChaCha20's
  for (int i = 0; i < 3; ++i) nonce[i] = hp_bswap32(nonce[i]);
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd, a, b, c, d, e;
    in >> cmd;
    Bytes x, y, z, u, v;
    if (cmd == "seal" || cmd == "rt") {
      in >> a >> b >> c >> d;
      if (!unhex(a, &x) || !unhex(b, &y) || !unhex(c, &z) || !unhex(d, &u) || x.size() != 32 ||
          y.size() != 12) {
        std::printf("err bad arguments\n");
        continue;
      }
      uint32_t key[8], nonce[3];
      le32_words(x, key);
      le32_words(y, nonce);
      const Bytes ct = do_seal(key, nonce, z, u);
      if (cmd == "seal") {
        std::printf("%s\n", hex(ct.data(), ct.size()).c_str());
        continue;
      }
      uint32_t tag[4];
      load_block(ct.data() + u.size(), 16, tag);
      Bytes body(ct.begin(), ct.begin() + u.size()), pt(u.size(), 0xaa);
      body.shrink_to_fit();
      const bool ok = chacha20poly1305_open(key, nonce, PackedBytes{z.data(), z.size()},
                                            PackedBytes{body.data(), body.size()}, tag, pt.data());
      std::printf("%d %s\n", ok ? 1 : 0, hex(pt.data(), pt.size()).c_str());
    } else if (cmd == "hseal") {
      int kdf = 0;
      in >> kdf >> a >> b >> c >> d >> e;
      const size_t nh = kdf == 2 ? 48 : 64;
      if ((kdf != 2 && kdf != 3) || !unhex(a, &x) || !unhex(b, &y) || !unhex(c, &z) ||
          !unhex(d, &u) || !unhex(e, &v) || x.size() != 32 || y.size() != nh || z.size() != nh) {
        std::printf("err bad arguments\n");
        continue;
      }
      uint32_t key[8], nonce[3];
      if (kdf == 2) kdf_key_nonce<2>(x, y, z, key, nonce);
      else kdf_key_nonce<3>(x, y, z, key, nonce);
      const Bytes ct = do_seal(key, nonce, u, v);
      std::printf("%s\n", hex(ct.data(), ct.size()).c_str());
    } else if (!cmd.empty()) {
      std::printf("err unknown command\n");
    }
  }
  return 0;
}
