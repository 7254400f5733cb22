// Driver of tests/test_hpke_prims.py: janus_amd/csrc/hpke_prims.h (the SHA-512, HMAC, key
// schedule, ChaCha20 and Poly1305 the GPU kernels of hpke_gpu.h run) built for the host.  A text
// protocol on stdin / stdout, one answer line per command; byte strings are hex, "-" when empty,
// and every input is used from a heap block of exactly its length, so a sanitizer build sees any
// read past it:
//   sha <kdf> <msg>                      -> SHA-384 (kdf 2) / SHA-512 (kdf 3) of msg (<= 240 bytes)
//   hmac <kdf> <key> <msg>               -> HMAC; key 32, 48 or 64 bytes, msg <= 240 bytes
//   poly <key r||s> <msg>                -> the Poly1305 tag
//   ks <kdf> <aead> <shared_secret> <psk_id_hash> <info_hash>   -> "<secret> <key> <base_nonce>"
//   open <key> <nonce> <aad> <ct || tag> -> "<1 | 0> <plaintext>" of chacha20poly1305_open; the
//                                           plaintext block is preset to 0xaa
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

static std::string hex_be64(const uint64_t* w, int nbytes) {
  Bytes b(nbytes);
  for (int i = 0; i < nbytes; ++i) b[i] = (uint8_t)(w[i >> 3] >> (56 - 8 * (i & 7)));
  return hex(b.data(), b.size());
}

static std::string hex_be32(const uint32_t* w, int nbytes) {
  Bytes b(nbytes);
  for (int i = 0; i < nbytes; ++i) b[i] = (uint8_t)(w[i >> 2] >> (24 - 8 * (i & 3)));
  return hex(b.data(), b.size());
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

// msg (<= 240 bytes) as padded blocks after `before` hashed bytes; returns the block count
static int padded(const Bytes& msg, int before, uint64_t w[48]) {
  for (int i = 0; i < 48; ++i) w[i] = 0;
  for (size_t i = 0; i < msg.size(); ++i) msg64_byte(w, (int)i, msg[i]);
  const int nblk = ((int)msg.size() + 17 + 127) / 128;
  msg64_pad(w, (int)msg.size(), nblk, before);
  return nblk;
}

template <int KDF>
static std::string do_sha(const Bytes& msg) {
  uint64_t w[48], h[8];
  const int nblk = padded(msg, 0, w);
  if (KDF == 2) sha384_iv(h); else sha512_iv(h);
  for (int b = 0; b < nblk; ++b) sha512_compress(h, w + 16 * b);
  return hex_be64(h, Kdf512<KDF>::NH);
}

template <int KDF>
static std::string do_hmac(const Bytes& key, const Bytes& msg) {
  uint64_t kw[8] = {0}, w[48], ist[8], ost[8], out[8];
  for (size_t i = 0; i < key.size(); ++i) msg64_byte(kw, (int)i, key[i]);
  hmac512_pads<KDF>(kw, (int)key.size() / 8, ist, ost);
  const int nblk = padded(msg, 128, w);
  if (nblk == 1) hmac512_finish<KDF, 1>(ist, ost, w, out);
  else if (nblk == 2) hmac512_finish<KDF, 2>(ist, ost, w, out);
  else hmac512_finish<KDF, 3>(ist, ost, w, out);
  return hex_be64(out, Kdf512<KDF>::NH);
}

template <int KDF, int AEAD>
static std::string do_ks(const Bytes& ss, const Bytes& psk, const Bytes& info) {
  uint32_t ssw[8], pw[16], iw[16], key[8], nonce[3];
  uint64_t secret[8];
  be32_words(ss, ssw);
  be32_words(psk, pw);
  be32_words(info, iw);
  hpke_kdf512_key_nonce<KDF, AEAD>(ssw, pw, iw, secret, key, nonce);
  return hex_be64(secret, Kdf512<KDF>::NH) + " " + hex_be32(key, hpke_aead_nk(AEAD)) + " " +
         hex_be32(nonce, 12);
}

template <int KDF>
static std::string do_ks_aead(int aead, const Bytes& ss, const Bytes& psk, const Bytes& info) {
  if (aead == 1) return do_ks<KDF, 1>(ss, psk, info);
  if (aead == 2) return do_ks<KDF, 2>(ss, psk, info);
  return do_ks<KDF, 3>(ss, psk, info);
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd, a, b, c, d;
    int kdf = 0, aead = 0;
    in >> cmd;
    Bytes x, y, z, u;
    if (cmd == "sha") {
      in >> kdf >> a;
      if ((kdf != 2 && kdf != 3) || !unhex(a, &x) || x.size() > 240) {
        std::printf("err bad arguments\n");
        continue;
      }
      std::printf("%s\n", (kdf == 2 ? do_sha<2>(x) : do_sha<3>(x)).c_str());
    } else if (cmd == "hmac") {
      in >> kdf >> a >> b;
      if ((kdf != 2 && kdf != 3) || !unhex(a, &x) || !unhex(b, &y) || y.size() > 240 ||
          (x.size() != 32 && x.size() != 48 && x.size() != 64)) {
        std::printf("err bad arguments\n");
        continue;
      }
      std::printf("%s\n", (kdf == 2 ? do_hmac<2>(x, y) : do_hmac<3>(x, y)).c_str());
    } else if (cmd == "poly") {
      in >> a >> b;
      if (!unhex(a, &x) || !unhex(b, &y) || x.size() != 32) {
        std::printf("err bad arguments\n");
        continue;
      }
      uint32_t k[8], tag[4];
      le32_words(x, k);
      poly1305_mac(k, y.data(), y.size(), tag);
      uint8_t t[16];
      for (int j = 0; j < 16; ++j) t[j] = (uint8_t)(tag[j >> 2] >> (8 * (j & 3)));
      std::printf("%s\n", hex(t, 16).c_str());
    } else if (cmd == "ks") {
      in >> kdf >> aead >> a >> b >> c;
      const size_t nh = kdf == 2 ? 48 : 64;
      if ((kdf != 2 && kdf != 3) || aead < 1 || aead > 3 || !unhex(a, &x) || !unhex(b, &y) ||
          !unhex(c, &z) || x.size() != 32 || y.size() != nh || z.size() != nh) {
        std::printf("err bad arguments\n");
        continue;
      }
      std::printf("%s\n",
                  (kdf == 2 ? do_ks_aead<2>(aead, x, y, z) : do_ks_aead<3>(aead, x, y, z)).c_str());
    } else if (cmd == "open") {
      in >> a >> b >> c >> d;
      if (!unhex(a, &x) || !unhex(b, &y) || !unhex(c, &z) || !unhex(d, &u) || x.size() != 32 ||
          y.size() != 12 || u.size() < 16) {
        std::printf("err bad arguments\n");
        continue;
      }
      uint32_t key[8], nonce[3], tag[4];
      le32_words(x, key);
      le32_words(y, nonce);
      const size_t body = u.size() - 16;
      load_block(u.data() + body, 16, tag);
      Bytes ct(u.begin(), u.begin() + body), pt(body, 0xaa);
      ct.shrink_to_fit();
      const bool ok = chacha20poly1305_open(key, nonce, PackedBytes{z.data(), z.size()},
                                            PackedBytes{ct.data(), ct.size()}, tag, pt.data());
      std::printf("%d %s\n", ok ? 1 : 0, hex(pt.data(), pt.size()).c_str());
    } else if (!cmd.empty()) {
      std::printf("err unknown command\n");
    }
  }
  return 0;
}
