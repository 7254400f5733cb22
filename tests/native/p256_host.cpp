// Driver of tests/test_p256_prims.py: janus_amd/csrc/p256.h and p256_kem.h (the field, curve and KEM code the GPU
// kernels k_p256_dh / k_p256_dh_idx run) built for the host.  A text protocol on stdin / stdout,
// one answer line per command; byte strings are hex, and every input is used from a heap block of
// exactly its length, so a sanitizer build sees any read past it:
//   fe <mul|sqr|add|sub|inv> <a> <b>   a, b: 32-byte big-endian values below p -> the result, after
//                                      a trip through Montgomery form; "noncanonical" if the raw
//                                      result is not below p
//   dec <enc>                          -> "1 <x> <y>" or "0" (any length; only 65 bytes can decode)
//   mul <k> <enc>                      k: 32-byte big-endian scalar in [1, n) -> x([k] P) or "invalid"
//   kem <dh> <enc> <pk>                -> the DHKEM shared secret (enc, pk: 65 bytes, not validated)
//   lane <k> <enc> <pk>                -> "<ok> <shared_secret>" of p256_dh_lane
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../janus_amd/csrc/p256_kem.h"

using namespace p3g;
typedef std::vector<uint8_t> Bytes;

static int nib(char c) {
  if (c >= '0' && c <= '9') return c - '0';
  if (c >= 'a' && c <= 'f') return c - 'a' + 10;
  return -1;
}

static bool unhex(std::string hex, Bytes* out) {
  if (hex == "-") hex.clear();
  if (hex.size() % 2) return false;
  out->resize(hex.size() / 2);
  out->shrink_to_fit();
  for (size_t i = 0; i < out->size(); ++i) {
    const int h = nib(hex[2 * i]), l = nib(hex[2 * i + 1]);
    if (h < 0 || l < 0) return false;
    (*out)[i] = (uint8_t)(h * 16 + l);
  }
  return true;
}

static std::string hex_be32(const uint32_t* w, int nwords) {
  static const char* d = "0123456789abcdef";
  std::string s;
  for (int i = 0; i < nwords; ++i)
    for (int sh = 28; sh >= 0; sh -= 4) s += d[(w[i] >> sh) & 15];
  return s;
}

static bool load_fe(const Bytes& b, Fp256* mont) {  // 32 big-endian bytes below p
  if (b.size() != 32) return false;
  uint32_t be[8];
  p256_load_be_words8(b.data(), be);
  Fp256 plain;
  fp_from_be(plain, be);
  if (!fp_is_canonical(plain)) return false;
  fp_to_mont(*mont, plain);
  return true;
}

static bool load_scalar(const Bytes& b, P256Scalar* k) {
  if (b.size() != 32) return false;
  uint32_t be[8];
  p256_load_be_words8(b.data(), be);
  for (int i = 0; i < 8; ++i) k->w[i] = be[7 - i];
  return true;
}

static void load_pk(const Bytes& b, P256PublicKey* pk) {  // 65 bytes
  p256_load_be_words8(b.data() + 1, pk->x);
  p256_load_be_words8(b.data() + 33, pk->y);
}

static void salt0_pads(uint32_t ist[8], uint32_t ost[8]) {  // HMAC-SHA256 under the empty salt
  uint32_t w[16];
  for (int i = 0; i < 16; ++i) w[i] = 0x36363636u;
  sha256_iv(ist);
  sha256_compress(ist, w);
  for (int i = 0; i < 16; ++i) w[i] = 0x5c5c5c5cu;
  sha256_iv(ost);
  sha256_compress(ost, w);
}

int main() {
  std::string line;
  uint32_t ist[8], ost[8];
  salt0_pads(ist, ost);
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd, op, a, b, c;
    in >> cmd;
    Bytes x, y, z;
    if (cmd == "fe") {
      in >> op >> a >> b;
      Fp256 fa, fb, r;
      if (!unhex(a, &x) || !unhex(b, &y) || !load_fe(x, &fa) || !load_fe(y, &fb)) {
        std::printf("err bad arguments\n");
        continue;
      }
      if (op == "mul") fp_mul(r, fa, fb);
      else if (op == "sqr") fp_sqr(r, fa);
      else if (op == "add") fp_add(r, fa, fb);
      else if (op == "sub") fp_sub(r, fa, fb);
      else if (op == "inv") fp_inv(r, fa);
      else {
        std::printf("err unknown operation\n");
        continue;
      }
      if (!fp_is_canonical(r)) {
        std::printf("noncanonical\n");
        continue;
      }
      fp_from_mont(r, r);
      uint32_t be[8];
      for (int i = 0; i < 8; ++i) be[i] = r.v[7 - i];
      std::printf("%s\n", hex_be32(be, 8).c_str());
    } else if (cmd == "dec") {
      in >> a;
      uint32_t xb[8], yb[8];
      Fp256 X, Y;
      if (!unhex(a, &x)) {
        std::printf("err bad arguments\n");
      } else if (x.size() != 65 || !p256_decode(x.data(), xb, yb, X, Y)) {
        std::printf("0\n");
      } else {
        std::printf("1 %s %s\n", hex_be32(xb, 8).c_str(), hex_be32(yb, 8).c_str());
      }
    } else if (cmd == "mul") {
      in >> a >> b;
      P256Scalar k;
      uint32_t xb[8], yb[8], out[8];
      Fp256 X, Y;
      if (!unhex(a, &x) || !unhex(b, &y) || !load_scalar(x, &k)) {
        std::printf("err bad arguments\n");
      } else if (y.size() != 65 || !p256_decode(y.data(), xb, yb, X, Y)) {
        std::printf("invalid\n");
      } else {
        p256_dh_x(k, X, Y, out);
        std::printf("%s\n", hex_be32(out, 8).c_str());
      }
    } else if (cmd == "kem") {
      in >> a >> b >> c;
      if (!unhex(a, &x) || !unhex(b, &y) || !unhex(c, &z) || x.size() != 32 || y.size() != 65 ||
          z.size() != 65) {
        std::printf("err bad arguments\n");
        continue;
      }
      uint32_t dh[8], ss[8];
      P256PublicKey e, pk;
      p256_load_be_words8(x.data(), dh);
      load_pk(y, &e);
      load_pk(z, &pk);
      p256_kem_shared_secret(ist, ost, dh, e.x, e.y, pk, ss);
      std::printf("%s\n", hex_be32(ss, 8).c_str());
    } else if (cmd == "lane") {
      in >> a >> b >> c;
      P256Scalar k;
      if (!unhex(a, &x) || !unhex(b, &y) || !unhex(c, &z) || !load_scalar(x, &k) ||
          z.size() != 65) {
        std::printf("err bad arguments\n");
        continue;
      }
      P256PublicKey pk;
      load_pk(z, &pk);
      uint32_t ss[8];
      const bool ok = p256_dh_lane(k, pk, ist, ost, y.data(), y.size() == 65, false, ss);
      std::printf("%d %s\n", ok ? 1 : 0, hex_be32(ss, 8).c_str());
    } else if (!cmd.empty()) {
      std::printf("err unknown command\n");
    }
  }
  return 0;
}
