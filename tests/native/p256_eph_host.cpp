// Driver of tests/test_p256_eph_prims.py: the sender's side of DHKEM(P-256, HKDF-SHA256) as the
// GPU seal runs it per report (janus_amd/csrc/p256.h's ladder with the lane's own scalar,
// p256_kem.h's p256_eph_lane and p256_eph_shared_secret, hpke_lane.h's hpke_seal_lane with
// bc.dh_ok set; the kernels k_p256_eph, k_p256_eph_kem and k_hpke_seal* of hpke_seal_gpu.h) built
// for the host.  A text protocol on stdin / stdout, one answer line per command; byte strings are
// hex, "-" when empty, and every input is used from a heap block of exactly its length and every
// output written to one of exactly its length, so a sanitizer build sees any access past either:
//   mulxy <k> <enc>     k: 32 big-endian bytes, any value; enc: a 65-byte point
//                       -> "<ok> <x> <y>" of p256_eph_lane, or "invalid" for a refused point
//   mulx <k> <enc>      k in [1, n) -> x([k] P) of p256_dh_x with the lane's own scalar
//   eph <sk_e> <pk>     -> "<ok> <enc> <shared_secret>": both ladders and the KEM half of one
//                       report, as k_p256_eph's two lanes and k_p256_eph_kem compute them
//   lseal <kdf> <aead> <psk_id_hash> <info_hash> <sk_e> <pk> <aad> <pt> <ct_cap>
//                       -> "<status> <enc_out[0 .. 65)> <ct[0 .. ct_cap)>" of hpke_seal_lane over
//                       the output of `eph` laid out as the kernels read it (both presets 0xaa)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../janus_amd/csrc/hpke_lane.h"
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

static std::string hex(const uint8_t* p, size_t n) {
  static const char* d = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; ++i) {
    s += d[p[i] >> 4];
    s += d[p[i] & 15];
  }
  return s;
}

static std::string hex_be32(const uint32_t* w, int nwords) {
  static const char* d = "0123456789abcdef";
  std::string s;
  for (int i = 0; i < nwords; ++i)
    for (int sh = 28; sh >= 0; sh -= 4) s += d[(w[i] >> sh) & 15];
  return s;
}

static Bytes block(size_t n) {  // a heap block of exactly n bytes, preset
  Bytes b(n, 0xaa);
  b.shrink_to_fit();
  return b;
}

static void be32_words(const Bytes& b, uint32_t* w) {
  for (size_t i = 0; i < b.size() / 4; ++i)
    w[i] = (uint32_t)b[4 * i] << 24 | (uint32_t)b[4 * i + 1] << 16 | (uint32_t)b[4 * i + 2] << 8 |
           b[4 * i + 3];
}

static const uint8_t kG[65] = {
    0x04, 0x6b, 0x17, 0xd1, 0xf2, 0xe1, 0x2c, 0x42, 0x47, 0xf8, 0xbc, 0xe6, 0xe5, 0x63, 0xa4,
    0x40, 0xf2, 0x77, 0x03, 0x7d, 0x81, 0x2d, 0xeb, 0x33, 0xa0, 0xf4, 0xa1, 0x39, 0x45, 0xd8,
    0x98, 0xc2, 0x96, 0x4f, 0xe3, 0x42, 0xe2, 0xfe, 0x1a, 0x7f, 0x9b, 0x8e, 0xe7, 0xeb, 0x4a,
    0x7c, 0x0f, 0x9e, 0x16, 0x2b, 0xce, 0x33, 0x57, 0x6b, 0x31, 0x5e, 0xce, 0xcb, 0xb6, 0x40,
    0x68, 0x37, 0xbf, 0x51, 0xf5};

static void salt0_pads(uint32_t ist[8], uint32_t ost[8]) {  // HMAC-SHA256 under the empty salt
  uint32_t w[16];
  for (int i = 0; i < 16; ++i) w[i] = 0x36363636u;
  sha256_iv(ist);
  sha256_compress(ist, w);
  for (int i = 0; i < 16; ++i) w[i] = 0x5c5c5c5cu;
  sha256_iv(ost);
  sha256_compress(ost, w);
}

// One report's ladders and KEM half in the kernels' order and layout: out[0 .. 64) the ephemeral
// point's x || y, out[64 .. 96) the shared secret, out[96] the validity byte.  false for a pk that
// is no point (the engine refuses it before any launch).
static bool eph_report(const uint32_t ist[8], const uint32_t ost[8], const Bytes& sk_e,
                       const Bytes& pk, uint8_t out[97]) {
  uint32_t gx[8], gy[8], px[8], py[8];
  Fp256 GX, GY, PX, PY;
  if (pk.size() != 65 || sk_e.size() != 32 || !p256_decode(kG, gx, gy, GX, GY) ||
      !p256_decode(pk.data(), px, py, PX, PY))
    return false;
  uint32_t ex[8], ey[8], dh[8], dy[8], ss[8];
  const bool ok0 = p256_eph_lane(sk_e.data(), GX, GY, ex, ey);  // blockIdx.y = 0
  const bool ok1 = p256_eph_lane(sk_e.data(), PX, PY, dh, dy);  // blockIdx.y = 1
  if (ok0 != ok1) return false;
  P256PublicKey pkw;
  for (int i = 0; i < 8; ++i) pkw.x[i] = px[i], pkw.y[i] = py[i];
  p256_eph_shared_secret(ist, ost, dh, ex, ey, pkw, ok0, ss);
  for (int i = 0; i < 8; ++i)
    for (int b = 0; b < 4; ++b) {
      out[4 * i + b] = (uint8_t)(ex[i] >> (24 - 8 * b));
      out[32 + 4 * i + b] = (uint8_t)(ey[i] >> (24 - 8 * b));
      out[64 + 4 * i + b] = (uint8_t)(ss[i] >> (24 - 8 * b));
    }
  out[96] = ok0 ? 1 : 0;
  return true;
}

template <int KDF, int AEAD>
static std::string lane_seal(const HpkeBatchConsts& bc, const uint8_t eph[97], const Bytes& aad,
                             const Bytes& pt, size_t cap) {
  uint8_t sbox[256];
  aes_sbox_fill(sbox, 0, 1);
  uint32_t encw[16], dhw[8];  // aligned words over the bytes, as the kernels' buffer holds them
  memcpy(encw, eph, 64);
  memcpy(dhw, eph + 64, 32);
  Bytes enc_out = block(65), ct = block(cap);
  uint8_t status = 0;
  hpke_seal_lane<KDF, AEAD>(AEAD == 3 ? nullptr : sbox, bc, encw, dhw,
                            PackedBytes{pt.data(), pt.size()}, PackedBytes{aad.data(), aad.size()},
                            enc_out.data(), ct.data(), cap, &status, eph[96]);
  return std::to_string(status) + " " + hex(enc_out.data(), 65) + " " + hex(ct.data(), ct.size());
}

static std::string lane_suite(int kdf, int aead, const HpkeBatchConsts& bc, const uint8_t eph[97],
                              const Bytes& aad, const Bytes& pt, size_t cap) {
  switch (10 * kdf + aead) {
    case 11: return lane_seal<1, 1>(bc, eph, aad, pt, cap);
    case 12: return lane_seal<1, 2>(bc, eph, aad, pt, cap);
    case 13: return lane_seal<1, 3>(bc, eph, aad, pt, cap);
    case 21: return lane_seal<2, 1>(bc, eph, aad, pt, cap);
    case 22: return lane_seal<2, 2>(bc, eph, aad, pt, cap);
    case 23: return lane_seal<2, 3>(bc, eph, aad, pt, cap);
    case 31: return lane_seal<3, 1>(bc, eph, aad, pt, cap);
    case 32: return lane_seal<3, 2>(bc, eph, aad, pt, cap);
    case 33: return lane_seal<3, 3>(bc, eph, aad, pt, cap);
  }
  return "err bad suite";
}

int main() {
  std::string line;
  uint32_t ist[8], ost[8];
  salt0_pads(ist, ost);
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd, a, b;
    in >> cmd;
    Bytes x, y;
    if (cmd == "mulxy" || cmd == "mulx") {
      in >> a >> b;
      uint32_t xb[8], yb[8], ox[8], oy[8];
      Fp256 X, Y;
      if (!unhex(a, &x) || !unhex(b, &y) || x.size() != 32) {
        std::printf("err bad arguments\n");
      } else if (y.size() != 65 || !p256_decode(y.data(), xb, yb, X, Y)) {
        std::printf("invalid\n");
      } else if (cmd == "mulxy") {
        const bool ok = p256_eph_lane(x.data(), X, Y, ox, oy);
        std::printf("%d %s %s\n", ok ? 1 : 0, hex_be32(ox, 8).c_str(), hex_be32(oy, 8).c_str());
      } else {
        P256LaneScalar k;
        if (!p256_lane_scalar(x.data(), k)) {
          std::printf("err scalar outside [1, n)\n");
          continue;
        }
        p256_dh_x(k, X, Y, ox);
        std::printf("%s\n", hex_be32(ox, 8).c_str());
      }
    } else if (cmd == "eph") {
      in >> a >> b;
      uint8_t out[97];
      if (!unhex(a, &x) || !unhex(b, &y) || !eph_report(ist, ost, x, y, out)) {
        std::printf("err bad arguments\n");
        continue;
      }
      std::printf("%d %s%s %s\n", out[96], out[96] ? "04" : "00", hex(out, 64).c_str(),
                  hex(out + 64, 32).c_str());
    } else if (cmd == "lseal") {
      int kdf = 0, aead = 0;
      std::string psk, info, ske, pk, aad, pt;
      size_t cap = 0;
      in >> kdf >> aead >> psk >> info >> ske >> pk >> aad >> pt >> cap;
      Bytes bpsk, binfo, bske, bpk, baad, bpt;
      uint8_t eph[97];
      if (!unhex(psk, &bpsk) || !unhex(info, &binfo) || !unhex(ske, &bske) || !unhex(pk, &bpk) ||
          !unhex(aad, &baad) || !unhex(pt, &bpt) || bpsk.size() > 64 || binfo.size() > 64 ||
          !eph_report(ist, ost, bske, bpk, eph)) {
        std::printf("err bad arguments\n");
        continue;
      }
      HpkeBatchConsts bc = {};
      bc.kdf_id = (uint32_t)kdf;
      bc.aead_id = (uint32_t)aead;
      be32_words(bpsk, bc.psk_id_hash);
      be32_words(binfo, bc.info_hash);
      for (int i = 0; i < 8; ++i) bc.salt0_i[i] = ist[i], bc.salt0_o[i] = ost[i];
      bc.kem_lo = 0x10;
      bc.nenc = 65;
      bc.dh_ok = eph + 96;
      std::printf("%s\n", lane_suite(kdf, aead, bc, eph, baad, bpt, cap).c_str());
    } else if (!cmd.empty()) {
      std::printf("err unknown command\n");
    }
  }
  return 0;
}
