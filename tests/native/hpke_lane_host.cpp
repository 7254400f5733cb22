// Driver of tests/test_hpke_lane_prims.py: the per-lane code of the GPU HPKE open and seal
// (janus_amd/csrc/x25519.h, hpke_kdf256.h, aes_gcm.h, hpke_lane.h; what the kernels of hpke_gpu.h,
// helper_request.h and hpke_seal_gpu.h run per report) built for the host.  A text protocol on
// stdin / stdout, one answer line per command; byte strings are hex, "-" when empty, and every
// input is used from a heap block of exactly its length and every output written to one of
// exactly its length, so a sanitizer build sees any access past either:
//   x25519 <scalar> <u>                  -> x25519_lane(clamp(scalar), u)
//   x25519iter <n>                       -> RFC 7748 §5.2's iteration from k = u = 9, n rounds
//   sbox <step>                          -> the S-box filled by aes_sbox_fill(sbox, t, step), t < step
//   aes <key> <block>                    -> aes_encrypt of the block under aes_expand(key), 16 / 32
//   gcmseal <key> <nonce> <aad> <pt>     -> ct || tag of aes_gcm_seal
//   gcmopen <key> <nonce> <aad> <ct || tag>
//                                        -> "<1 | 0> <plaintext>" of aes_gcm_open (the plaintext
//                                           block is preset to 0xaa)
//   lseal <kdf> <aead> <pkR> <psk_id_hash> <info_hash> <enc> <dh> <aad> <pt> <ct_cap>
//                                        -> "<status> <enc_out> <ct[0 .. ct_cap)>" of hpke_seal_lane
//                                           (both presets 0xaa)
//   lopen <kdf> <aead> <kem> <pkR> <psk_id_hash> <info_hash> <enc> <dh> <dh_flag> <aad>
//         <ct || tag> <pt_cap>           -> "<status> <pt[0 .. pt_cap)>" of hpke_open_lane (preset
//                                           0xaa).  kem 32: X25519, dh is the DH value; kem 16:
//                                           the P-256 form (bc.dh_ok set), dh is the shared_secret,
//                                           dh_flag its validity, pkR and enc are not read ("-")
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../janus_amd/csrc/hpke_lane.h"
#include "../../janus_amd/csrc/x25519.h"

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

static Bytes le32_bytes(const uint32_t* w, size_t n) {
  Bytes b(4 * n);
  for (size_t i = 0; i < 4 * n; ++i) b[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
  return b;
}

static Bytes block(size_t n) {  // exactly n bytes, preset
  Bytes b(n, 0xaa);
  b.shrink_to_fit();
  return b;
}

// X25519(scalar, u) on 32-byte strings; the scalar is clamped as k_x25519_eph and the host do
static Bytes x25519(const Bytes& scalar, const Bytes& u) {
  X25519Scalar k;
  uint32_t w[8];
  load_le_words8(scalar.data(), k.w);
  k.w[0] &= ~7u;
  k.w[7] = (k.w[7] & 0x7FFFFFFFu) | 0x40000000u;
  load_le_words8(u.data(), w);
  x25519_lane(k, w);
  return le32_bytes(w, 8);
}

static void fill_sbox(uint8_t* sbox, uint32_t step) {
  for (uint32_t t = 0; t < step; ++t) aes_sbox_fill(sbox, t, step);
}

template <int NK>
static Bytes aes_block(const Bytes& key, const Bytes& in) {
  uint8_t sbox[256];
  uint32_t kw[NK], rk[4 * (NK + 7)], x[4], y[4];
  fill_sbox(sbox, 1);
  be32_words(key, kw);
  aes_expand<NK>(sbox, kw, rk);
  load_block(in.data(), 16, x);
  aes_encrypt<NK>(sbox, rk, x, y);
  return le32_bytes(y, 4);
}

template <int NK>
static Bytes gcm_seal(const Bytes& key, const Bytes& nonce, const Bytes& aad, const Bytes& pt) {
  uint8_t sbox[256];
  uint32_t kw[NK], nw[3];
  fill_sbox(sbox, 1);
  be32_words(key, kw);
  be32_words(nonce, nw);
  Bytes ct = block(pt.size() + 16);
  aes_gcm_seal<NK>(sbox, kw, nw, PackedBytes{aad.data(), aad.size()},
                   PackedBytes{pt.data(), pt.size()}, ct.data());
  return ct;
}

template <int NK>
static bool gcm_open(const Bytes& key, const Bytes& nonce, const Bytes& aad, const Bytes& ct,
                     Bytes* pt) {
  uint8_t sbox[256];
  uint32_t kw[NK], nw[3], tag[4];
  fill_sbox(sbox, 1);
  be32_words(key, kw);
  be32_words(nonce, nw);
  const size_t body = ct.size() - 16;
  load_block(ct.data() + body, 16, tag);
  Bytes text(ct.begin(), ct.begin() + body);  // the body alone: a read past it is past the block
  text.shrink_to_fit();
  *pt = block(body);
  return aes_gcm_open<NK>(sbox, kw, nw, PackedBytes{aad.data(), aad.size()},
                          PackedBytes{text.data(), text.size()}, tag, pt->data());
}

// the batch's constants as hpke.cpp's hpke_batch_consts gives them; the pad states of the empty
// salt are those of an all-zero key
static HpkeBatchConsts consts(int kdf, int aead, int kem, const Bytes& pk, const Bytes& psk,
                              const Bytes& info, const uint8_t* dh_ok) {
  HpkeBatchConsts bc = {};
  bc.kdf_id = (uint32_t)kdf;
  bc.aead_id = (uint32_t)aead;
  be32_words(pk, bc.pk);
  be32_words(psk, bc.psk_id_hash);
  be32_words(info, bc.info_hash);
  const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  hmac_pads(zero, bc.salt0_i, bc.salt0_o);
  bc.kem_lo = (uint32_t)kem;
  bc.nenc = kem == 0x20 ? 32 : 65;
  bc.dh_ok = dh_ok;
  return bc;
}

struct LaneArgs {
  Bytes enc, dh, aad, text;
  uint32_t dh_flag;
  size_t cap;
};

template <int KDF, int AEAD>
static std::string lane_seal(const HpkeBatchConsts& bc, const uint8_t* sbox, const LaneArgs& a) {
  uint32_t encw[8], dhw[8];
  le32_words(a.enc, encw);
  le32_words(a.dh, dhw);
  Bytes enc_out = block(32), ct = block(a.cap);
  uint8_t status = 0;
  hpke_seal_lane<KDF, AEAD>(sbox, bc, encw, dhw, PackedBytes{a.text.data(), a.text.size()},
                            PackedBytes{a.aad.data(), a.aad.size()}, enc_out.data(), ct.data(),
                            a.cap, &status);
  return std::to_string(status) + " " + hex(enc_out.data(), 32) + " " + hex(ct.data(), ct.size());
}

template <int KDF, int AEAD>
static std::string lane_open(const HpkeBatchConsts& bc, const uint8_t* sbox, const LaneArgs& a) {
  uint32_t dhw[8];
  le32_words(a.dh, dhw);
  Bytes pt = block(a.cap);
  uint8_t status = 0;
  hpke_open_lane<KDF, AEAD>(sbox, bc, dhw, a.dh_flag, a.enc.data(),
                            PackedBytes{a.aad.data(), a.aad.size()}, a.text.data(),
                            a.text.size() - 16, pt.data(), a.cap, &status);
  return std::to_string(status) + " " + hex(pt.data(), pt.size());
}

template <int KDF, int AEAD>
static std::string lane(bool seal, const HpkeBatchConsts& bc, const uint8_t* sbox,
                        const LaneArgs& a) {
  return seal ? lane_seal<KDF, AEAD>(bc, sbox, a) : lane_open<KDF, AEAD>(bc, sbox, a);
}

static std::string lane_suite(int kdf, int aead, bool seal, const HpkeBatchConsts& bc,
                              const LaneArgs& a) {
  uint8_t sbox[256];
  fill_sbox(sbox, 1);
  const uint8_t* sb = aead == 3 ? nullptr : sbox;  // as the kernels pass it
  switch (10 * kdf + aead) {
    case 11: return lane<1, 1>(seal, bc, sb, a);
    case 12: return lane<1, 2>(seal, bc, sb, a);
    case 13: return lane<1, 3>(seal, bc, sb, a);
    case 21: return lane<2, 1>(seal, bc, sb, a);
    case 22: return lane<2, 2>(seal, bc, sb, a);
    case 23: return lane<2, 3>(seal, bc, sb, a);
    case 31: return lane<3, 1>(seal, bc, sb, a);
    case 32: return lane<3, 2>(seal, bc, sb, a);
    case 33: return lane<3, 3>(seal, bc, sb, a);
  }
  return "err bad suite";
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd, a, b, c, d;
    in >> cmd;
    Bytes x, y, z, u;
    if (cmd == "x25519") {
      in >> a >> b;
      if (!unhex(a, &x) || !unhex(b, &y) || x.size() != 32 || y.size() != 32) {
        std::printf("err bad arguments\n");
        continue;
      }
      std::printf("%s\n", hex(x25519(x, y).data(), 32).c_str());
    } else if (cmd == "x25519iter") {
      int n = 0;
      in >> n;
      Bytes k(32, 0), v(32, 0);
      k[0] = v[0] = 9;
      for (int i = 0; i < n; ++i) {
        Bytes r = x25519(k, v);
        v = k;
        k = r;
      }
      std::printf("%s\n", hex(k.data(), 32).c_str());
    } else if (cmd == "sbox") {
      uint32_t step = 0;
      in >> step;
      Bytes s = block(256);
      if (step == 0 || step > 256) {
        std::printf("err bad arguments\n");
        continue;
      }
      fill_sbox(s.data(), step);
      std::printf("%s\n", hex(s.data(), 256).c_str());
    } else if (cmd == "aes") {
      in >> a >> b;
      if (!unhex(a, &x) || !unhex(b, &y) || (x.size() != 16 && x.size() != 32) || y.size() != 16) {
        std::printf("err bad arguments\n");
        continue;
      }
      const Bytes o = x.size() == 16 ? aes_block<4>(x, y) : aes_block<8>(x, y);
      std::printf("%s\n", hex(o.data(), 16).c_str());
    } else if (cmd == "gcmseal" || cmd == "gcmopen") {
      in >> a >> b >> c >> d;
      const bool open = cmd == "gcmopen";
      if (!unhex(a, &x) || !unhex(b, &y) || !unhex(c, &z) || !unhex(d, &u) ||
          (x.size() != 16 && x.size() != 32) || y.size() != 12 || (open && u.size() < 16)) {
        std::printf("err bad arguments\n");
        continue;
      }
      if (!open) {
        const Bytes ct = x.size() == 16 ? gcm_seal<4>(x, y, z, u) : gcm_seal<8>(x, y, z, u);
        std::printf("%s\n", hex(ct.data(), ct.size()).c_str());
      } else {
        Bytes pt;
        const bool ok = x.size() == 16 ? gcm_open<4>(x, y, z, u, &pt) : gcm_open<8>(x, y, z, u, &pt);
        std::printf("%d %s\n", ok ? 1 : 0, hex(pt.data(), pt.size()).c_str());
      }
    } else if (cmd == "lseal" || cmd == "lopen") {
      const bool seal = cmd == "lseal";
      int kdf = 0, aead = 0, kem = 0x20;
      std::string pk, psk, info, enc, dh, aad, text;
      Bytes pkb, pskb, infob;
      LaneArgs la;
      la.dh_flag = 1;
      in >> kdf >> aead;
      if (!seal) in >> kem;
      in >> pk >> psk >> info >> enc >> dh;
      if (!seal) in >> la.dh_flag;
      in >> aad >> text >> la.cap;
      const size_t nh = kdf == 1 ? 32 : kdf == 2 ? 48 : 64;
      const bool p256 = kem == 0x10;
      if (!in || kdf < 1 || kdf > 3 || aead < 1 || aead > 3 || (kem != 0x20 && !p256) ||
          !unhex(pk, &pkb) || !unhex(psk, &pskb) || !unhex(info, &infob) || !unhex(enc, &la.enc) ||
          !unhex(dh, &la.dh) || !unhex(aad, &la.aad) || !unhex(text, &la.text) ||
          pkb.size() != (p256 ? 0u : 32u) || pskb.size() != nh || infob.size() != nh ||
          la.enc.size() != (p256 ? 0u : 32u) || la.dh.size() != 32 ||
          (seal ? la.text.size() + 16 > la.cap : la.text.size() < 16 || la.text.size() - 16 > la.cap)) {
        std::printf("err bad arguments\n");
        continue;
      }
      const uint8_t flags[1] = {1};  // only its address is used: the lane gets dh_flag itself
      const HpkeBatchConsts bc = consts(kdf, aead, kem, pkb, pskb, infob, p256 ? flags : nullptr);
      std::printf("%s\n", lane_suite(kdf, aead, seal, bc, la).c_str());
    } else if (!cmd.empty()) {
      std::printf("err unknown command\n");
    }
  }
  return 0;
}
