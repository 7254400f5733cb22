// One report's HPKE open and seal after the DH (RFC 9180 base mode, single shot, sequence number
// 0), as one lane of hpke_gpu.h's, helper_request.h's and hpke_seal_gpu.h's kernels runs it: the
// key schedule (hpke_kdf256.h), then one AEAD call (aes_gcm.h or hpke_prims.h's
// ChaCha20-Poly1305), then the slot's tail and the report's status.  With them the two byte
// sources the request path and the client driver read through, ReqAad and SharePlaintext.
// Free of HIP like hpke_prims.h: the kernels and a CPU test (tests/native/hpke_lane_host.cpp)
// run the same text.
#pragma once
#include "aes_gcm.h"
#include "hpke_kdf256.h"

namespace p3g {

constexpr uint8_t ST_HPKE_DECRYPT = 4;  // PrepareError::HpkeDecryptError

// A report that is not opened: its slot is zeroed; status 4 unless it was skipped on entry.
DEVI void hpke_open_reject(uint8_t* pt, uint64_t pt_cap, uint8_t* status, bool skip) {
  for (uint64_t j = 0; j < pt_cap; ++j) pt[j] = 0;
  if (!skip) *status = ST_HPKE_DECRYPT;
}

// One report, one lane: derive (key, base_nonce) from the lane's dh (8 words as k_x25519 or
// k_p256_dh wrote them) and enc (32 bytes; not read for P-256), check the AEAD's tag over aad ||
// ct[0 .. body), then write the plaintext to pt[0 .. body) and zeros up to pt_cap -- or zeros and
// status 4 when the tag does not match or the DH failed: never unauthenticated plaintext.  The DH
// failed when dh is all zero (X25519, RFC 9180 §7.1.4) or, with bc.dh_ok set (P-256), when the
// report's flag dh_flag is zero -- there an all-zero value is no marker.  A failed DH is rejected
// after the key schedule and, for AES-GCM, after the AEAD has run: the same work as a bad tag.  ct
// holds body + 16 bytes.  sbox is unused (null) for ChaCha20-Poly1305.
template <int KDF, int AEAD, class Aad>
DEVI void hpke_open_lane(const uint8_t* sbox, const HpkeBatchConsts& bc, const uint32_t* dh,
                         uint32_t dh_flag, const uint8_t* enc, const Aad& aad, const uint8_t* ct,
                         uint64_t body, uint8_t* pt, uint64_t pt_cap, uint8_t* status) {
  uint32_t dhw[8], encw[8], nz = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t d = dh[i];
    nz |= d;
    dhw[i] = bswap32(d);
    encw[i] = 0;
  }
  if (bc.dh_ok) {
    nz = dh_flag;
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint8_t* e = enc + 4 * i;
      encw[i] = ((uint32_t)e[0] << 24) | ((uint32_t)e[1] << 16) | ((uint32_t)e[2] << 8) | e[3];
    }
  }
  constexpr int NKW = hpke_aead_nk(AEAD) / 4;
  uint32_t key[NKW], nonce[3], tag[4];
  hpke_key_nonce<KDF, AEAD>(bc, dhw, encw, key, nonce);
  if constexpr (AEAD == 3) {
#pragma unroll
    for (int i = 0; i < NKW; ++i) key[i] = bswap32(key[i]);
#pragma unroll
    for (int i = 0; i < 3; ++i) nonce[i] = bswap32(nonce[i]);
    load_block(ct + body, 16, tag);
    if (nz == 0u || !chacha20poly1305_open(key, nonce, aad, PackedBytes{ct, body}, tag, pt)) {
      hpke_open_reject(pt, pt_cap, status, false);
      return;
    }
  } else {
    load_block(ct + body, 16, tag);
    if (!aes_gcm_open<NKW>(sbox, key, nonce, aad, PackedBytes{ct, body}, tag, pt) || nz == 0u) {
      hpke_open_reject(pt, pt_cap, status, false);
      return;
    }
  }
  for (uint64_t j = body; j < pt_cap; ++j) pt[j] = 0;
}

// A report that is not sealed: zeros in its enc and ciphertext slots; status 4 unless it was
// skipped on entry.  nenc: the enc slot's bytes (HpkeBatchConsts::nenc).
DEVI void hpke_seal_reject(uint8_t* enc_out, uint8_t* ct, uint64_t ct_cap, uint8_t* status,
                           bool skip, uint32_t nenc = 32) {
  for (uint32_t j = 0; j < nenc; ++j) enc_out[j] = 0;
  for (uint64_t j = 0; j < ct_cap; ++j) ct[j] = 0;
  if (!skip) *status = ST_HPKE_DECRYPT;
}

// One report, one lane: derive (key, base_nonce) from the lane's enc and dh (8 little-endian words
// each, as k_x25519_eph wrote them), then AEAD-encrypt pt under aad with sequence number 0: enc_out
// gets the 32 bytes of enc, ct gets pt.len() + 16 bytes (ciphertext || tag) and zeros up to
// ct_cap -- or everything zeros and status 4 when the DH value is all zero (pkR of small order,
// RFC 9180 §7.1.4).  With bc.dh_ok set (P-256: k_p256_eph and k_p256_eph_kem have run) dh is the
// finished shared_secret, the report's flag dh_flag says whether its ephemeral scalar was valid
// (zero: everything zeros and status 4; an all-zero value is no marker there), and enc is the 64
// bytes x || y of the ephemeral point: enc_out gets the bc.nenc = 65 bytes 0x04 || x || y, at any
// alignment.  The KEM is a wave-uniform branch.  pt and aad are byte sources (len(), block(o, d)).
// sbox is unused (null) for ChaCha20-Poly1305.
template <int KDF, int AEAD, class Pt, class Aad>
DEVI void hpke_seal_lane(const uint8_t* sbox, const HpkeBatchConsts& bc, const uint32_t* enc,
                         const uint32_t* dh, const Pt& pt, const Aad& aad, uint8_t* enc_out,
                         uint8_t* ct, uint64_t ct_cap, uint8_t* status, uint32_t dh_flag = 1u) {
  uint32_t dhw[8], encw[8], ence[8], nz = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t d = dh[i];
    nz |= d;
    dhw[i] = bswap32(d);
    ence[i] = encw[i] = 0;
  }
  if (bc.dh_ok) {
    nz = dh_flag;
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      ence[i] = enc[i];
      encw[i] = bswap32(ence[i]);
    }
  }
  if (nz == 0u) {
    hpke_seal_reject(enc_out, ct, ct_cap, status, false, bc.nenc);
    return;
  }
  if (bc.dh_ok) {  // before the key schedule: nothing of enc stays live across it
    const uint8_t* xy = reinterpret_cast<const uint8_t*>(enc);
    enc_out[0] = 0x04;
    for (int j = 0; j < 64; ++j) enc_out[1 + j] = xy[j];
  }
  constexpr int NKW = hpke_aead_nk(AEAD) / 4;
  uint32_t key[NKW], nonce[3];
  hpke_key_nonce<KDF, AEAD>(bc, dhw, encw, key, nonce);
  if (!bc.dh_ok) {
    store_block(enc_out, 16, ence);
    store_block(enc_out + 16, 16, ence + 4);
  }
  const uint64_t plen = pt.len();
  if constexpr (AEAD == 3) {
#pragma unroll
    for (int i = 0; i < NKW; ++i) key[i] = bswap32(key[i]);
#pragma unroll
    for (int i = 0; i < 3; ++i) nonce[i] = bswap32(nonce[i]);
    chacha20poly1305_seal(key, nonce, aad, pt, ct);
  } else {
    aes_gcm_seal<NKW>(sbox, key, nonce, aad, pt, ct);
  }
  for (uint64_t j = plen + 16; j < ct_cap; ++j) ct[j] = 0;
}

// Where report r's enc and DH words lie in the seal ladders' output (hpke_dh_gpu.h):
// k_x25519_eph's n encs of 8 words, then n DH values; under P-256 (bc.dh_ok) n points of 16 words,
// then n shared secrets.
DEVI const uint32_t* eph_enc(const HpkeBatchConsts& bc, const uint32_t* eph, uint32_t r) {
  return eph + (size_t)r * (bc.dh_ok ? 16 : 8);
}
DEVI const uint32_t* eph_dh(const HpkeBatchConsts& bc, const uint32_t* eph, uint32_t n,
                            uint32_t r) {
  return eph + (size_t)n * (bc.dh_ok ? 16 : 8) + (size_t)r * 8;
}

struct ReqTaskId {  // the 32-byte TaskId as block words (byte j at bits 8 (j & 3) of word j >> 2)
  uint32_t w[8];
};

// InputShareAad (messages/src/lib.rs:1790-1827; hpke.cpp's open_i) as a GHASH / Poly1305 byte
// source:
//   task_id[32] | report_id[16] | time u64 BE | public_share_len u32 BE | public share
// Blocks 0, 1: the task id; block 2: the report ID; block 3: time, length and the first four
// public-share bytes; block k >= 4: public-share bytes 16 k - 60 ..., none on a block boundary.
struct ReqAad {
  ReqTaskId tid;
  const uint8_t* rid;
  uint64_t time;
  uint32_t pslen;
  const uint8_t* ps;
  DEVI uint64_t len() const { return 60 + (uint64_t)pslen; }
  DEVI void block(uint64_t o, uint32_t d[4]) const {
    if (o < 32) {
#pragma unroll
      for (int i = 0; i < 4; ++i) d[i] = o ? tid.w[4 + i] : tid.w[i];
    } else if (o == 32) {
      load_block(rid, 16, d);
    } else if (o == 48) {
      d[0] = bswap32((uint32_t)(time >> 32));
      d[1] = bswap32((uint32_t)time);
      d[2] = bswap32(pslen);
      d[3] = 0;
      for (uint32_t j = 0; j < 4 && j < pslen; ++j) d[3] |= (uint32_t)ps[j] << (8 * j);
    } else {
      load_block(ps + (o - 60), (uint64_t)pslen - (o - 60), d);
    }
  }
};

// PlaintextInputShare with no extensions (messages/src/lib.rs:1850-1895) as a byte source:
//   00 00 (the empty extension list) | payload length u32 BE | the input share
struct SharePlaintext {
  const uint8_t* share;
  uint32_t slen;
  DEVI uint64_t len() const { return 6 + (uint64_t)slen; }
  DEVI void block(uint64_t o, uint32_t d[4]) const {
    if (o == 0) {
      const uint32_t be = bswap32(slen);  // byte j of the big-endian length at bits 8 j
      d[0] = be << 16;
      d[1] = be >> 16;
      d[2] = d[3] = 0;
#pragma unroll
      for (int j = 0; j < 10; ++j)  // unrolled: d stays in registers
        if ((uint32_t)j < slen) d[(6 + j) >> 2] |= (uint32_t)share[j] << (8 * ((6 + j) & 3));
    } else {
      load_block(share + (o - 6), (uint64_t)slen - (o - 6), d);
    }
  }
  // block(o, d) where all sixteen bytes exist (o + 16 <= len()): one 16-byte load of the row, or
  // for block 0 the header from registers and the row's first ten bytes
  DEVI void whole(uint64_t o, uint32_t d[4]) const {
    if (o == 0) {
      const uint32_t be = bswap32(slen);
      uint64_t lo;
      uint16_t hi;
      __builtin_memcpy(&lo, share, 8);
      __builtin_memcpy(&hi, share + 8, 2);
      d[0] = be << 16;
      d[1] = (be >> 16) | ((uint32_t)lo << 16);
      d[2] = (uint32_t)(lo >> 16);
      d[3] = (uint32_t)(lo >> 48) | ((uint32_t)hi << 16);
    } else {
      __builtin_memcpy(d, share + (o - 6), 16);
    }
  }
};

}  // namespace p3g
