// Batched HPKE seal on the GPU for DHKEM(X25519, HKDF-SHA256) with every KDF and AEAD Janus accepts
// (KDF 1-3 x AEAD 1-3), RFC 9180 base mode, single shot: what a DAP client does once per input
// share (client/src/lib.rs:212-258, core/src/hpke.rs:158-182).  The mirror image of hpke_gpu.h's
// open, one lane per report, every report of a launch to ONE recipient key, each under its own
// ephemeral key:
//   k_x25519_eph               enc = X25519(skE, 9), dh = X25519(skE, pkR)         RFC 9180 §4.1
//   k_hpke_seal<KDF, AEAD>     key schedule + AEAD encryption over packed plaintexts and AADs
//   k_hpke_seal_shares<KDF, AEAD>   the same over Prio3 input shares: the PlaintextInputShare and
//                              the InputShareAad are byte sources over the caller's rows and are
//                              never written to memory
// The two ladders of a report run on two lanes of one launch (blockIdx.y picks the point), each
// the unchanged x25519_lane with the lane's own scalar: one ladder's registers per lane, no
// scratch, and twice the lanes for the latency-bound field arithmetic to hide behind.
// Included by engine_hpke.hip after helper_request.h (ReqAad is the InputShareAad source).
#pragma once
#include "hpke_gpu.h"
#include "helper_request.h"

namespace p3g {

struct X25519Point {  // a u coordinate as little-endian words; a kernel argument
  uint32_t w[8];
};

// out[which n 8 + r 8 ..] = X25519(sk_es[r], which ? pkR : 9) as 8 little-endian words:
// blockIdx.y = 0 the encapsulated keys, 1 the DH values.  The scalar is clamped here
// (decodeScalar25519); its bits are read with selects inside x25519_lane, so no branch and no
// address depends on it or on a field value.
__global__ void __launch_bounds__(64) k_x25519_eph(uint32_t n, const uint8_t* sk_es,
                                                   X25519Point pk, uint32_t* out) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t which = blockIdx.y;
  const bool live = r < n;
  X25519Scalar k;
  load_le_words8(sk_es + (size_t)(live ? r : n - 1) * 32, k.w);
  k.w[0] &= ~7u;
  k.w[7] = (k.w[7] & 0x7FFFFFFFu) | 0x40000000u;
  uint32_t w[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = which ? pk.w[i] : (i ? 0u : 9u);
  x25519_lane(k, w);
  if (live) {
    uint32_t* o = out + ((size_t)which * n + r) * 8;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = w[i];
  }
}

// A report that is not sealed: zeros in its enc and ciphertext slots; status 4 unless it was
// skipped on entry.
DEVI void hpke_seal_reject(uint8_t* enc_out, uint8_t* ct, uint64_t ct_cap, uint8_t* status,
                           bool skip) {
  for (int j = 0; j < 32; ++j) enc_out[j] = 0;
  for (uint64_t j = 0; j < ct_cap; ++j) ct[j] = 0;
  if (!skip) *status = ST_HPKE_DECRYPT;
}

// One report, one lane: derive (key, base_nonce) from the lane's enc and dh (8 little-endian words
// each, as k_x25519_eph wrote them), then AEAD-encrypt pt under aad with sequence number 0: enc_out
// gets the 32 bytes of enc, ct gets pt.len() + 16 bytes (ciphertext || tag) and zeros up to
// ct_cap -- or everything zeros and status 4 when the DH value is all zero (pkR of small order,
// RFC 9180 §7.1.4).  pt and aad are byte sources (len(), block(o, d)).  sbox is unused (null) for
// ChaCha20-Poly1305.
template <int KDF, int AEAD, class Pt, class Aad>
DEVI void hpke_seal_lane(const uint8_t* sbox, const HpkeBatchConsts& bc, const uint32_t* enc,
                         const uint32_t* dh, const Pt& pt, const Aad& aad, uint8_t* enc_out,
                         uint8_t* ct, uint64_t ct_cap, uint8_t* status) {
  uint32_t dhw[8], encw[8], ence[8], nz = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t d = dh[i];
    nz |= d;
    dhw[i] = bswap32(d);
    ence[i] = enc[i];
    encw[i] = bswap32(ence[i]);
  }
  if (nz == 0u) {
    hpke_seal_reject(enc_out, ct, ct_cap, status, false);
    return;
  }
  constexpr int NKW = hpke_aead_nk(AEAD) / 4;
  uint32_t key[NKW], nonce[3];
  hpke_key_nonce<KDF, AEAD>(bc, dhw, encw, key, nonce);
  store_block(enc_out, 16, ence);
  store_block(enc_out + 16, 16, ence + 4);
  const uint64_t plen = pt.len();
  if constexpr (AEAD == 3) {
#pragma unroll
    for (int i = 0; i < NKW; ++i) key[i] = bswap32(key[i]);
#pragma unroll
    for (int i = 0; i < 3; ++i) nonce[i] = bswap32(nonce[i]);
    chacha20poly1305_seal(key, nonce, aad, pt, ct);
  } else {
    uint32_t rk[4 * (NKW + 7)];
    aes_expand<NKW>(sbox, key, rk);
    const uint32_t zero[4] = {0, 0, 0, 0};
    uint32_t hle[4], h[4], ctr[4], ek[4];
    aes_encrypt<NKW>(sbox, rk, zero, hle);  // H = E(K, 0)
#pragma unroll
    for (int i = 0; i < 4; ++i) h[i] = bswap32(hle[i]);
    uint32_t y[4] = {0, 0, 0, 0};
    ghash_bytes(y, h, aad);
#pragma unroll
    for (int i = 0; i < 3; ++i) ctr[i] = bswap32(nonce[i]);
    for (uint64_t o = 0; o < plen; o += 16) {  // CTR from counter 2; GHASH of what was stored
      uint32_t d[4], x[4];
      pt.block(o, d);
      ctr[3] = bswap32((uint32_t)(o >> 4) + 2u);
      aes_encrypt<NKW>(sbox, rk, ctr, ek);
#pragma unroll
      for (int i = 0; i < 4; ++i) d[i] ^= ek[i];
      mask_block(d, plen - o);
      store_block(ct + o, plen - o, d);
#pragma unroll
      for (int i = 0; i < 4; ++i) x[i] = bswap32(d[i]);
      ghash_step(y, x, h);
    }
    const uint64_t abits = aad.len() * 8, cbits = plen * 8;
    const uint32_t lens[4] = {(uint32_t)(abits >> 32), (uint32_t)abits, (uint32_t)(cbits >> 32),
                              (uint32_t)cbits};
    ghash_step(y, lens, h);
    ctr[3] = bswap32(1u);  // J0 = nonce || 1 (seq 0: the nonce is base_nonce)
    aes_encrypt<NKW>(sbox, rk, ctr, ek);
    uint32_t tag[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) tag[i] = bswap32(y[i]) ^ ek[i];
    store_block(ct + plen, 16, tag);
  }
  for (uint64_t j = plen + 16; j < ct_cap; ++j) ct[j] = 0;
}

// One lane per report: hpke_seal_lane over packed plaintexts and AADs; report r's ciphertext ||
// tag goes to cts[ct_off[r] .. ct_off[r + 1]) and its enc to encs[32 r ..].  A slot shorter than
// the plaintext + 16 or offsets that do not fit: zeros and status 4.  A report whose status is
// non-zero on entry keeps it and gets zeros.  `eph` is k_x25519_eph's output (n encs, then n DH
// values).  Lanes have their own lengths; the only barrier is the one after the S-box is built,
// before any lane diverges (no S-box for ChaCha20-Poly1305).
template <int KDF, int AEAD>
__global__ void __launch_bounds__(256) k_hpke_seal(
    uint32_t n, HpkeBatchConsts bc, const uint32_t* eph, const uint8_t* aads,
    const uint64_t* aad_off, uint64_t aad_total, const uint8_t* pts, const uint64_t* pt_off,
    uint64_t pt_total, uint8_t* encs, uint8_t* cts, const uint64_t* ct_off, uint64_t ct_total,
    uint8_t* status) {
  const uint8_t* sbox = nullptr;
  if constexpr (AEAD != 3) {
    __shared__ uint8_t sbox_lds[256];
    aes_sbox_init(sbox_lds);
    __syncthreads();
    sbox = sbox_lds;
  }
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const uint64_t a0 = aad_off[r], a1 = aad_off[r + 1], p0 = pt_off[r], p1 = pt_off[r + 1];
  const uint64_t c0 = ct_off[r], c1 = ct_off[r + 1];
  const bool ct_fits = c0 <= c1 && c1 <= ct_total;
  const uint64_t ct_cap = ct_fits ? c1 - c0 : 0;
  uint8_t* ct = cts + (ct_fits ? c0 : 0);
  uint8_t* enc_out = encs + (size_t)r * 32;
  const bool skip = status[r] != 0;
  const bool ok = !skip && ct_fits && a0 <= a1 && a1 <= aad_total && p0 <= p1 && p1 <= pt_total &&
                  ct_cap >= 16 && p1 - p0 <= ct_cap - 16;
  if (!ok) {  // nothing to read: skip the work, not just the result
    hpke_seal_reject(enc_out, ct, ct_cap, status + r, skip);
    return;
  }
  hpke_seal_lane<KDF, AEAD>(sbox, bc, eph + (size_t)r * 8, eph + ((size_t)n + r) * 8,
                            PackedBytes{pts + p0, p1 - p0}, PackedBytes{aads + a0, a1 - a0},
                            enc_out, ct, ct_cap, status + r);
}

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
};

// One lane per report: hpke_seal_lane over the rows of a batch of Prio3 input shares to one
// aggregator.  Report r's plaintext is the PlaintextInputShare of shares[r spitch ..] (slen bytes),
// its AAD the InputShareAad of (tid, rids[16 r ..], times[r], pubs[r pslen ..]); neither frame
// exists in memory.  Its enc goes to encs[r enc_pitch ..] (32 bytes) and its payload, exactly
// 6 + slen + 16 bytes, to payloads[r ppitch ..]; nothing else of either buffer is written.
template <int KDF, int AEAD>
__global__ void __launch_bounds__(256) k_hpke_seal_shares(
    uint32_t n, HpkeBatchConsts bc, ReqTaskId tid, const uint32_t* eph, const uint8_t* rids,
    const uint64_t* times, const uint8_t* pubs, uint32_t pslen, const uint8_t* shares,
    uint32_t slen, uint64_t spitch, uint8_t* encs, uint64_t enc_pitch, uint8_t* payloads,
    uint64_t ppitch, uint8_t* status) {
  const uint8_t* sbox = nullptr;
  if constexpr (AEAD != 3) {
    __shared__ uint8_t sbox_lds[256];
    aes_sbox_init(sbox_lds);
    __syncthreads();
    sbox = sbox_lds;
  }
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  uint8_t* enc_out = encs + (uint64_t)r * enc_pitch;
  uint8_t* ct = payloads + (uint64_t)r * ppitch;
  const uint64_t ct_cap = 6 + (uint64_t)slen + 16;
  if (status[r] != 0) {
    hpke_seal_reject(enc_out, ct, ct_cap, status + r, true);
    return;
  }
  const ReqAad aad{tid, rids + (size_t)r * 16, times[r], pslen, pubs + (size_t)r * pslen};
  hpke_seal_lane<KDF, AEAD>(sbox, bc, eph + (size_t)r * 8, eph + ((size_t)n + r) * 8,
                            SharePlaintext{shares + (uint64_t)r * spitch, slen}, aad, enc_out, ct,
                            ct_cap, status + r);
}

}  // namespace p3g
