// What the host half (hpke.cpp) and the GPU half (hpke_lane.h, engine_hpke.hip) of the batched HPKE
// open share: the values one batch of opens under ONE keypair has in common, computed once on the
// host.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace p3g {

// DHKEM(X25519, HKDF-SHA256) (KEM 0x0020) or DHKEM(P-256, HKDF-SHA256) (0x0010) with KDF kdf_id (1 HKDF-SHA256, 2 -SHA384, 3 -SHA512) and AEAD
// aead_id (1 AES-128-GCM, 2 AES-256-GCM, 3 ChaCha20-Poly1305), base mode.  Every field is
// big-endian 32-bit words (the form SHA-256 consumes and produces; SHA-512 pairs them); the two
// hashes are Nh = 32 / 48 / 64 bytes of the suite's KDF, the rest zero.
struct HpkeBatchConsts {
  uint32_t kdf_id, aead_id;  // the suite (a launch's kernel is instantiated for it)
  uint32_t pk[8];            // pkR, the recipient public key (kem_context = enc || pkR)
  uint32_t psk_id_hash[16];  // LabeledExtract("", "psk_id_hash", "")
  uint32_t info_hash[16];    // LabeledExtract("", "info_hash", info)
  uint32_t salt0_i[8];       // HMAC-SHA256 under the empty salt: state after the ipad block ...
  uint32_t salt0_o[8];       // ... and after the opad block (LabeledExtract("", "eae_prk", dh))
  uint32_t kem_lo;           // the KEM id's low byte in the suite ids: 0x20 / 0x10
  uint32_t nenc;             // bytes of an encapsulated key: 32 / 65
  // Where a report's DH validity comes from.  Null (X25519): the 8-word per-report buffer holds
  // the DH value, all zero is the failure, and the open kernel runs the KEM half with pk.
  // Non-null (P-256, where an all-zero x coordinate is a legal DH value): one flag byte per
  // report beside the buffer, which then holds the finished shared_secret (k_p256_dh has run
  // the KEM half; pk is unused).  Set by the engine once the buffer exists.
  const uint8_t* dh_ok;
};

// The wave-per-report kernels' geometry, which their launches' grids follow.
constexpr uint32_t kTeam = 64;          // lanes per report: one wave
constexpr uint32_t kTeamsPerBlock = 4;  // reports per 256-thread block

// hpke.cpp.  false if the suite is not one above or its primitives are unavailable.  pk is pkR's
// 32 bytes for X25519 and is not read for P-256.
bool hpke_batch_consts(uint16_t kem_id, uint16_t kdf_id, uint16_t aead_id, const uint8_t* pk, const uint8_t* info,
                       size_t info_len, HpkeBatchConsts* out);

}  // namespace p3g
