// What the host half (hpke.cpp) and the GPU half (hpke_gpu.h, engine_hpke.hip) of the batched HPKE
// open share: the values one batch of opens under ONE keypair has in common, computed once on the
// host.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace p3g {

// DHKEM(X25519, HKDF-SHA256) with KDF kdf_id (1 HKDF-SHA256, 2 -SHA384, 3 -SHA512) and AEAD
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
};

// hpke.cpp.  false if the suite is not an X25519 suite above or its primitives are unavailable.
bool hpke_batch_consts(uint16_t kdf_id, uint16_t aead_id, const uint8_t* pk, const uint8_t* info,
                       size_t info_len, HpkeBatchConsts* out);

}  // namespace p3g
