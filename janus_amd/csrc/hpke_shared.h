// What the host half (hpke.cpp) and the GPU half (hpke_gpu.h, engine.hip) of the batched HPKE open
// share: the values one batch of opens under ONE keypair has in common, computed once on the host.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace p3g {

// DHKEM(X25519, HKDF-SHA256) / HKDF-SHA256 / AES-128-GCM, base mode.  Every field is eight
// big-endian 32-bit words (the form SHA-256 consumes and produces).
struct HpkeBatchConsts {
  uint32_t pk[8];           // pkR, the recipient public key (kem_context = enc || pkR)
  uint32_t psk_id_hash[8];  // LabeledExtract("", "psk_id_hash", "")
  uint32_t info_hash[8];    // LabeledExtract("", "info_hash", info)
  uint32_t salt0_i[8];      // HMAC-SHA256 under the empty salt: state after the ipad block ...
  uint32_t salt0_o[8];      // ... and after the opad block (LabeledExtract("", "eae_prk", dh))
};

// hpke.cpp.  false if the suite's primitives are unavailable.
bool hpke_batch_consts(const uint8_t* pk, const uint8_t* info, size_t info_len,
                       HpkeBatchConsts* out);

}  // namespace p3g
