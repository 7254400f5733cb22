// The plain structs the DH and request kernels take as arguments, and the layout of the P-256
// seal ladders' output: what the kernel headers (hpke_dh_gpu.h, helper_request.h) and the host
// (hpke_launch.h, engine_hpke.hip) both name.  No HIP and no kernel.  Included after
// include/prio3gpu.h.
#pragma once
#include "p256_kem.h"
#include "x25519.h"

namespace p3g {

using ReqView = prio3gpu_prepare_init_view;

// The batch-shared inputs of the P-256 DH kernels: pkRm's coordinates and the HMAC-SHA256 pad
// states of the empty salt (the KEM half runs in the DH kernel).
struct P256DhConsts {
  P256PublicKey pk;
  uint32_t salt0_i[8], salt0_o[8];
};

struct X25519Point {  // a u coordinate as little-endian words; a kernel argument
  uint32_t w[8];
};

// The ladders' output for n reports under P-256, as the seal kernels read it (bc.dh_ok set), in
// bytes: [0, 64 n) the ephemeral points' x || y, 64 per report; [64 n, 96 n) the DH values' x, after
// k_p256_eph_kem the shared secrets; [96 n, 97 n) one validity byte per report (bc.dh_ok).
constexpr size_t kP256EphBytes = 97;

struct P256EphPoints {  // G ([0]) and pkR ([1]) in Montgomery coordinates; a kernel argument
  Fp256 X[2], Y[2];
};

}  // namespace p3g
