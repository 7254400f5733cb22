// What the host planner and the kernels agree on: the VDAF kind, status and usage codes, the XOF
// selector and Cfg, the by-value kernel argument that describes one VDAF instance.  No HIP here:
// plan_cfg.h fills a Cfg on any host (tests/test_host_plan.py builds it with g++), and
// prio3_kernels.h / keccak.h include this file for the device.  Cfg's member order, types and
// padding are the kernels' argument layout.
#pragma once
#include <stdint.h>

// The XOF of a context: XofShake128 (Keccak-f[1600] = 24 rounds, SHAKE padding byte 0x1F; prio
// 0.15.1 / VDAF-07, Janus 0.6) or XofTurboShake128 (Keccak-p[1600, 12], domain byte 0x01;
// draft-irtf-cfrg-vdaf-08+).  Both absorb the same message u8(len(dst)) || dst || seed || binder.
struct Xof {
  uint32_t full;  // 1: 24 rounds (SHAKE128), 0: 12 rounds (TurboSHAKE128)
  uint32_t pad;   // first padding byte: 0x1F (SHAKE128) or the TurboSHAKE domain byte 0x01
};
constexpr Xof kXofShake128{1u, 0x1Fu};
constexpr Xof kXofTurboShake128{0u, 0x01u};

namespace p3g {

enum Kind : uint32_t {
  KIND_COUNT = 0,
  KIND_SUM = 1,
  KIND_SUMVEC = 2,
  KIND_HISTOGRAM = 3,
  KIND_FPVEC = 4  // FixedPointBoundedL2VecSum (bits = 16/32/64 per entry, length = entries)
};

// Per-report status codes = DAP PrepareError (messages/src/lib.rs:2288-2298) + 0 = ok.
enum Status : uint8_t { ST_OK = 0, ST_VDAF_PREP_ERROR = 5, ST_INVALID_MESSAGE = 8, ST_SKIPPED = 0xFF };

enum Usage : uint32_t {
  DST_MEASUREMENT_SHARE = 1,
  DST_PROOF_SHARE = 2,
  DST_JOINT_RANDOMNESS = 3,
  DST_PROVE_RANDOMNESS = 4,
  DST_QUERY_RANDOMNESS = 5,
  DST_JOINT_RAND_SEED = 6,
  DST_JOINT_RAND_PART = 7,
};

struct Cfg {
  uint32_t kind, algo_id, es;
  uint32_t meas_len, proof_len, verifier_len, jr_len, out_len, prove_rand_len;
  uint32_t bits, length, chunk, calls, m, logm, arity, gp_len;
  uint32_t leader_share_len, helper_share_len, public_share_len, prep_share_len, prep_msg_len;
  uint32_t qr_len;          // query-randomness elements (one per gadget)
  uint32_t exact_squeeze;   // test switch: every XOF squeeze takes the per-element path
  // engine option wave_prio: FixedPoint chain waves issue at s_setprio 3 and its matrix-core wire
  // passes at 2, over whatever co-runs on their SIMDs (the other aggregator's query, k_fpv_regen)
  uint32_t wave_prio;
  Xof xof;                  // XofShake128 (default) or XofTurboShake128
  const uint8_t* twiddles;  // device: alpha_m^k, k < m, Montgomery form, ES bytes each
  // FixedPointBoundedL2VecSum's second gadget, ParallelSum(PolyEval(norm poly), chunk1)
  uint32_t chunk1, calls1, m1, logm1, gp_len1;
  const uint8_t* twiddles1;  // same table layout as `twiddles`, for m1 / calls1
};

}  // namespace p3g
