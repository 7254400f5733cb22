// What engine_hpke.hip asks of the HPKE kernel units: every launch of the GPU HPKE paths, host
// side only.  Each kernel header is one unit's alone, so the units compile side by side:
//   engine_hpke_dh.hip          hpke_dh_gpu.h                  the ladders
//   engine_hpke_seal.hip        hpke_seal_gpu.h                a lane per report
//   engine_hpke_team.hip        hpke_gpu.h, helper_request.h, hpke_open_team.h, hpke_seal_team.h
//                               the lane open, the request path, a wave per report, the test hook
//   engine_hpke_split.hip       hpke_team_split.h              several waves per report
// A launch function sets the kernel's profiling scope, picks the instantiation of the call's
// suite, queues the kernel on the context's stream and returns the launch's error.  It checks
// nothing, stages nothing and owns no secret: those are engine_hpke.hip's.  No kernel header is
// included here.
#pragma once
#include <string.h>

#include <type_traits>

#include "engine_internal.h"
#include "hpke_kernel_args.h"
#include "hpke_lane.h"
#include "hpke_shared.h"

namespace p3g::eng {

inline void wipe(void* p, size_t n) {  // a memset the compiler may not drop
  memset(p, 0, n);
  __asm__ __volatile__("" : : "r"(p) : "memory");
}

// f(KDF, AEAD) with the suite of bc as compile-time constants (one kernel instantiation each of
// the nine pairs; the entry points have checked the suite, so no other value arrives).
template <class F>
void hpke_suite_dispatch(const HpkeBatchConsts& bc, F&& f) {
  auto with_aead = [&](auto kdf) {
    if (bc.aead_id == 1) f(kdf, std::integral_constant<int, 1>{});
    else if (bc.aead_id == 2) f(kdf, std::integral_constant<int, 2>{});
    else f(kdf, std::integral_constant<int, 3>{});
  };
  if (bc.kdf_id == 1) with_aead(std::integral_constant<int, 1>{});
  else if (bc.kdf_id == 2) with_aead(std::integral_constant<int, 2>{});
  else with_aead(std::integral_constant<int, 3>{});
}

// ---- the ladders (engine_hpke_dh.hip) -----------------------------------------------------------
// A recipient's private key sk travels as a kernel argument, so no device buffer ever holds it,
// and its host copy in the argument's form is wiped after the launch.

// The generator, as SerializePublicKey writes it
inline constexpr uint8_t kP256G[65] = {
    0x04, 0x6b, 0x17, 0xd1, 0xf2, 0xe1, 0x2c, 0x42, 0x47, 0xf8, 0xbc, 0xe6, 0xe5, 0x63, 0xa4,
    0x40, 0xf2, 0x77, 0x03, 0x7d, 0x81, 0x2d, 0xeb, 0x33, 0xa0, 0xf4, 0xa1, 0x39, 0x45, 0xd8,
    0x98, 0xc2, 0x96, 0x4f, 0xe3, 0x42, 0xe2, 0xfe, 0x1a, 0x7f, 0x9b, 0x8e, 0xe7, 0xeb, 0x4a,
    0x7c, 0x0f, 0x9e, 0x16, 0x2b, 0xce, 0x33, 0x57, 0x6b, 0x31, 0x5e, 0xce, 0xcb, 0xb6, 0x40,
    0x68, 0x37, 0xbf, 0x51, 0xf5};

// d_out[r] = X25519(sk, d_points[r]) for r < n.
int launch_x25519(prio3gpu_ctx* c, const uint8_t* sk, size_t n, const uint8_t* d_points,
                  uint32_t* d_out);

// The same over a key group of the request in device memory: d_dh[idx[j]] for j < m.
int launch_x25519_idx(prio3gpu_ctx* c, const uint8_t* sk, size_t m, const uint32_t* d_idx,
                      const uint8_t* d_msg, const ReqView* d_views, uint32_t* d_dh);

// d_out[r] = the shared_secret (raw: x([sk] point)) and d_ok[r] for the n packed 65-byte points.
// pk is pkRm, and bc holds the empty salt's pad states; the keypair has passed
// p256_keypair_valid.
int launch_p256_dh(prio3gpu_ctx* c, const uint8_t* sk, const uint8_t* pk,
                   const HpkeBatchConsts& bc, bool raw, size_t n, const uint8_t* d_points,
                   uint32_t* d_out, uint8_t* d_ok);

// The same over a key group of the request in device memory.
int launch_p256_dh_idx(prio3gpu_ctx* c, const uint8_t* sk, const uint8_t* pk,
                       const HpkeBatchConsts& bc, size_t m, const uint32_t* d_idx,
                       const uint8_t* d_msg, const ReqView* d_views, uint32_t* d_ss,
                       uint8_t* d_ok);

// k_x25519_eph over n staged ephemeral scalars to the recipient pk: n encapsulated keys, then n
// DH values, 32 bytes each, at d_eph.
int launch_x25519_eph(prio3gpu_ctx* c, const uint8_t* pk, size_t n, const uint8_t* d_sk,
                      uint32_t* d_eph);

// k_p256_eph over n staged ephemeral scalars to the recipient pk (a point: the entry points have
// checked it): the points, the raw DH values and the validity bytes d_ok, in kP256EphBytes' layout
// at d_eph.
int launch_p256_eph(prio3gpu_ctx* c, const uint8_t* pk, size_t n, const uint8_t* d_sk,
                    uint32_t* d_eph, uint8_t* d_ok);

// k_p256_eph_kem after it: the DH values at d_eph become the shared secrets.
int launch_p256_eph_kem(prio3gpu_ctx* c, const uint8_t* pk, const HpkeBatchConsts& bc, size_t n,
                        uint32_t* d_eph, const uint8_t* d_ok);

// ---- a lane per report, a wave per report -------------------------------------------------------
// One struct per argument list a lane kernel and its wave-per-report counterpart share; the
// fields are the kernels' arguments, in their order.  A lane launch puts 256 reports in a block, a
// wave launch kTeamsPerBlock.

struct PackedOpenCall {  // k_hpke_open, k_hpke_open_team
  uint32_t n;
  HpkeBatchConsts bc;
  const uint32_t* dh;
  const uint8_t *encs, *aads;
  const uint64_t* aad_off;
  uint64_t aad_total;
  const uint8_t* cts;
  const uint64_t* ct_off;
  uint64_t ct_total;
  uint8_t* pts;
  const uint64_t* pt_off;
  uint64_t pt_total;
  uint8_t* status;
};
int launch_hpke_open(prio3gpu_ctx* c, const PackedOpenCall& q);       // engine_hpke_team.hip
int launch_hpke_open_team(prio3gpu_ctx* c, const PackedOpenCall& q);  // engine_hpke_team.hip

struct PackedSealCall {  // k_hpke_seal, k_hpke_seal_team
  uint32_t n;
  HpkeBatchConsts bc;
  const uint32_t* eph;
  const uint8_t* aads;
  const uint64_t* aad_off;
  uint64_t aad_total;
  const uint8_t* pts;
  const uint64_t* pt_off;
  uint64_t pt_total;
  uint8_t *encs, *cts;
  const uint64_t* ct_off;
  uint64_t ct_total;
  uint8_t* status;
};
int launch_hpke_seal(prio3gpu_ctx* c, const PackedSealCall& q);       // engine_hpke_seal.hip
int launch_hpke_seal_team(prio3gpu_ctx* c, const PackedSealCall& q);  // engine_hpke_team.hip

struct ShareSealCall {  // k_hpke_seal_shares, k_hpke_seal_team_shares
  uint32_t n;
  HpkeBatchConsts bc;
  ReqTaskId tid;
  const uint32_t* eph;
  const uint8_t* rids;
  const uint64_t* times;
  const uint8_t* pubs;
  uint32_t pslen;
  const uint8_t* shares;
  uint32_t slen;
  uint64_t spitch;
  uint8_t* encs;
  uint64_t enc_pitch;
  uint8_t* payloads;
  uint64_t ppitch;
  uint8_t* status;
};
int launch_hpke_seal_shares(prio3gpu_ctx* c, const ShareSealCall& q);       // ..._seal.hip
int launch_hpke_seal_team_shares(prio3gpu_ctx* c, const ShareSealCall& q);  // ..._team.hip

struct ShareOpenCall {  // k_hpke_open_team_shares
  uint32_t n;
  HpkeBatchConsts bc;
  ReqTaskId tid;
  const uint32_t* dh;
  const uint8_t* rids;
  const uint64_t* times;
  const uint8_t* pubs;
  uint32_t pslen;
  const uint8_t* encs;
  uint64_t enc_pitch;
  const uint8_t* payloads;
  uint64_t ppitch;
  uint32_t slen;
  uint8_t* out;
  uint64_t spitch;
  uint8_t* status;
};
int launch_hpke_open_team_shares(prio3gpu_ctx* c, const ShareOpenCall& q);  // ..._team.hip

// ---- several waves per report (engine_hpke_split.hip) -------------------------------------------
// What the kernels of one split share-row call have in common: n reports cut into S >= 2 segments
// of L blocks (plan_hpke.h's team_split_plan), the suite's constants, the InputShareAad's parts,
// the share length, and the call's scratch (split_scratch_bytes: n S segment sums, then n header
// flags), which is key-derived and the caller's to clear.
struct SplitShareCall {
  uint32_t n, S;
  uint64_t L;
  HpkeBatchConsts bc;
  ReqTaskId tid;
  const uint8_t* rids;
  const uint64_t* times;
  const uint8_t* pubs;
  uint32_t pslen, slen;
  uint8_t* scratch;
  uint8_t* status;
};

size_t split_scratch_bytes(size_t n, uint32_t S);

// The waves per SIMD the segment kernels of an AEAD run at (their resource remarks): with the
// device's compute units, the wave slots team_split_plan fills.
uint32_t split_waves_per_simd(uint32_t aead_id);

// k_hpke_open_team_split, k_hpke_open_team_join and k_hpke_team_wipe, queued back to back on the
// context's stream: prio3gpu_open_input_shares' columns (k_hpke_open_team_shares' arguments).  If
// a launch fails, the rows are zeroed whole before the error returns: in no case does
// unauthenticated plaintext stay in `out` once the stream has run what this call queued.
int launch_open_team_split(prio3gpu_ctx* c, const SplitShareCall& q, const uint32_t* dh,
                           const uint8_t* encs, uint64_t enc_pitch, const uint8_t* payloads,
                           uint64_t ppitch, uint8_t* out, uint64_t spitch);

// k_hpke_seal_team_split and k_hpke_seal_team_join: prio3gpu_seal_input_shares_long's columns
// (k_hpke_seal_team_shares' arguments).
int launch_seal_team_split(prio3gpu_ctx* c, const SplitShareCall& q, const uint32_t* eph,
                           const uint8_t* shares, uint64_t spitch, uint8_t* encs,
                           uint64_t enc_pitch, uint8_t* payloads, uint64_t ppitch);

// ---- the request path (engine_hpke_team.hip) ----------------------------------------------------
// k_req_gather over n checked views: rows of 16 / public_share_len / prep_share_len bytes.
int launch_req_gather(prio3gpu_ctx* c, size_t n, const uint8_t* d_msg, size_t msg_len,
                      const ReqView* d_views, uint8_t* d_nonces, uint8_t* d_pub, uint8_t* d_lps,
                      uint8_t* d_faults);

// k_hpke_open_req over one key group, instantiated for the suite of bc.
int launch_hpke_open_req(prio3gpu_ctx* c, const HpkeBatchConsts& bc, const ReqTaskId& tid,
                         size_t m, const uint32_t* d_idx, const uint32_t* d_dh,
                         const uint8_t* d_msg, const ReqView* d_views, uint8_t* d_pts,
                         const uint64_t* d_poff, uint8_t* d_status);

// k_decode_plaintext_input_shares over n reports: rows of `want` bytes, `pitch` apart.
int launch_decode_plaintext_input_shares(prio3gpu_ctx* c, size_t n, const uint8_t* d_pts,
                                         const uint64_t* d_poff, uint32_t want, uint8_t* d_rows,
                                         uint64_t pitch, const uint8_t* d_faults,
                                         uint8_t* d_status);

// k_req_scatter over the k reports the host opened.
int launch_req_scatter(prio3gpu_ctx* c, size_t k, const uint32_t* d_idx, const uint8_t* d_crows,
                       const uint8_t* d_sts, uint32_t want, uint8_t* d_rows, uint64_t pitch,
                       const uint8_t* d_faults, uint8_t* d_status);

// ---- the test hook (engine_hpke_team.hip) -------------------------------------------------------
// k_test_poly1305 over n messages (prio3gpu_test_poly1305_gpu).
int launch_test_poly1305(prio3gpu_ctx* c, size_t n, const uint8_t* d_keys, const uint8_t* d_msgs,
                         const uint64_t* d_off, uint8_t* d_tags);

}  // namespace p3g::eng
