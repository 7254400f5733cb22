// The launches of hpke_gpu.h's, helper_request.h's, hpke_open_team.h's and hpke_seal_team.h's
// kernels: the lane-per-report open, the request path's kernels, the wave-per-report open and
// seal, and the Poly1305 test kernel (hpke_launch.h).  They share one unit because the compiler
// schedules the ChaCha20-Poly1305 instantiations of these families by whether k_test_poly1305 is
// in their module: apart from it, the packed wave-per-report kernels or the lane open's come out
// in another instruction order ("Kernel-family units").
#include <hip/hip_runtime.h>

#include "hpke_launch.h"
#include "plan_hpke.h"
#include "hpke_gpu.h"
#include "helper_request.h"
#include "hpke_open_team.h"
#include "hpke_seal_team.h"

namespace p3g::eng {

int launch_hpke_open(prio3gpu_ctx* c, const PackedOpenCall& q) {
  {
    PROF(KID_HPKE_OPEN);
    hpke_suite_dispatch(q.bc, [&](auto kdf, auto aead) {
      hipLaunchKernelGGL((k_hpke_open<decltype(kdf)::value, decltype(aead)::value>),
                         grid1(q.n, 256), dim3(256), 0, c->stream, q.n, q.bc, q.dh, q.encs,
                         q.aads, q.aad_off, q.aad_total, q.cts, q.ct_off, q.ct_total, q.pts,
                         q.pt_off, q.pt_total, q.status);
    });
  }
  HIPCHK(hipGetLastError());
  return 0;
}

int launch_req_gather(prio3gpu_ctx* c, size_t n, const uint8_t* d_msg, size_t msg_len,
                      const ReqView* d_views, uint8_t* d_nonces, uint8_t* d_pub, uint8_t* d_lps,
                      uint8_t* d_faults) {
  const Cfg& g = c->cfg;
  {
    PROF(KID_REQ_GATHER);
    hipLaunchKernelGGL(k_req_gather, dim3((unsigned)req_gather_blocks(g, n), 3), dim3(256), 0,
                       c->stream, (uint32_t)n, d_msg, (uint64_t)msg_len, d_views,
                       g.public_share_len, g.prep_share_len, d_nonces, d_pub, d_lps, d_faults);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

int launch_hpke_open_req(prio3gpu_ctx* c, const HpkeBatchConsts& bc, const ReqTaskId& tid,
                         size_t m, const uint32_t* d_idx, const uint32_t* d_dh,
                         const uint8_t* d_msg, const ReqView* d_views, uint8_t* d_pts,
                         const uint64_t* d_poff, uint8_t* d_status) {
  {
    PROF(KID_HPKE_OPEN_REQ);
    hpke_suite_dispatch(bc, [&](auto kdf, auto aead) {
      hipLaunchKernelGGL((k_hpke_open_req<decltype(kdf)::value, decltype(aead)::value>),
                         dim3((unsigned)((m + 255) / 256)), dim3(256), 0, c->stream, (uint32_t)m,
                         bc, tid, d_idx, d_dh, d_msg, d_views, d_pts, d_poff, d_status);
    });
  }
  HIPCHK(hipGetLastError());
  return 0;
}

int launch_decode_plaintext_input_shares(prio3gpu_ctx* c, size_t n, const uint8_t* d_pts,
                                         const uint64_t* d_poff, uint32_t want, uint8_t* d_rows,
                                         uint64_t pitch, const uint8_t* d_faults,
                                         uint8_t* d_status) {
  {
    PROF(KID_DECODE_PT);
    hipLaunchKernelGGL(k_decode_plaintext_input_shares, grid1(n, 256), dim3(256), 0, c->stream,
                       (uint32_t)n, d_pts, d_poff, want, d_rows, pitch, d_faults, d_status);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

int launch_req_scatter(prio3gpu_ctx* c, size_t k, const uint32_t* d_idx, const uint8_t* d_crows,
                       const uint8_t* d_sts, uint32_t want, uint8_t* d_rows, uint64_t pitch,
                       const uint8_t* d_faults, uint8_t* d_status) {
  {
    PROF(KID_REQ_SCATTER);
    hipLaunchKernelGGL(k_req_scatter, grid1(k, 256), dim3(256), 0, c->stream, (uint32_t)k, d_idx,
                       d_crows, d_sts, want, d_rows, pitch, d_faults, d_status);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

int launch_hpke_open_team(prio3gpu_ctx* c, const PackedOpenCall& q) {
  {
    PROF(KID_HPKE_OPEN_TEAM);
    hpke_suite_dispatch(q.bc, [&](auto kdf, auto aead) {
      hipLaunchKernelGGL((k_hpke_open_team<decltype(kdf)::value, decltype(aead)::value>),
                         grid1(q.n, kTeamsPerBlock), dim3(256), 0, c->stream, q.n, q.bc, q.dh,
                         q.encs, q.aads, q.aad_off, q.aad_total, q.cts, q.ct_off, q.ct_total,
                         q.pts, q.pt_off, q.pt_total, q.status);
    });
  }
  HIPCHK(hipGetLastError());
  return 0;
}

int launch_hpke_open_team_shares(prio3gpu_ctx* c, const ShareOpenCall& q) {
  {
    PROF(KID_HPKE_OPEN_TEAM_SHARES);
    hpke_suite_dispatch(q.bc, [&](auto kdf, auto aead) {
      hipLaunchKernelGGL((k_hpke_open_team_shares<decltype(kdf)::value, decltype(aead)::value>),
                         grid1(q.n, kTeamsPerBlock), dim3(256), 0, c->stream, q.n, q.bc, q.tid,
                         q.dh, q.rids, q.times, q.pubs, q.pslen, q.encs, q.enc_pitch, q.payloads,
                         q.ppitch, q.slen, q.out, q.spitch, q.status);
    });
  }
  HIPCHK(hipGetLastError());
  return 0;
}

int launch_hpke_seal_team(prio3gpu_ctx* c, const PackedSealCall& q) {
  {
    PROF(KID_HPKE_SEAL_TEAM);
    hpke_suite_dispatch(q.bc, [&](auto kdf, auto aead) {
      hipLaunchKernelGGL((k_hpke_seal_team<decltype(kdf)::value, decltype(aead)::value>),
                         grid1(q.n, kTeamsPerBlock), dim3(256), 0, c->stream, q.n, q.bc, q.eph,
                         q.aads, q.aad_off, q.aad_total, q.pts, q.pt_off, q.pt_total, q.encs,
                         q.cts, q.ct_off, q.ct_total, q.status);
    });
  }
  HIPCHK(hipGetLastError());
  return 0;
}

int launch_hpke_seal_team_shares(prio3gpu_ctx* c, const ShareSealCall& q) {
  {
    PROF(KID_HPKE_SEAL_TEAM_SHARES);
    hpke_suite_dispatch(q.bc, [&](auto kdf, auto aead) {
      hipLaunchKernelGGL((k_hpke_seal_team_shares<decltype(kdf)::value, decltype(aead)::value>),
                         grid1(q.n, kTeamsPerBlock), dim3(256), 0, c->stream, q.n, q.bc, q.tid,
                         q.eph, q.rids, q.times, q.pubs, q.pslen, q.shares, q.slen, q.spitch,
                         q.encs, q.enc_pitch, q.payloads, q.ppitch, q.status);
    });
  }
  HIPCHK(hipGetLastError());
  return 0;
}

int launch_test_poly1305(prio3gpu_ctx* c, size_t n, const uint8_t* d_keys, const uint8_t* d_msgs,
                         const uint64_t* d_off, uint8_t* d_tags) {
  hipLaunchKernelGGL(k_test_poly1305, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c->stream,
                     (uint32_t)n, d_keys, d_msgs, d_off, d_tags);
  HIPCHK(hipGetLastError());
  return 0;
}

}  // namespace p3g::eng
