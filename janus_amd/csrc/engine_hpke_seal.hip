// The launches of hpke_seal_gpu.h's kernels: the lane-per-report seal over packed inputs and over
// Prio3 input-share rows (hpke_launch.h).
#include <hip/hip_runtime.h>

#include "hpke_launch.h"
#include "hpke_seal_gpu.h"

namespace p3g::eng {

int launch_hpke_seal(prio3gpu_ctx* c, const PackedSealCall& q) {
  {
    PROF(KID_HPKE_SEAL);
    hpke_suite_dispatch(q.bc, [&](auto kdf, auto aead) {
      hipLaunchKernelGGL((k_hpke_seal<decltype(kdf)::value, decltype(aead)::value>),
                         grid1(q.n, 256), dim3(256), 0, c->stream, q.n, q.bc, q.eph, q.aads,
                         q.aad_off, q.aad_total, q.pts, q.pt_off, q.pt_total, q.encs, q.cts,
                         q.ct_off, q.ct_total, q.status);
    });
  }
  HIPCHK(hipGetLastError());
  return 0;
}

int launch_hpke_seal_shares(prio3gpu_ctx* c, const ShareSealCall& q) {
  {
    PROF(KID_HPKE_SEAL_SHARES);
    hpke_suite_dispatch(q.bc, [&](auto kdf, auto aead) {
      hipLaunchKernelGGL((k_hpke_seal_shares<decltype(kdf)::value, decltype(aead)::value>),
                         grid1(q.n, 256), dim3(256), 0, c->stream, q.n, q.bc, q.tid, q.eph,
                         q.rids, q.times, q.pubs, q.pslen, q.shares, q.slen, q.spitch, q.encs,
                         q.enc_pitch, q.payloads, q.ppitch, q.status);
    });
  }
  HIPCHK(hipGetLastError());
  return 0;
}

}  // namespace p3g::eng
