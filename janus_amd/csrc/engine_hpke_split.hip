// The launches of hpke_team_split.h's kernels (several waves per report for the share-row HPKE
// open and seal, the context's "hpke_team_split" option), a unit of its own so that its thirty-six
// instantiations compile beside the other kernel units'.  engine_hpke.hip checks the call, stages
// its buffers, runs the DH and owns the secrets (CallSecrets); this unit only queues kernels on
// the context's stream (hpke_launch.h).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hpke_launch.h"
#include "hpke_team_split.h"

namespace p3g::eng {

namespace {

dim3 waves_grid(uint64_t waves) {
  return dim3((unsigned)((waves + kTeamsPerBlock - 1) / kTeamsPerBlock));
}

uint32_t* parts_of(const SplitShareCall& q) { return reinterpret_cast<uint32_t*>(q.scratch); }
uint8_t* flags_of(const SplitShareCall& q) {
  return q.scratch + (size_t)q.n * q.S * kSplitPartWords * sizeof(uint32_t);
}

}  // namespace

size_t split_scratch_bytes(size_t n, uint32_t S) {
  return n * S * kSplitPartWords * sizeof(uint32_t) + n;
}

// The segment kernels' occupancy (-Rpass-analysis=kernel-resource-usage):
// 185 to 216 VGPRs under AES-GCM, 118 to 123 under ChaCha20-Poly1305.
uint32_t split_waves_per_simd(uint32_t aead_id) { return aead_id == 3 ? 4u : 2u; }

int launch_open_team_split(prio3gpu_ctx* c, const SplitShareCall& q, const uint32_t* dh,
                           const uint8_t* encs, uint64_t enc_pitch, const uint8_t* payloads,
                           uint64_t ppitch, uint8_t* out, uint64_t spitch) {
  // the rows hold plaintext without a verdict from the first launch on: whatever fails after it,
  // they are zeroed whole before the error returns
  auto fail = [&](hipError_t e) {
    (void)hipMemset2DAsync(out, spitch, 0, q.slen, q.n, c->stream);
    set_err("a launch of the split open failed: %s", hipGetErrorString(e));
    return PRIO3GPU_E_HIP;
  };
  {
    PROF(KID_HPKE_OPEN_TEAM_SPLIT);
    hpke_suite_dispatch(q.bc, [&](auto kdf, auto aead) {
      hipLaunchKernelGGL((k_hpke_open_team_split<decltype(kdf)::value, decltype(aead)::value>),
                         waves_grid((uint64_t)q.n * q.S), dim3(256), 0, c->stream, q.n, q.S, q.L,
                         q.bc, q.tid, dh, q.rids, q.times, q.pubs, q.pslen, encs, enc_pitch,
                         payloads, ppitch, q.slen, out, spitch, q.status, parts_of(q),
                         flags_of(q));
    });
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(e);
  {
    PROF(KID_HPKE_OPEN_TEAM_JOIN);
    hpke_suite_dispatch(q.bc, [&](auto kdf, auto aead) {
      hipLaunchKernelGGL((k_hpke_open_team_join<decltype(kdf)::value, decltype(aead)::value>),
                         waves_grid(q.n), dim3(256), 0, c->stream, q.n, q.S, q.L, q.bc, dh, encs,
                         enc_pitch, payloads, ppitch, q.pslen, q.slen, parts_of(q), flags_of(q),
                         q.status);
    });
  }
  e = hipGetLastError();
  if (e != hipSuccess) return fail(e);
  {
    PROF(KID_HPKE_TEAM_WIPE);
    const unsigned gx =
        (unsigned)std::min<uint64_t>(((uint64_t)q.slen + 256 * 16 - 1) / (256 * 16), 256);
    hipLaunchKernelGGL(k_hpke_team_wipe, dim3(std::max(gx, 1u), q.n), dim3(256), 0, c->stream,
                       q.n, out, spitch, q.slen, q.status);
  }
  e = hipGetLastError();
  if (e != hipSuccess) return fail(e);
  return 0;
}

int launch_seal_team_split(prio3gpu_ctx* c, const SplitShareCall& q, const uint32_t* eph,
                           const uint8_t* shares, uint64_t spitch, uint8_t* encs,
                           uint64_t enc_pitch, uint8_t* payloads, uint64_t ppitch) {
  {
    PROF(KID_HPKE_SEAL_TEAM_SPLIT);
    hpke_suite_dispatch(q.bc, [&](auto kdf, auto aead) {
      hipLaunchKernelGGL((k_hpke_seal_team_split<decltype(kdf)::value, decltype(aead)::value>),
                         waves_grid((uint64_t)q.n * q.S), dim3(256), 0, c->stream, q.n, q.S, q.L,
                         q.bc, q.tid, eph, q.rids, q.times, q.pubs, q.pslen, shares, q.slen,
                         spitch, payloads, ppitch, q.status, parts_of(q));
    });
  }
  HIPCHK(hipGetLastError());
  {
    PROF(KID_HPKE_SEAL_TEAM_JOIN);
    hpke_suite_dispatch(q.bc, [&](auto kdf, auto aead) {
      hipLaunchKernelGGL((k_hpke_seal_team_join<decltype(kdf)::value, decltype(aead)::value>),
                         waves_grid(q.n), dim3(256), 0, c->stream, q.n, q.S, q.L, q.bc, eph,
                         q.pslen, q.slen, parts_of(q), encs, enc_pitch, payloads, ppitch,
                         q.status);
    });
  }
  HIPCHK(hipGetLastError());
  return 0;
}

}  // namespace p3g::eng
