// What engine_hpke.hip asks of engine_hpke_split.hip, the unit that holds hpke_team_split.h's
// kernels (several waves per report; eighteen more instantiations per direction, compiled beside
// the HPKE unit instead of after it): the launches of one share-row call, host side only.  No
// kernel header is included here.
#pragma once
#include "engine_internal.h"
#include "hpke_lane.h"
#include "hpke_shared.h"

namespace p3g::eng {

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

}  // namespace p3g::eng
