// What the engine's translation units (engine.hip, engine_hpke*.hip) share on the host: the error
// macros, the device buffer, the kernel ids and their HIP-event timing, the three objects behind
// the ABI's handles, and the few helpers both units call.  No kernel header is included here, so a
// unit gets only the kernels it includes itself.
#pragma once
#include <hip/hip_runtime.h>

#include <initializer_list>
#include <mutex>
#include <vector>

#include "../../include/prio3gpu.h"
#include "cfg.h"
#include "errors.h"
#include "plan_accum.h"
#include "rows.h"

#define set_err p3g::set_error

#define HIPCHK(x)                                                                 \
  do {                                                                            \
    hipError_t e_ = (x);                                                          \
    if (e_ != hipSuccess) {                                                       \
      set_err("%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
      return PRIO3GPU_E_HIP;                                                      \
    }                                                                             \
  } while (0)

#define CHK(x)                   \
  do {                           \
    int rc_ = (x);               \
    if (rc_ != 0) return rc_;    \
  } while (0)

namespace p3g::eng {

// Grow-only device buffer; owns its allocation (freed on destruction, never copied).  Every
// per-state buffer the kernels use is sized by prio3gpu_state_create (a hipFree inside a call
// would wait for the whole device).  Callers that pass device pointers get the no-allocation
// guarantee: such calls on a created state never allocate or grow one of its buffers.  Staging of
// host-pointer inputs, and prio3gpu_shard, allocate on first use at a new size and report
// PRIO3GPU_E_CAPACITY if the device cannot hold it.  The context's scratch (accumulation plan and
// partial sums, staged outputs) grows to the largest batch the context has seen.  A state's
// verify-key table and key index (prio3gpu_state_set_verify_keys) are allocated by the first keyed
// use, the index for the state's capacity; the table grows with the number of keys.  An allocation
// the device cannot hold is PRIO3GPU_E_CAPACITY, with the HIP error cleared so the next launch
// check of the same context does not report it.
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  int ensure(size_t bytes) {
    if (bytes <= cap) return 0;
    if (p) HIPCHK(hipFree(p));
    p = nullptr;
    cap = 0;
    const size_t want = bytes ? bytes : 16;
    const hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      p = nullptr;
      size_t fr = 0, tot = 0;
      (void)hipMemGetInfo(&fr, &tot);
      set_err("device allocation of %zu bytes failed: %s (%zu of %zu bytes free)", want,
              hipGetErrorString(e), fr, tot);
      return e == hipErrorOutOfMemory ? PRIO3GPU_E_CAPACITY : PRIO3GPU_E_HIP;
    }
    cap = bytes;
    return 0;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  uint8_t* u8() const { return static_cast<uint8_t*>(p); }
};

// One id per kernel, named exactly as rocprofv3 reports it (kernel-trace names are the
// template-stripped function names), so the bench's HIP-event table and the profiles agree.
enum KernelId {
  KID_QUERY = 0, KID_EXPAND, KID_HELPER_XOF, KID_JR, KID_FLP_WEIGHTS, KID_FLP_WIRES,
  KID_FPV_WEIGHTS, KID_FPV_WIRES0, KID_FPV_WIRES1, KID_FPV_FINAL, KID_DECIDE, KID_FPV_DECIDE,
  KID_PNEXT, KID_ACC_PART, KID_ACC_SPEC, KID_ACC_MERGE, KID_OUT, KID_MERGE, KID_SHARD_SEEDS,
  KID_SHARD_MEAS, KID_SHARD_JR, KID_PROVE, KID_SHARD_PROOF, KID_REPORT_META, KID_REPORT_META_FOLD,
  KID_SHARD_NORM, KID_JR_RING, KID_FLP_QUERY_LANE, KID_FLP_WIRES_COLS, KID_FLP_WIRES_MFMA,
  KID_FPV_REGEN, KID_X25519, KID_HPKE_OPEN, KID_REQ_GATHER, KID_X25519_IDX, KID_HPKE_OPEN_REQ,
  KID_DECODE_PT, KID_REQ_SCATTER, KID_REQ_COPY, KID_P256_DH, KID_P256_DH_IDX, KID_X25519_EPH,
  KID_HPKE_SEAL, KID_HPKE_SEAL_SHARES, KID_HPKE_OPEN_TEAM, KID_HPKE_OPEN_TEAM_SHARES,
  KID_HPKE_SEAL_TEAM, KID_HPKE_SEAL_TEAM_SHARES, KID_P256_EPH, KID_P256_EPH_KEM,
  KID_HPKE_OPEN_TEAM_SPLIT, KID_HPKE_OPEN_TEAM_JOIN, KID_HPKE_TEAM_WIPE, KID_HPKE_SEAL_TEAM_SPLIT,
  KID_HPKE_SEAL_TEAM_JOIN, KID_QUERY_KEYED, KID_COUNT
};

// Per-kernel HIP-event timing on the context's stream (opt-in; used by bench.py).
struct Prof {
  bool on = false;
  struct Rec {
    int kid;
    hipEvent_t a, b;
  };
  std::vector<Rec> recs;
  std::vector<hipEvent_t> pool;
  hipEvent_t get() {
    if (!pool.empty()) {
      hipEvent_t e = pool.back();
      pool.pop_back();
      return e;
    }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
  }
};

// The context's scratch of the GPU HPKE paths (engine_hpke.hip), a member per buffer, named after
// its widest use and grown on demand to the largest call seen.  Where a call uses another
// family's member it is said here, so a reader sees which uses may overlap.

// The opens: staging of host inputs and outputs, and the ladder's DH values (dh_bytes: 32 bytes
// per report, for P-256 the shared secrets, then P-256's validity bytes).  The seals stage their
// AADs, AAD offsets, ciphertext offsets and statuses in aad, aad_off, ct_off and status;
// prio3gpu_open_input_shares has its payload rows in ct_in and its opened share rows in pt_out.
// split: the segments' sums and the header flags of a call that gives a report several waves
// (hpke_team_split.h), opens and seals alike.
struct HpkeOpenScratch {
  DevBuf enc_in, aad, aad_off, ct_in, ct_off, pt_out, pt_off, status, dh, split;
};

// The seals: staging of host inputs (ephemeral keys, plaintexts or share rows, plaintext
// offsets, report IDs, times, public shares), the ladders' output (eph_bytes) and staging of host
// outputs.  prio3gpu_open_input_shares stages its report IDs, times and public shares in rid,
// time and pub.  enc_packed has two roles: the seals' staged enc rows, and the packed copy that
// open's ladder reads when its enc column is pitched.
struct HpkeSealScratch {
  DevBuf eph_sk, eph, pt_in, pt_off, rid, time, pub, enc_packed, ct_out;
};

// prio3gpu_helper_init_request: the request, its views, the key groups' member lists, DH values
// (as HpkeOpenScratch::dh), plaintexts, their offsets, the gather's fault bytes, and the
// host-fallback reports' packed upload.
struct ReqScratch {
  DevBuf msg, views, group_idx, dh, pt, pt_off, faults, fallback;
};

}  // namespace p3g::eng

// The engine's units work inside these two namespaces; the ABI's handle types below are global.
using namespace p3g;
using namespace p3g::eng;

struct prio3gpu_ctx {
  Cfg cfg{};
  prio3gpu_sizes sz{};
  uint8_t vk[16];
  int device = 0;
  hipStream_t stream = nullptr;
  // snapshot-mode helper query: k_fpv_regen of the next half-chunk runs on `aux` beside the
  // current half-chunk's query on `stream` (created on first use); aux_ev[0..1] regenerated,
  // aux_ev[2..3] read, per scratch half
  hipStream_t aux = nullptr;
  hipEvent_t aux_ev[4] = {};
  DevBuf twiddles, twiddles1, twiddles2;
  // generic staging (inputs given as host pointers) and scratch
  DevBuf io[6];
  DevBuf perm, chunks, partials, pcounts, spec_idx;
  HpkeOpenScratch hpke;  // the GPU HPKE paths' scratch, by family (above)
  ReqScratch req;
  HpkeSealScratch seal;
  // Engine options (prio3gpu_ctx_set_option; include/prio3gpu.h lists them).  The defaults are the
  // measured-fastest paths; every alternative is parity-tested against the oracle.
  bool speculate = true;     // "speculate": accumulation from k_jr's column sums (0: direct)
  bool fused_helper = true;  // "fused_helper": FixedPoint helper via k_helper_xof (0: two-pass)
  // "helper_snap": FixedPoint helper states keep sponge snapshots instead of the expanded share
  // (k_fpv_regen rewrites it per chunk); read when a state is created
  bool helper_snap = true;
  uint32_t snap_chunk = 512;  // "snap_chunk": reports per FixedPoint query / regeneration chunk
  bool spread = true;        // "spread": one CU per workgroup for latency-bound sponge launches
  // "spread_lds": the dynamic LDS such a workgroup requests (96 KB: one per CU; <= 80 KB lets a
  // leader and a helper workgroup share a CU when both aggregators run on one GPU)
  size_t spread_lds = 96 * 1024;
  bool jr_ring = true;       // "jr_ring": FixedPoint leader joint-rand part via k_jr_ring
  // "chain_pairs": 64-report chains per k_helper_xof / k_jr_ring workgroup (0: auto -- 1 while the
  // launch takes at most half the CUs, else 2, so a leader and a helper launch side by side
  // still give every sponge wave its own SIMD)
  uint32_t chain_pairs = 0;
  // "pair_chains": the FixedPoint chains with each sponge state on a lane pair (fpvec_pair.h:
  // k_helper_xof_pair, k_jr_ring_pair; half the instructions on the latency-bound chain)
  bool pair_chains = true;
  // "query_overlap": snapshot-mode helper query regenerates half-chunk i+1 on a second stream
  // while half-chunk i is queried (two scratch halves; the default since the lane-pair chains:
  // config E 1,232 -> 1,200 ms per step at 10,240 reports, profiles/r05/pair/r5_pair8, r5_pair9;
  // with the one-lane chains it measured 1,773 vs 1,765 ms, the regeneration starving the wires)
  bool query_overlap = true;
  bool wires_mfma = true;    // "wires_mfma": SumVec chunk > 64 wire pass on the matrix cores
  bool wires_cols = true;    // "wires_cols": chunk <= 64 lane-per-column wire pass
  // "hpke_gpu_suites": which HPKE suites the GPU opens (hpke_gpu_suite): 0 only X25519 /
  // HKDF-SHA256 / AES-128-GCM, 1 every X25519 suite (KDF 1-3 x AEAD 1-3)
  bool hpke_gpu_suites = false;
  // "hpke_gpu_p256": 1 lets the GPU open DHKEM(P-256, HKDF-SHA256) too (k_p256_dh): with
  // HKDF-SHA256 / AES-128-GCM, and with every KDF and AEAD when "hpke_gpu_suites" is on as well
  bool hpke_gpu_p256 = false;
  // "hpke_team_chacha": 1 lets the wave-per-report opens and seals (hpke_team_suite) take
  // ChaCha20-Poly1305 (AEAD 3) beside AES-GCM; 0 leaves it PRIO3GPU_E_UNSUPPORTED there
  bool hpke_team_chacha = false;
  // "hpke_team_split": at most this many waves per report in prio3gpu_open_input_shares and
  // prio3gpu_seal_input_shares_long (hpke_team_split.h; 0 and 1: one wave, the one-wave kernels);
  // "hpke_team_split_blocks": the smallest segment a wave is given, in 16-byte blocks (256 KiB:
  // the smallest measured size at which two segments beat one wave)
  uint32_t hpke_team_split = 0;
  uint32_t hpke_team_split_blocks = 16384;
  size_t expand_lds = 0;     // "expand_lds": dynamic LDS per k_expand block (occupancy cap)
  size_t jr_lds = 0;         // "jr_lds": dynamic LDS per k_jr block (occupancy cap)
  uint32_t cus = 0;          // compute units of the device
  DevBuf fallback;           // k_helper_xof's non-canonical-element counter
  Prof prof;
  // async mode (prio3gpu_ctx_set_async): calls whose buffers are all device memory return once
  // their work is queued; cross-context order via prio3gpu_ctx_wait
  bool async_mode = false;
  static constexpr int kMarks = 16;
  hipEvent_t ev[kMarks] = {};  // ring of marks (prio3gpu_ctx_mark)
  uint32_t ev_gen[kMarks] = {};  // generation of each ring slot: a mark = gen * kMarks + slot
  int ev_next = 0;
  uint32_t gen_next = 1;
  hipEvent_t wait_ev = nullptr;  // prio3gpu_ctx_wait: recorded on the other context, not a mark
  int wait_ev_dev = -1;          // device wait_ev was created on (the other context's)
  std::mutex mark_mu;            // ev_next / ev_gen / wait_ev
  // the accumulation plan of the last call (plan_accum.h), as uploaded to perm / chunks /
  // spec_idx.  plan_valid: that call had no per-report slots, so a call with an equal key reuses
  // the plan on the device -- no host planning, no upload
  AccumPlan plan;
  AccumKey plan_key;
  bool plan_valid = false;
};

namespace p3g::eng {
struct ProfScope {
  prio3gpu_ctx* c;
  int kid;
  hipEvent_t a{}, b{};
  hipStream_t s;
  ProfScope(prio3gpu_ctx* c_, int kid_, hipStream_t s_ = nullptr)
      : c(c_), kid(kid_), s(s_ ? s_ : c_->stream) {
    if (c->prof.on) {
      a = c->prof.get();
      b = c->prof.get();
      (void)hipEventRecord(a, s);
    }
  }
  ~ProfScope() {
    if (c->prof.on) {
      (void)hipEventRecord(b, s);
      c->prof.recs.push_back({kid, a, b});
    }
  }
};
}  // namespace p3g::eng
#define PROF(kid) ProfScope prof_scope_##kid(c, kid)
#define PROF_ON(kid, strm) ProfScope prof_scope_##kid(c, kid, strm)

struct prio3gpu_state {
  prio3gpu_ctx* ctx = nullptr;
  int agg_id = 0;
  size_t cap = 0;
  size_t n = 0;
  size_t in_pitch = 0;  // row pitch of the caller's input shares (0: packed, the share length)
  // prio3gpu_state_set_verify_keys: the batch's key table (vk_num x 16 B) and report r's row in it
  // (vk_n x u32), allocated on the first keyed use.  vk_num == 0: the context's key, as ever.
  DevBuf vkeys, vkidx;
  uint32_t vk_num = 0;
  size_t vk_n = 0;
  DevBuf t, jr, part, seed, meas, proof, prep, msg, status, nonces, pub, input, w;
  DevBuf fpart, flags;  // FixedPointBoundedL2VecSum: wire partials per row group, query flags
  size_t fpart_rows = 0;  // reports fpart holds (the query runs in chunks of at most this many)
  // FixedPoint helper, snapshot mode (helper_snap): k_helper_xof's sponge snapshots of every
  // report; `scratch` holds one chunk of regenerated measurement-share rows.  snap_active: the
  // prepared batch's share exists only as snapshots (the fused path ran), so every reader of
  // meas_rows goes through regen_rows.
  DevBuf snaps, scratch;
  bool snap = false, snap_active = false;
  bool snap_pair = false;  // the snapshots were written by k_helper_xof_pair (dword-pair halves)
  CRows meas_rows{nullptr, 0};  // measurement shares of the prepared batch
  CRows proof_rows{nullptr, 0};  // proof shares (prepare_init_xof -> prepare_init_query)
  bool xof_done = false;         // the XOF phase ran; the query phase is due
  bool weights_done = false;     // ParallelSum: k_flp_weights of the query phase ran already
  bool query_done = false;       // Count: the XOF phase ran the whole query (fused query rand)
  // speculative accumulation: per-wave column sums of meas-share words, written by k_jr
  DevBuf spec_lo, spec_cy;
  bool spec_ok = false;
  size_t spec_n = 0;
  uint32_t spec_nd = 0, spec_e0 = 0, spec_e1 = 0;
};

struct prio3gpu_agg {
  prio3gpu_ctx* ctx = nullptr;
  uint32_t slots = 0;
  DevBuf share;   // slots x out_len x ES
  DevBuf counts;  // slots x u64
  DevBuf meta;    // slots x SlotMeta: report-ID checksum + client timestamp interval
  DevBuf wmeta;   // per-wave partials of k_report_meta
};

// The helpers engine_hpke.hip calls too (defined in engine.hip).
namespace p3g::eng {

bool is_device_ptr(const void* p);

// Make `src` (host or device, `bytes`) available on device; returns the device pointer.
// A null or empty source is passed through, unless `min_bytes` asks for a staging buffer of at
// least that size in its place (the HPKE kernels take non-null pointers).
int stage_in(prio3gpu_ctx* c, DevBuf& buf, const void* src, size_t bytes, const uint8_t** out,
             size_t min_bytes = 0);

int copy_out(prio3gpu_ctx* c, void* dst, const void* dev_src, size_t bytes);

int check_state(prio3gpu_ctx* c, prio3gpu_state* st, size_t n);

// End of an ABI call: wait for the context's stream unless the context is in async mode and every
// buffer the call touched is device memory (host inputs are staged by async copies and host
// outputs are written by them: those need the wait).
int finish_call(prio3gpu_ctx* c, std::initializer_list<const void*> bufs);

inline dim3 grid1(size_t n, uint32_t tpb) { return dim3((unsigned)((n + tpb - 1) / tpb)); }

// A keyed state (prio3gpu_state_set_verify_keys) prepares exactly the n reports its index covers.
int check_keyed_n(const prio3gpu_state* st, size_t n);

// Row pitch of a state's input shares: the caller's (prio3gpu_state_set_input_pitch) or packed.
inline size_t input_pitch(const prio3gpu_state* st) {
  const Cfg& g = st->ctx->cfg;
  return st->in_pitch ? st->in_pitch : (st->agg_id == 0 ? g.leader_share_len : g.helper_share_len);
}

}  // namespace p3g::eng
