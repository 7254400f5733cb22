/*
 * prio3gpu.h -- C ABI of the MI355X (gfx950) batched Prio3 preparation + aggregation engine.
 *
 * This is the drop-in boundary for Janus's leader/helper aggregate-init hot path.  The reference
 * (Janus 0.6, DAP-07) calls prio 0.15.1's `prio::vdaf::Aggregator` trait ONE REPORT AT A TIME:
 *
 *   trait Aggregator<16, 16>            (prio 0.15.1 src/vdaf.rs; surface mirrored by the fake VDAF
 *                                        at core/src/test_util/dummy_vdaf.rs:80-141)
 *     prepare_init(verify_key, agg_id, &(), nonce, public_share, input_share)
 *         -> (PrepareState, PrepareShare)                       -> prio3gpu_prepare_init
 *     prepare_shares_to_prepare_message(&(), [PrepareShare; 2])
 *         -> PrepareMessage                                     -> prio3gpu_prepare_shares_to_prepare_message
 *     prepare_next(PrepareState, PrepareMessage)
 *         -> PrepareTransition::Finish(OutputShare)             -> prio3gpu_prepare_next
 *     aggregate(&(), impl IntoIterator<OutputShare>) -> AggregateShare
 *   Aggregatable::{merge, accumulate}  (dummy_vdaf.rs:230-242)  -> prio3gpu_prepare_next(agg != NULL),
 *                                                                  prio3gpu_agg_merge_bytes
 *   Collector::unshard (collector/src/lib.rs:539)               -> prio3gpu_agg_read + host sum
 *
 * called from
 *   helper  aggregator/src/aggregator.rs:1775-1797   helper_initialized + evaluate + accumulate
 *                                                    -> prio3gpu_helper_init (fused, whole job)
 *   leader  aggregator/src/aggregator/aggregation_job_driver.rs:362-380   leader_initialized
 *                                                    -> prio3gpu_prepare_init(agg_id = 0)
 *           aggregation_job_driver.rs:579-627         leader_continued + accumulate
 *                                                    -> prio3gpu_prepare_next(agg != NULL)
 *   accumulate aggregator/src/aggregator/accumulator.rs:76-122  (per batch identifier)
 *   VDAF construction aggregator/src/aggregator.rs:797-840 (TaskAggregator::new)
 *                                                    -> prio3gpu_ctx_create
 *
 * Every batch entry point takes n reports.  Buffers hold the DAP/VDAF little-endian encodings,
 * report-major (report r at base + r * <len>).  They may be HOST or DEVICE pointers (detected);
 * device pointers avoid all PCIe traffic.  Errors never fail a whole batch for one report:
 * per-report status bytes mirror DAP `PrepareError` (messages/src/lib.rs:2288-2298):
 *   0 = ok, 3 = HpkeUnknownConfigId, 4 = HpkeDecryptError (HPKE stage), 5 = VdafPrepError,
 *   8 = InvalidMessage.  A report whose status is non-zero on entry to
 * a later stage is skipped by that stage (its outputs are left as zeros).
 * Return codes: 0 = ok, < 0 = API error (bad argument, HIP failure).
 *
 * Thread safety: one context may be used by one thread at a time; create one context per
 * concurrent job driver (each context owns its own HIP stream).
 */
#ifndef PRIO3GPU_H
#define PRIO3GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* VDAF kinds (VdafInstance, core/src/task.rs:24-59).  Prio3CountVec{length} is
 * SUMVEC with bits = 1 (aggregator.rs:805-813). */
enum prio3gpu_kind {
  PRIO3GPU_COUNT = 0,     /* Prio3Count                     Field64  */
  PRIO3GPU_SUM = 1,       /* Prio3Sum { bits }               Field128 */
  PRIO3GPU_SUMVEC = 2,    /* Prio3SumVec { bits, length, chunk_length }  Field128 */
  PRIO3GPU_HISTOGRAM = 3, /* Prio3Histogram { length, chunk_length }     Field128 */
  /* Prio3FixedPoint{16,32,64}BitBoundedL2VecSum { length } (core/src/task.rs:24-59,
   * aggregator.rs:839-861): bits = 16/32/64 (FixedI16<U15>/FixedI32<U31>/FixedI64<U63>),
   * length = entries; chunk_length is ignored (prio picks both gadgets' chunk lengths with
   * optimal_chunk_length).  Field128, algorithm ID 0xFFFF0000.  prio3gpu_shard takes the raw
   * two's-complement entries (see there). */
  PRIO3GPU_FPVEC = 4
};

enum prio3gpu_status {
  PRIO3GPU_OK = 0,
  PRIO3GPU_HPKE_UNKNOWN_CONFIG_ID = 3,
  PRIO3GPU_HPKE_DECRYPT_ERROR = 4,
  PRIO3GPU_VDAF_PREP_ERROR = 5,
  PRIO3GPU_INVALID_MESSAGE = 8
};

enum prio3gpu_err {
  PRIO3GPU_E_OK = 0,
  PRIO3GPU_E_ARG = -1,
  PRIO3GPU_E_HIP = -2,
  PRIO3GPU_E_RCCL = -3,
  PRIO3GPU_E_CAPACITY = -4,
  PRIO3GPU_E_HPKE = -5,        /* HPKE open/seal failed (bad key, tag mismatch) */
  PRIO3GPU_E_UNSUPPORTED = -6, /* HPKE suite not supported */
  /* The whole request is invalid (DAP "invalidMessage" for the request, not one report):
   * duplicate report IDs (aggregator.rs:1588-1598), an aggregation parameter that is not
   * Prio3's empty `()` (aggregator.rs:1605). */
  PRIO3GPU_E_INVALID_MESSAGE = -7
};

typedef struct prio3gpu_ctx prio3gpu_ctx;
typedef struct prio3gpu_state prio3gpu_state;
typedef struct prio3gpu_agg prio3gpu_agg;
typedef struct prio3gpu_comm prio3gpu_comm;

/* Sizes of the encodings for a configured context. */
typedef struct prio3gpu_sizes {
  uint32_t field_size;          /* 8 (Field64) or 16 (Field128) */
  uint32_t meas_len;            /* measurement-share length (field elements) */
  uint32_t proof_len;           /* proof-share length */
  uint32_t verifier_len;
  uint32_t joint_rand_len;
  uint32_t output_len;
  uint32_t leader_input_share;  /* bytes: meas || proof || [blind] */
  uint32_t helper_input_share;  /* bytes: meas seed || proof seed || [blind] */
  uint32_t public_share;        /* bytes: [part_0 || part_1] */
  uint32_t prep_share;          /* bytes: verifier || [part] */
  uint32_t prep_msg;            /* bytes: [joint rand seed] */
  uint32_t aggregate_share;     /* bytes: output_len * field_size */
} prio3gpu_sizes;

/* Prio3::new_{count,sum,sum_vec,histogram,fixedpoint_boundedl2_vec_sum}(2, ...) + verify key
 * (aggregator.rs:797-861).
 * `bits`, `length`, `chunk_length` are ignored where the kind does not use them.
 * `device` = HIP device ordinal. */
int prio3gpu_ctx_create(int kind, uint32_t bits, uint32_t length, uint32_t chunk_length,
                        const uint8_t verify_key[16], int device, prio3gpu_ctx** out);
/* The XOF behind every Prio3 stream of a context.  PRIO3GPU_XOF_SHAKE128 is prio 0.15.1's
 * XofShake128 (VDAF-07; what Janus 0.6 runs, aggregator/src/aggregator.rs:73) and the default of
 * prio3gpu_ctx_create.  PRIO3GPU_XOF_TURBOSHAKE128 is draft-irtf-cfrg-vdaf-08+'s
 * XofTurboShake128 (Keccak-p[1600, 12], domain byte 0x01) over the same message framing, with the
 * rest of Prio3 unchanged: a forward-compatibility mode, parity unpinned (no reference vectors). */
#define PRIO3GPU_XOF_SHAKE128 0
#define PRIO3GPU_XOF_TURBOSHAKE128 1
int prio3gpu_ctx_create2(int kind, uint32_t bits, uint32_t length, uint32_t chunk_length,
                         const uint8_t verify_key[16], int device, int xof, prio3gpu_ctx** out);
int prio3gpu_ctx_destroy(prio3gpu_ctx* ctx);
int prio3gpu_ctx_sizes(const prio3gpu_ctx* ctx, prio3gpu_sizes* out);
/* Wait for all work queued on the context's stream. */
int prio3gpu_ctx_sync(prio3gpu_ctx* ctx);
/* Async mode (default off): a call whose buffers are ALL device memory returns once its work is
 * queued on the context's stream instead of waiting for it (calls with any host buffer still
 * wait: their staging copies / results need it).  Lets a job driver queue job k+1 behind job k
 * (Janus runs aggregation jobs concurrently, aggregator/src/binary_utils/job_driver.rs:119-216);
 * order work across contexts with prio3gpu_ctx_wait and finish with prio3gpu_ctx_sync. */
int prio3gpu_ctx_set_async(prio3gpu_ctx* ctx, int on);
/* Engine options of a context (all default to the measured-fastest path; each alternative is
 * parity-tested against the oracle; value 0/1 for switches):
 *   "speculate"     1: accumulate from k_jr's per-wave column sums; 0: direct accumulation
 *   "wires_mfma"    1: SumVec (chunk > 64) wire pass on the matrix cores; 0: VALU k_flp_wires
 *   "wires_cols"    1: chunk <= 64 lane-per-column wire pass; 0: VALU k_flp_wires
 *   "fused_helper"  1: FixedPoint helper XOF pipeline (k_helper_xof); 0: exact two-pass path
 *   "helper_snap"   1: FixedPoint helper states (created after the call) keep 200-B sponge
 *                   snapshots of every 64th block instead of the expanded measurement share
 *                   (1/54 of its HBM); its rows are regenerated per chunk where they are read
 *                   (FLP query, accumulation past the column sums, output shares); 0: full rows
 *   "snap_chunk"    reports per FixedPoint query / regeneration chunk (default 512; the
 *                   regenerated rows of one chunk are the only full-size helper scratch)
 *   "query_overlap" 1 (default): the snapshot-mode helper query regenerates half-chunk i + 1 on a
 *                   second stream while half-chunk i is queried (two scratch halves); 0: in turn
 *   "wave_prio"     1: FixedPoint chain waves (k_helper_xof, k_jr_ring; the lane-pair kernels'
 *                   sponge waves only) issue at s_setprio 3 and the FixedPoint matrix-core wire
 *                   passes at 2 over co-running waves; 2: also the lane-pair kernels' storer /
 *                   loader waves; 0: all at 0
 *   "jr_ring"       1: FixedPoint leader joint-rand part via k_jr_ring; 0: k_jr
 *   "pair_chains"   1: the FixedPoint chains (k_helper_xof_pair, k_jr_ring_pair) keep each
 *                   sponge state on a lane pair, bit-interleaved (half the instructions on the
 *                   latency-bound chain; 64 / 128 reports per workgroup); 0: one lane per state
 *   "chain_pairs"   (pair_chains 0) 64-report chains per k_helper_xof / k_jr_ring workgroup: 1, 2, or 0 (auto,
 *                   default: 2 once the launch would take more than half the CUs, so a leader's
 *                   and a helper's launches side by side keep one sponge wave per SIMD)
 *   "spread"        1: latency-bound sponge launches take one CU per workgroup
 *   "spread_lds"    the dynamic LDS bytes that spreading requests (default 98304 = one workgroup
 *                   per CU; <= 81920 lets two, e.g. a leader's and a helper's, share a CU)
 *   "expand_lds", "jr_lds"  dynamic LDS bytes per k_expand / k_jr block (0 = none): caps those
 *                   kernels' occupancy so another context's kernels fit beside them
 *   "exact_squeeze" test switch: every XOF squeeze takes the exact per-element rejection path
 *   "hpke_gpu_suites"  the HPKE suites the GPU opens (prio3gpu_hpke_open_batch,
 *                   prio3gpu_hpke_open_report_shares_gpu, prio3gpu_helper_init_request): 0
 *                   (default) only DHKEM(X25519, HKDF-SHA256) / HKDF-SHA256 / AES-128-GCM
 *                   (0x0020 / 1 / 1); 1 every X25519 suite Janus accepts, KDF HKDF-SHA256 /
 *                   -SHA384 / -SHA512 (1-3) x AEAD AES-128-GCM / AES-256-GCM / ChaCha20-Poly1305
 *                   (1-3).  It does not add a KEM: P-256 keys are the host's unless
 *                   "hpke_gpu_p256" is on.  Any other value is PRIO3GPU_E_ARG
 *   "hpke_gpu_p256"  0 (default): DHKEM(P-256, HKDF-SHA256) (KEM 0x0010) keys are opened on the
 *                   host.  1: the GPU opens them too (k_p256_dh): 0x0010 / 1 / 1 with this option
 *                   alone, all nine 0x0010 / KDF 1-3 / AEAD 1-3 with "hpke_gpu_suites" = 1 as
 *                   well.  Independent of "hpke_gpu_suites".  1 also lets the seal entry points
 *                   (prio3gpu_hpke_seal_batch, prio3gpu_seal_input_shares and their _long forms)
 *                   and the wave-per-report opens (prio3gpu_hpke_open_long_batch,
 *                   prio3gpu_open_input_shares) take KEM 0x0010 with the KDFs and AEADs they take
 *                   under X25519 (k_p256_eph, k_p256_eph_kem; k_p256_dh); at 0 they answer
 *                   PRIO3GPU_E_UNSUPPORTED for it.  Any other value is PRIO3GPU_E_ARG
 *   "hpke_team_chacha"  0 (default): the wave-per-report entry points (prio3gpu_hpke_open_long_batch,
 *                   prio3gpu_open_input_shares, prio3gpu_hpke_seal_long_batch,
 *                   prio3gpu_seal_input_shares_long) take AES-GCM only and answer
 *                   PRIO3GPU_E_UNSUPPORTED for ChaCha20-Poly1305 (AEAD 3).  1: they take 0x0020 /
 *                   KDF 1-3 / AEAD 3 as well (chacha_poly_team.h).  It changes no other entry
 *                   point.  Any other value is PRIO3GPU_E_ARG
 *   "hpke_team_split"  0 (default) to 256: the most waves prio3gpu_open_input_shares and
 *                   prio3gpu_seal_input_shares_long give one report.  0 and 1: one wave per report,
 *                   the same kernels and launches as without the option.  k >= 2: a call whose
 *                   reports do not fill the chip by themselves cuts every report's body (6 +
 *                   input_share_len bytes) into at most k segments, a wave each, then computes the
 *                   tags per report (janus_amd/csrc/hpke_team_split.h; team_split_plan in
 *                   plan_hpke.h chooses the count from n, the body, k, the option below and the
 *                   device's wave slots, and falls back to one wave per report whenever two
 *                   segments of the smallest size do not fit or n alone fills the chip).  Output
 *                   bytes, statuses and the handling of secrets are the same either way.  It
 *                   affects those two entry points only: the packed prio3gpu_hpke_open_long_batch
 *                   and prio3gpu_hpke_seal_long_batch and every other call ignore it.  It adds no
 *                   suite: the KEM and AEAD options above apply unchanged.  Any other value is
 *                   PRIO3GPU_E_ARG
 *   "hpke_team_split_blocks"  the smallest segment "hpke_team_split" gives a wave, in 16-byte
 *                   blocks: a multiple of 256 from 256 to 2^24.  Default 16384 (256 KiB), the
 *                   smallest measured size at which a share of two such segments is sealed and
 *                   opened faster by two waves than by one: the tags per
 *                   report cost about 0.6 ms of their own under AES-GCM, so shorter segments
 *                   lose.  Any other value is PRIO3GPU_E_ARG
 * The engine reads no environment variables.  PRIO3GPU_E_ARG for an unknown name. */
int prio3gpu_ctx_set_option(prio3gpu_ctx* ctx, const char* name, int64_t value);
/* Work queued on `ctx` from now on starts only after all work queued on `other` so far. */
int prio3gpu_ctx_wait(prio3gpu_ctx* ctx, prio3gpu_ctx* other);
/* The same in two steps: mark what is queued on `ctx` now; later make another context wait for
 * that mark.  Marks live in a ring of 16 per context, each carrying a generation: waiting on a mark
 * after 16 newer ones were taken fails with PRIO3GPU_E_ARG ("stale mark") instead of waiting on
 * newer work.  prio3gpu_ctx_wait uses a private event and takes no mark.  Marking and waiting are
 * thread-safe per context. */
int prio3gpu_ctx_mark(prio3gpu_ctx* ctx, int* out_mark);
int prio3gpu_ctx_wait_mark(prio3gpu_ctx* ctx, prio3gpu_ctx* other, int mark);
/* The context's HIP stream (hipStream_t), for callers that interoperate (e.g. bench timing). */
void* prio3gpu_ctx_stream(prio3gpu_ctx* ctx);

/* Preparation state + device scratch for up to `capacity` reports of one aggregator
 * (Prio3PrepareState for a whole batch).  Every buffer the kernels of a call on the state use is
 * allocated here, after checking the total against the device's free memory: a state the device
 * cannot hold is PRIO3GPU_E_CAPACITY (the message gives the bytes needed and free) with nothing
 * allocated.
 * Callers that pass device pointers get the no-allocation guarantee: such calls on a created state
 * never allocate or grow one of its buffers.  Staging of host-pointer inputs, and prio3gpu_shard,
 * allocate on first use at a new size and report PRIO3GPU_E_CAPACITY if the device cannot hold it.
 * The context's scratch (accumulation plan and partial sums, staged outputs) grows to the largest
 * batch the context has seen.
 * (The one other exception is the FixedPoint helper's exact path after a non-canonical squeezed
 * element in snapshot mode, which allocates the full rows and also reports a failure as
 * PRIO3GPU_E_CAPACITY.)  The GPU HPKE open (prio3gpu_hpke_open_batch,
 * prio3gpu_hpke_open_report_shares_gpu) takes no state: its scratch belongs to the CONTEXT and
 * grows on demand to the largest batch the context has opened (PRIO3GPU_E_CAPACITY if the device
 * cannot hold it), so the first call at a new size does allocate. */
int prio3gpu_state_create(prio3gpu_ctx* ctx, int agg_id, size_t capacity, prio3gpu_state** out);
int prio3gpu_state_destroy(prio3gpu_state* st);
/* Row pitch of the input shares this state's prepare_init / prepare_init_xof / helper_init calls
 * read: report i's input share at input_shares + i * pitch (0 = packed, the default: pitch = the
 * input share length).  A non-zero pitch is a multiple of 16 and >= the share length.  A caller
 * that decodes leader input shares (134,944 B for SumVec(8,1000)) into 128-B-aligned rows
 * (pitch 135,040) gives k_jr's LDS-DMA windows and the FLP wire pass line-aligned rows
 * (aggregator_core/src/datastore.rs:1298-1304 decodes each LeaderStoredReport's share). */
int prio3gpu_state_set_input_pitch(prio3gpu_state* st, size_t pitch);
/* Reports of several tasks in one batch: report r of the next calls on `st` is prepared under
 * verify_keys[key_index[r]] instead of the context's key.  Of all Prio3 preparation only the query
 * randomness t = XOF(verify_key, dst5, nonce) reads the key, so the tasks need nothing else in
 * common than the context's VDAF shape (kind, bits, length, chunk length, XOF).
 * `verify_keys` and `key_index` are host or device memory; both are copied into buffers the state
 * owns, and the caller's memory is free again on return.  Those buffers are allocated by the first
 * keyed use (the index for the state's capacity; the table grows with num_keys): one more exception
 * to the no-allocation guarantee of prio3gpu_state_create, a failure being PRIO3GPU_E_CAPACITY.
 * Checked before anything is launched or changed: num_keys >= 1, n <= the state's capacity, and
 * every key_index[r] < num_keys (a device index through a host copy).  A violation is
 * PRIO3GPU_E_ARG, prio3gpu_last_error naming the first bad row, and the state's previous setting
 * stays in place.  num_keys == 0 clears the setting (verify_keys and key_index may be NULL, n is
 * ignored); a state with no keys set behaves, and launches, exactly as before this call existed.
 * The setting persists until it is replaced or cleared.  While it is set, prio3gpu_prepare_init,
 * prio3gpu_prepare_init_xof and prio3gpu_helper_init take exactly the `n` of this call (anything
 * else is PRIO3GPU_E_ARG with nothing launched), and prio3gpu_helper_init_request (one task id,
 * one request) and prio3gpu_shard return PRIO3GPU_E_ARG.  The call waits for the context's
 * stream. */
int prio3gpu_state_set_verify_keys(prio3gpu_state* st, const uint8_t* verify_keys /* num_keys x 16 */,
                                   uint32_t num_keys, const uint32_t* key_index /* n */, size_t n);

/* Aggregate shares: `num_slots` batch identifiers (caller maps BatchIdentifier -> slot). */
int prio3gpu_agg_create(prio3gpu_ctx* ctx, uint32_t num_slots, prio3gpu_agg** out);
int prio3gpu_agg_destroy(prio3gpu_agg* agg);
int prio3gpu_agg_reset(prio3gpu_agg* agg);
/* Read one slot's aggregate share (aggregate_share bytes) and report count. */
int prio3gpu_agg_read(prio3gpu_agg* agg, uint32_t slot, uint8_t* out_share, uint64_t* out_count);
/* Aggregatable::merge: slot += share (aggregate_share bytes, host or device), count += count.
 * Every element of `share` must be canonical (< p), as prio's AggregateShare decoding requires:
 * the share is checked before anything is launched (a device share through a host copy), and an
 * element >= p returns PRIO3GPU_E_ARG, prio3gpu_last_error naming its index, with the slot's
 * share and count unchanged. */
int prio3gpu_agg_merge_bytes(prio3gpu_agg* agg, uint32_t slot, const uint8_t* share,
                             uint64_t count);

/* Accumulator::update's report bookkeeping (accumulator.rs:76-122): for every report whose status
 * is 0, slot checksum ^= SHA-256(report_id) (ReportIdChecksum, core/src/report_id.rs:18-44) and
 * the slot's client_timestamp_interval is merged with [time, time + 1) (core/src/time.rs:289-312).
 * report_ids n x 16, times n x u64 (seconds), status / batch_slots may be NULL (all ok / slot 0);
 * host or device pointers.  Call with the final statuses (after prepare_next / helper_init). */
int prio3gpu_agg_update_reports(prio3gpu_agg* agg, size_t n, const uint8_t* report_ids,
                                const uint64_t* times, const uint8_t* status,
                                const uint32_t* batch_slots);
/* The slot's ReportIdChecksum (32 bytes) and interval (start, duration; 0, 0 when empty). */
int prio3gpu_agg_read_reports(prio3gpu_agg* agg, uint32_t slot, uint8_t* out_checksum,
                              uint64_t* out_interval_start, uint64_t* out_interval_duration);

/* Collector::unshard (collector/src/lib.rs:539): sum `num_shares` aggregate shares
 * (num_shares x aggregate_share bytes, host) mod p and decode the aggregate result:
 *   Count / Sum / SumVec / Histogram -> out_u128: output_len x 16-byte LE integers;
 *   FixedPoint vectors               -> out_f64:  d * 2^(1-bits) - num_measurements per entry
 *                                                 (prio to_float_bits; interop FP16 KAT). */
int prio3gpu_unshard(const prio3gpu_ctx* ctx, const uint8_t* agg_shares, size_t num_shares,
                     uint64_t num_measurements, uint8_t* out_u128, double* out_f64);

/* prepare_init for n reports with the state's agg_id (0 = leader, 1 = helper).
 *   nonces          n x 16          (report IDs)
 *   public_shares   n x public_share
 *   input_shares    n x (agg_id == 0 ? leader_input_share : helper_input_share)
 *   out_prep_shares n x prep_share   (may be NULL: kept only inside the state)
 *   status          n bytes, in/out (initialise to 0)
 * The leader's input shares must stay valid (unchanged) until prio3gpu_prepare_next on the same
 * state when they are DEVICE pointers; host inputs are copied into the state. */
int prio3gpu_prepare_init(prio3gpu_ctx* ctx, prio3gpu_state* st, size_t n, const uint8_t* nonces,
                          const uint8_t* public_shares, const uint8_t* input_shares,
                          uint8_t* out_prep_shares, uint8_t* status);
/* prio3gpu_prepare_init in two phases over the same state and n: the XOF phase (query and joint
 * randomness, the helper's share expansion; VALU-bound Keccak) and the FLP-query phase (weights +
 * one HBM pass over the measurement shares).  prepare_init == xof then query.  Split so a driver
 * can overlap one batch's HBM-bound query with another batch's Keccak on a second context.  The
 * input buffers must stay valid until the query phase.  Count has no HBM-bound half: its XOF phase
 * runs the whole query (one kernel derives t and evaluates the FLP), and its query phase only
 * copies the prep shares out. */
int prio3gpu_prepare_init_xof(prio3gpu_ctx* ctx, prio3gpu_state* st, size_t n,
                              const uint8_t* nonces, const uint8_t* public_shares,
                              const uint8_t* input_shares, uint8_t* status);
/* Optional step between the two: the latency-bound first half of the FLP query (ParallelSum types:
 * k_flp_weights -- Lagrange weights, gadget poly at t, circuit output), so a scheduler can keep it
 * out from under another context's sponge kernels and overlap only the HBM-bound wire pass
 * (prio3gpu_prepare_init_query then runs just that).  A no-op for Count / Sum / FixedPoint. */
int prio3gpu_prepare_init_weights(prio3gpu_ctx* ctx, prio3gpu_state* st, size_t n, uint8_t* status);
int prio3gpu_prepare_init_query(prio3gpu_ctx* ctx, prio3gpu_state* st, size_t n,
                                uint8_t* out_prep_shares, uint8_t* status);

/* prepare_shares_to_prepare_message for n reports (leader share, helper share) -> prep msg. */
int prio3gpu_prepare_shares_to_prepare_message(prio3gpu_ctx* ctx, size_t n,
                                               const uint8_t* leader_prep_shares,
                                               const uint8_t* helper_prep_shares,
                                               uint8_t* out_prep_msgs, uint8_t* status);

/* prepare_next for the n reports prepared in `st`: check prep msg == corrected joint-rand seed;
 * optionally write output shares (n x aggregate_share bytes) and/or accumulate into `agg` at
 * `batch_slots[r]` (NULL slots = slot 0).  Reports with non-zero status are not accumulated. */
int prio3gpu_prepare_next(prio3gpu_ctx* ctx, prio3gpu_state* st, size_t n, const uint8_t* prep_msgs,
                          uint8_t* status, uint8_t* out_output_shares, const uint32_t* batch_slots,
                          prio3gpu_agg* agg);

/* Helper aggregate-init, fused (aggregator.rs:1613-1848 for a whole job): prepare_init(1) +
 * prepare_shares_to_prepare_message(leader share, own share) + prepare_next + accumulate.
 * Writes the prep msg each report's Finish message carries. */
int prio3gpu_helper_init(prio3gpu_ctx* ctx, prio3gpu_state* st, size_t n, const uint8_t* nonces,
                         const uint8_t* public_shares, const uint8_t* helper_input_shares,
                         const uint8_t* leader_prep_shares, const uint32_t* batch_slots,
                         uint8_t* out_prep_msgs, uint8_t* status, prio3gpu_agg* agg);

/* Client::shard for n reports (prio 0.15.1 shard_with_random; SURVEY §8(f) #1: batched client
 * shard + FLP prove, used to generate inputs at scale).
 *   measurements  n x (SUMVEC or FPVEC ? length : 1) u64 (Count 0/1, Sum value, SumVec entries,
 *                 Histogram bucket index, FixedPoint raw two's-complement entries whose L2 norm
 *                 is < 1 -- prio's shard rejects others; here they yield reports that fail
 *                 verification; client/src/lib.rs:212-258)
 *   rand          n x prio3gpu_random_size() bytes, prio order:
 *                 k_meas, k_proof, [blind_helper, blind_leader], k_prove
 *   outputs       public shares, leader input shares, helper input shares (DAP encodings)
 * `st` must be a helper (agg_id 1) state of sufficient capacity; it is used as scratch. */
int prio3gpu_random_size(const prio3gpu_ctx* ctx);
int prio3gpu_shard(prio3gpu_ctx* ctx, prio3gpu_state* st, size_t n, const uint8_t* nonces,
                   const uint64_t* measurements, const uint8_t* rand, uint8_t* out_public,
                   uint8_t* out_leader, uint8_t* out_helper);

/* BatchAggregation::merged_with (aggregator_core/src/datastore/models.rs:962-991) on host
 * buffers: the merge Janus applies to the batch-aggregation shards of a batch at collection
 * (aggregate_share.rs:47-65) and prio3gpu_agg_allreduce applies to the per-GPU partials.
 *   aggregate_share  dst += src elementwise mod p (Aggregatable::merge); output_len elements of
 *                    field_size (8: Field64, 16: Field128) canonical LE bytes; both NULL: skipped
 *   report_count     dst += src
 *   checksum         dst ^= src (ReportIdChecksum::combined_with, core/src/report_id.rs:18-44)
 *   interval         Interval::merge (core/src/time.rs:289-302): a zero-duration interval is
 *                    empty and yields the other; else [min start, max end).
 * Host only (no GPU).  PRIO3GPU_E_ARG on a non-canonical share element or interval overflow. */
typedef struct prio3gpu_batch_aggregation {
  uint8_t* aggregate_share;
  uint64_t report_count;
  uint8_t checksum[32];
  uint64_t interval_start, interval_duration;
} prio3gpu_batch_aggregation;
int prio3gpu_batch_aggregation_merge(uint32_t field_size, size_t output_len,
                                     prio3gpu_batch_aggregation* dst,
                                     const prio3gpu_batch_aggregation* src);

/* Multi-GPU merge of per-GPU partial aggregates (one process per GPU).  RCCL all-gather of the
 * raw field-element bytes over xGMI, then a mod-p add kernel (RCCL sum is neither modular nor
 * 128-bit).  Counts are summed with an RCCL uint64 all-reduce.
 * agg_allreduce: total += sum over ranks of local, then local is reset (the per-GPU partial of one
 * aggregation job is flushed into the running aggregate, like Accumulator::flush_to_datastore,
 * accumulator.rs:133-215).  With total == NULL, local is replaced by the sum over ranks.
 * agg_allreduce is a collective per call: every rank must issue its flushes on a communicator in
 * the same order with the same slot count.  Within a process the communicator serialises
 * concurrent contexts, but across processes nothing orders them -- concurrent job workers that
 * flush per job need one communicator each (or prio3gpu_agg_epoch_merge below, which keeps the
 * partials across jobs and merges once per epoch). */
int prio3gpu_comm_unique_id(uint8_t out_id[128]);
int prio3gpu_comm_init(const uint8_t id[128], int nranks, int rank, int device,
                       prio3gpu_comm** out);
int prio3gpu_comm_destroy(prio3gpu_comm* comm);
int prio3gpu_agg_allreduce(prio3gpu_comm* comm, prio3gpu_ctx* ctx, prio3gpu_agg* local,
                           prio3gpu_agg* total);

/* Epoch merge: the multi-GPU contract for independent job drivers.  Each GPU keeps its partial
 * aggregate across ANY number of jobs (its own slots, keyed by the batch identifiers it saw) and
 * the ranks merge once per epoch -- a collection boundary, as aggregate_share.rs:44-66 merges the
 * batch-aggregation shards -- instead of in lockstep per job:
 *   slot_map[s]   for each of local's slots, its index in the epoch's union slot table
 *                 (union_slots entries: the sorted union of every rank's batch identifiers,
 *                 agreed over the caller's host channel, the same on every rank); injective,
 *                 < union_slots, or PRIO3GPU_SLOT_UNUSED for a slot no job of the epoch used
 *   total         union_slots slots; total[slot_map[s]] += sum over ranks of local[s] (mod p,
 *                 counts, checksum XOR, interval union, folded in rank order), then local is reset
 * Ordering contract: a collective over `comm`.  Every rank calls it once per epoch with epochs in
 * the same order, from ONE thread per communicator, and no other flush (agg_allreduce) is in
 * flight on that communicator -- give each merger (task x aggregator role) its own communicator
 * or serialise them.  Synchronous: returns after the merge has completed on this rank. */
#define PRIO3GPU_SLOT_UNUSED 0xFFFFFFFFu
int prio3gpu_agg_epoch_merge(prio3gpu_comm* comm, prio3gpu_ctx* ctx, prio3gpu_agg* local,
                             const uint32_t* slot_map, uint32_t union_slots, prio3gpu_agg* total);

/* Per-kernel timing with HIP events on the context's stream (opt-in; bench.py uses it for the
 * live roofline numbers).  prof_read returns min(kernel ids, max_kernels) and fills, per kernel id,
 * the summed milliseconds and launch count since the last read. */
int prio3gpu_prof_enable(prio3gpu_ctx* ctx, int on);
int prio3gpu_prof_read(prio3gpu_ctx* ctx, double* ms, uint64_t* launches, int max_kernels);
const char* prio3gpu_prof_kernel_name(int kernel_id);

/* ---- DAP codec edge (host-only; janus_amd/csrc/codec.cpp) ------------------------------------
 * Batched decode/encode of the aggregate-init messages around the engine,
 * replacing the per-report Decode/Encode calls of the helper and leader loops:
 *   helper  AggregationJobInitializeReq::get_decoded   aggregator.rs:1561-1612 (request body)
 *           PlaintextInputShare::get_decoded + InputShare/PublicShare::get_decoded_with_param
 *                                                        aggregator.rs:1702-1768
 *           AggregationJobResp::get_encoded             aggregator.rs:1811-1848
 *   leader  AggregationJobInitializeReq::new + encode   aggregation_job_driver.rs:329-437
 *           AggregationJobResp::get_decoded             aggregation_job_driver.rs:530-600
 * Message layouts: messages/src/lib.rs (see codec.cpp).  Offsets are byte offsets into `msg`.
 * query_type: 1 = TimeInterval, 2 = FixedSize (lib.rs:2024-2028). */
typedef struct prio3gpu_prepare_init_view {
  uint64_t report_id_off;    /* 16-byte ReportId (= VDAF nonce) */
  uint64_t time;             /* ReportMetadata time, seconds since the epoch */
  uint64_t public_share_off;
  uint64_t enc_off;          /* HpkeCiphertext encapsulated key */
  uint64_t payload_off;      /* HpkeCiphertext payload */
  uint64_t prep_share_off;   /* PingPongMessage Initialize/Continue prep share */
  uint64_t prep_msg_off;     /* PingPongMessage Continue/Finish prep msg */
  uint32_t public_share_len, enc_len, payload_len, prep_share_len, prep_msg_len;
  uint8_t hpke_config_id;
  uint8_t message_type;      /* 0 Initialize, 1 Continue, 2 Finish */
} prio3gpu_prepare_init_view;

typedef struct prio3gpu_prepare_resp_view {
  uint64_t report_id_off;
  uint64_t prep_share_off, prep_msg_off;
  uint32_t prep_share_len, prep_msg_len;
  uint8_t result;            /* PrepareStepResult: 0 Continue, 1 Finished, 2 Reject */
  uint8_t message_type;      /* Continue: PingPongMessage type */
  uint8_t error;             /* Reject: PrepareError */
} prio3gpu_prepare_resp_view;

/* AggregationJobInitializeReq -> one view per PrepareInit.  views == NULL counts only.
 * out_agg_param (may be NULL) = {offset, length}; out_batch_id (FixedSize, may be NULL) 32 bytes.
 * A malformed request is PRIO3GPU_E_ARG (Janus rejects the whole request,
 * AggregationJobInitializeReq::get_decoded at aggregator.rs:1586). */
int prio3gpu_decode_agg_init_req(const uint8_t* msg, size_t len, int query_type,
                                 uint8_t* out_batch_id, uint64_t* out_agg_param,
                                 prio3gpu_prepare_init_view* views, size_t max_views,
                                 size_t* out_n);
/* Helper: the request-level checks handle_aggregate_init_generic makes after decoding, each
 * PRIO3GPU_E_INVALID_MESSAGE for the whole request:
 *   two PrepareInits with the same report ID           (aggregator.rs:1588-1598)
 *   an aggregation parameter other than Prio3's `()`   (aggregator.rs:1605: non-empty bytes). */
int prio3gpu_check_agg_init_req(const uint8_t* msg, const prio3gpu_prepare_init_view* views,
                                size_t n, uint64_t agg_param_len);
/* Helper: pack the engine inputs of n PrepareInits (nonces n x 16, public shares, leader prep
 * shares) and record each report's structural fault WITHOUT touching its status:
 *   faults[i] = 8 InvalidMessage  public share of the wrong length        (aggregator.rs:1755-1768)
 *             = 5 VdafPrepError   not Initialize{prep share of the right length}
 *                                 (ping-pong, aggregator.rs:1775-1797 / error.rs:240-300)
 *             = 0                 none.
 * Janus reaches these checks only after HPKE open (3 / 4) and the plaintext / input-share decode
 * (8) succeeded, so the caller applies faults to the reports whose status is still 0 after those
 * stages (prio3gpu_apply_faults).  Rows of faulty reports are zeroed. */
int prio3gpu_gather_prepare_inits(const prio3gpu_sizes* sizes, const uint8_t* msg,
                                  const prio3gpu_prepare_init_view* views, size_t n,
                                  uint8_t* nonces, uint8_t* public_shares,
                                  uint8_t* leader_prep_shares, uint8_t* faults);
/* status[i] = faults[i] for every report whose status is 0 (the precedence of the helper loop,
 * aggregator.rs:1663-1797: HPKE config / decrypt, plaintext + input-share decode, public-share
 * decode, ping-pong). */
int prio3gpu_apply_faults(size_t n, const uint8_t* faults, uint8_t* status);
/* HPKE-opened PlaintextInputShares (report i = plaintexts[offsets[i] .. offsets[i+1])) ->
 * n x input share (agg_id 0: leader, 1: helper).  Undecodable, duplicate extensions or wrong
 * payload length -> InvalidMessage.  status in/out. */
int prio3gpu_decode_plaintext_input_shares(const prio3gpu_sizes* sizes, const uint8_t* plaintexts,
                                           const uint64_t* offsets, size_t n, int agg_id,
                                           uint8_t* out_input_shares, uint8_t* status);
/* Helper: AggregationJobResp from the batch outputs: status 0 -> Continue{Finish{prep msg}},
 * otherwise Reject(status).  out == NULL (or too small) reports the length in out_len. */
int prio3gpu_encode_agg_job_resp(const uint8_t* nonces, const uint8_t* prep_msgs,
                                 uint32_t prep_msg_len, const uint8_t* status, size_t n,
                                 uint8_t* out, size_t cap, size_t* out_len);
/* Leader: AggregationJobInitializeReq for the reports whose status is 0 (status may be NULL):
 * ReportShare{id, time, public share, HpkeCiphertext{config id, enc, payload}} +
 * Initialize{leader prep share}.  Variable-length enc/payload use offset arrays (n + 1). */
int prio3gpu_encode_agg_init_req(int query_type, const uint8_t* batch_id, const uint8_t* agg_param,
                                 uint32_t agg_param_len, size_t n, const uint8_t* nonces,
                                 const uint64_t* times, const uint8_t* public_shares,
                                 uint32_t public_share_len, const uint8_t* hpke_config_ids,
                                 const uint8_t* encs, const uint64_t* enc_offsets,
                                 const uint8_t* payloads, const uint64_t* payload_offsets,
                                 const uint8_t* prep_shares, uint32_t prep_share_len,
                                 const uint8_t* status, uint8_t* out, size_t cap,
                                 size_t* out_len);
/* AggregationJobResp -> one view per PrepareResp (views == NULL counts only). */
int prio3gpu_decode_agg_job_resp(const uint8_t* msg, size_t len,
                                 prio3gpu_prepare_resp_view* views, size_t max_views,
                                 size_t* out_n);
/* Leader: match the helper's responses to the n reports it sent (status 0 ones, in order):
 * Continue{Finish{prep msg}} -> prep msg; Reject(e) -> status e; anything else -> VdafPrepError.
 * A response for an unexpected report ID is an API error (the job fails). */
int prio3gpu_gather_helper_resps(const prio3gpu_sizes* sizes, const uint8_t* msg,
                                 const prio3gpu_prepare_resp_view* views, size_t n_views,
                                 const uint8_t* nonces, size_t n, uint8_t* prep_msgs,
                                 uint8_t* status);

/* ---- HPKE open on host threads (janus_amd/csrc/hpke.cpp) -------------------
 * RFC 9180 base mode, single shot, as core/src/hpke.rs:158-202 (hpke::seal / hpke::open).
 * Suites: KEM 0x20 X25519HkdfSha256 | 0x10 P256HkdfSha256; KDF 1/2/3 HkdfSha256/384/512;
 * AEAD 1/2/3 Aes128Gcm/Aes256Gcm/ChaCha20Poly1305.  Keys are the RFC 9180 serializations
 * (X25519: 32 B; P-256: 32-B scalar, 65-B uncompressed point).
 * Returns 0, PRIO3GPU_E_HPKE (decryption / key failure), PRIO3GPU_E_UNSUPPORTED (suite),
 * PRIO3GPU_E_CAPACITY (out buffer too small; the needed length is stored), PRIO3GPU_E_ARG. */
typedef struct prio3gpu_hpke_keypair {  /* HpkeKeypair (core/src/hpke.rs:233-255) */
  uint8_t config_id;
  uint16_t kem_id, kdf_id, aead_id;
  const uint8_t* public_key;
  uint32_t public_key_len;
  const uint8_t* private_key;
  uint32_t private_key_len;
} prio3gpu_hpke_keypair;

int prio3gpu_hpke_open(uint16_t kem_id, uint16_t kdf_id, uint16_t aead_id, const uint8_t* sk,
                       size_t sk_len, const uint8_t* pk, size_t pk_len, const uint8_t* enc,
                       size_t enc_len, const uint8_t* info, size_t info_len, const uint8_t* aad,
                       size_t aad_len, const uint8_t* ct, size_t ct_len, uint8_t* pt, size_t cap,
                       size_t* pt_len);
/* sk_e = ephemeral private key (NULL: fresh random; fixed keys are for tests). */
int prio3gpu_hpke_seal(uint16_t kem_id, uint16_t kdf_id, uint16_t aead_id, const uint8_t* pk,
                       size_t pk_len, const uint8_t* sk_e, size_t sk_e_len, const uint8_t* info,
                       size_t info_len, const uint8_t* aad, size_t aad_len, const uint8_t* pt,
                       size_t pt_len, uint8_t* enc, size_t enc_cap, size_t* enc_len, uint8_t* ct,
                       size_t ct_cap, size_t* ct_len);
/* SerializePublicKey(pk(sk)) -- key generation (generate_hpke_config_and_private_key,
 * core/src/hpke.rs:204-231); PRIO3GPU_E_HPKE if sk is not a valid private key. */
int prio3gpu_hpke_public_key(uint16_t kem_id, const uint8_t* sk, size_t sk_len, uint8_t* pk,
                             size_t cap, size_t* pk_len);
/* out[i] = X25519(sk, points[i]) (RFC 7748 §5; the DH of the DHKEM Decap inside hpke::open,
 * core/src/hpke.rs:184-200) for n 32-byte points under ONE private key.  simd != 0 runs groups of
 * eight in the AVX-512 IFMA ladder the batched open uses (PRIO3GPU_E_UNSUPPORTED if the host CPU
 * lacks IFMA); simd == 0 is the scalar ladder.  Exposed so tests can check one against the other. */
int prio3gpu_x25519_batch(const uint8_t* sk, const uint8_t* points, size_t n, uint8_t* out,
                          int simd);
/* Helper: open the n encrypted input shares of a decoded AggregationJobInitializeReq on
 * `threads` host threads (<= 0: all cores), replacing the per-report hpke::open of
 * aggregator.rs:1634-1700: keypair by config id (task keys first, global keys on decryption
 * failure), info = "dap-07 input share" || sender_role || recipient_role, aad = InputShareAad
 * (task_id[32], report metadata, public share).  Unknown config id -> status 3
 * (HpkeUnknownConfigId), failure -> 4 (HpkeDecryptError); reports with status != 0 on entry are
 * skipped.  offsets (n + 1) are always filled: report i's plaintext (a PlaintextInputShare for
 * prio3gpu_decode_plaintext_input_shares) is plaintexts[offsets[i] .. offsets[i+1]);
 * plaintexts == NULL is a sizing call. */
int prio3gpu_hpke_open_report_shares(const uint8_t* task_id, const prio3gpu_hpke_keypair* task_keys,
                                     size_t n_task_keys, const prio3gpu_hpke_keypair* global_keys,
                                     size_t n_global_keys, uint8_t sender_role,
                                     uint8_t recipient_role, const uint8_t* msg,
                                     const prio3gpu_prepare_init_view* views, size_t n,
                                     uint8_t* plaintexts, uint64_t* offsets, uint8_t* status,
                                     int threads);

/* ---- HPKE open on the GPU (janus_amd/csrc/hpke_gpu.h) ------------------------------------------
 * n opens under ONE keypair, one GPU lane per report, for the suites the context opens on the GPU:
 * by default the one Janus generates, DHKEM(X25519, HKDF-SHA256) / HKDF-SHA256 / AES-128-GCM
 * (0x0020 / 1 / 1); with the context option "hpke_gpu_suites" = 1 every X25519 suite (0x0020 /
 * KDF 1-3 / AEAD 1-3: HKDF-SHA256, -SHA384, -SHA512 x AES-128-GCM, AES-256-GCM,
 * ChaCha20-Poly1305); with "hpke_gpu_p256" = 1 the same choice under DHKEM(P-256, HKDF-SHA256)
 * (KEM 0x0010).  Any other suite (P-256 while that option is 0; the wider KDFs and AEADs while
 * "hpke_gpu_suites" is 0) is PRIO3GPU_E_UNSUPPORTED with nothing launched (use the host functions
 * above).  sk is 32 bytes; pk and every enc are Nenc bytes, 32 for X25519 and 65 for KEM 0x0010
 * (uncompressed points).  A P-256 keypair whose scalar is not in [1, n) or whose public key is no
 * point on the curve is PRIO3GPU_E_HPKE with nothing launched, as the host's prio3gpu_hpke_open
 * fails under it.  sk, pk and info
 * are host memory; every other pointer may be host or device (detected).  Report i has
 * enc = encs[Nenc i .. Nenc i + Nenc), aad = aads[aad_offsets[i] .. aad_offsets[i+1]), ciphertext ||
 * tag = cts[ct_offsets[i] .. ct_offsets[i+1]) and its plaintext goes to pts[pt_offsets[i] ..
 * pt_offsets[i+1]) (room for the ciphertext length - 16; a longer slot is zero-filled).
 * status in/out: non-zero on entry = skipped (the slot is zeroed); a failed open -- bad tag,
 * ciphertext shorter than the tag, an all-zero X25519 DH value, a P-256 enc that is no valid
 * point (prefix, coordinate range, curve equation), offsets that do not fit -- sets 4
 * (HpkeDecryptError) and writes zeros, never unauthenticated plaintext.  The private key reaches
 * the GPU only as a kernel argument; the device buffer that held the per-report DH values is
 * zeroed before the call returns.  Scratch belongs to the context (see prio3gpu_state_create). */
int prio3gpu_hpke_open_batch(prio3gpu_ctx* ctx, uint16_t kem_id, uint16_t kdf_id, uint16_t aead_id,
                             const uint8_t* sk, size_t sk_len, const uint8_t* pk, size_t pk_len,
                             const uint8_t* info, size_t info_len, size_t n, const uint8_t* encs,
                             const uint8_t* aads, const uint64_t* aad_offsets, const uint8_t* cts,
                             const uint64_t* ct_offsets, uint8_t* pts, const uint64_t* pt_offsets,
                             uint8_t* status);
/* prio3gpu_hpke_open_report_shares with the GPU opening every report whose first-choice key (task
 * key by config id, else global key) is of a suite above (as the context's "hpke_gpu_suites" and
 * "hpke_gpu_p256" options select), one batch per key: same arguments, offsets, statuses and
 * key-selection order.  Reports whose first choice is another suite (P-256 with "hpke_gpu_p256" at
 * 0; with "hpke_gpu_suites" at 0 also SHA-384/512, AES-256, ChaCha20) or a malformed keypair, and
 * the global-key second trial after a failed task-key open, run on the host path
 * on `threads` threads.  The plaintext slot of a report that ends with a
 * non-zero status is unspecified in both functions.  All pointers are host memory. */
int prio3gpu_hpke_open_report_shares_gpu(prio3gpu_ctx* ctx, const uint8_t* task_id,
                                         const prio3gpu_hpke_keypair* task_keys, size_t n_task_keys,
                                         const prio3gpu_hpke_keypair* global_keys,
                                         size_t n_global_keys, uint8_t sender_role,
                                         uint8_t recipient_role, const uint8_t* msg,
                                         const prio3gpu_prepare_init_view* views, size_t n,
                                         uint8_t* plaintexts, uint64_t* offsets, uint8_t* status,
                                         int threads);

/* ---- HPKE seal on the GPU (janus_amd/csrc/hpke_seal_gpu.h) -------------------------------------
 * n seals to ONE recipient key, one GPU lane per report, each under its own ephemeral key: the
 * batched hpke::seal (core/src/hpke.rs:158-182).  Suites: DHKEM(X25519, HKDF-SHA256) (KEM 0x0020)
 * with KDF 1-3 and AEAD 1-3, no context option needed, and with the context option
 * "hpke_gpu_p256" = 1 DHKEM(P-256, HKDF-SHA256) (KEM 0x0010) with the same KDFs and AEADs.  KEM
 * 0x0010 while that option is 0 (such seals stay on the host's prio3gpu_hpke_seal) or an unknown
 * KDF or AEAD is PRIO3GPU_E_UNSUPPORTED with nothing launched.  pk_len other than Nenc -- 32 for
 * X25519, 65 for P-256 (an uncompressed point) -- is PRIO3GPU_E_ARG; a P-256 pk that
 * DeserializePublicKey refuses (not 0x04 || x || y, a coordinate >= p, off the curve) is
 * PRIO3GPU_E_HPKE with nothing launched; n == 0 returns 0 and launches nothing.  pk and info are
 * host memory; every other pointer may be host or device (detected).
 * Report i is sealed under the ephemeral private key sk_es[32 i .. 32 i + 32) (X25519: clamped
 * inside; P-256: a big-endian scalar, which must lie in [1, n)) with
 * aad = aads[aad_offsets[i] .. aad_offsets[i+1]) and plaintext = pts[pt_offsets[i] ..
 * pt_offsets[i+1]); its encapsulated key goes to encs[Nenc i .. Nenc i + Nenc) and its
 * ciphertext || tag to cts[ct_offsets[i] .. ct_offsets[i+1]) (room for the plaintext length + 16; a longer slot is
 * zero-filled).  The bytes are those of prio3gpu_hpke_seal with the same sk_e.
 * status in/out: non-zero on entry = skipped; a report that is not sealed -- skipped, an all-zero
 * DH value (pk of small order, RFC 9180 §7.1.4; prio3gpu_hpke_seal returns PRIO3GPU_E_HPKE
 * there), a P-256 ephemeral scalar outside [1, n) (PRIO3GPU_E_HPKE there too), a slot shorter than the plaintext + 16, offsets that do not fit -- gets zeros in its
 * enc and ciphertext slots and, unless it was skipped, status 4 (PRIO3GPU_HPKE_DECRYPT_ERROR, the
 * ABI's one per-report HPKE failure).
 * Secrets: the engine's device copies of the ephemeral keys and of the plaintexts, and the buffer
 * of the per-report DH values (P-256: shared secrets and validity bytes), are zeroed before the call returns, on the error paths too; keys
 * and nonces never leave registers.  Scratch belongs to the context (see prio3gpu_state_create). */
int prio3gpu_hpke_seal_batch(prio3gpu_ctx* ctx, uint16_t kem_id, uint16_t kdf_id, uint16_t aead_id,
                             const uint8_t* pk, size_t pk_len, const uint8_t* info,
                             size_t info_len, size_t n, const uint8_t* sk_es, const uint8_t* aads,
                             const uint64_t* aad_offsets, const uint8_t* pts,
                             const uint64_t* pt_offsets, uint8_t* encs, uint8_t* cts,
                             const uint64_t* ct_offsets, uint8_t* status);
/* Client: seal n Prio3 input shares to one aggregator (Client::prepare_report's per-aggregator
 * half, client/src/lib.rs:228-251) without materialising a frame.  Report i's plaintext is the
 * PlaintextInputShare with no extensions -- 00 00, the share length as u32 big-endian, then
 * input_shares[i pitch .. i pitch + input_share_len) -- and its AAD the InputShareAad of task_id,
 * report_ids[16 i ..], times[i] (u64, seconds; encoded big-endian) and public_shares[i
 * public_share_len ..] with its u32 length prefix; both are read from the caller's rows lane by
 * lane and never written to memory.  info = "dap-07 input share" || Client || recipient_role.
 * Report i's encapsulated key (Nenc bytes: 32, or 65 for KEM 0x0010, at any alignment) goes to
 * out_encs + i enc_pitch and its payload, exactly
 * 6 + input_share_len + 16 bytes, to out_payloads + i payload_pitch; no other byte of either
 * buffer is written, so both may be columns of one fixed-stride Report buffer.  A pitch of 0 is
 * the packed one (the row's own length); a pitch shorter than its row is PRIO3GPU_E_ARG.
 * task_id and pk are host memory; every other pointer may be host or device (detected), the
 * device outputs of the sharding call being the intended input.  Suites, sk_es, status and the
 * handling of secrets are prio3gpu_hpke_seal_batch's. */
int prio3gpu_seal_input_shares(prio3gpu_ctx* ctx, const uint8_t* task_id, uint16_t kem_id,
                               uint16_t kdf_id, uint16_t aead_id, const uint8_t* pk,
                               size_t pk_len, uint8_t recipient_role, size_t n,
                               const uint8_t* report_ids, const uint64_t* times,
                               const uint8_t* public_shares, uint32_t public_share_len,
                               const uint8_t* input_shares, uint32_t input_share_len,
                               size_t input_share_pitch, const uint8_t* sk_es, uint8_t* out_encs,
                               size_t enc_pitch, uint8_t* out_payloads, size_t payload_pitch,
                               uint8_t* status);

/* ---- HPKE open of long ciphertexts on the GPU (janus_amd/csrc/hpke_open_team.h) -----------------
 * n opens under ONE keypair, one GPU WAVE per report: what the leader does once per upload with an
 * input share of a hundred kilobytes (aggregator.rs:1325-1497), where a lane per report would walk
 * each ciphertext alone.  Suites: DHKEM(X25519, HKDF-SHA256) (KEM 0x0020) with KDF 1-3 and
 * AES-128-GCM / AES-256-GCM (AEAD 1, 2), no context option needed, and with the context option
 * "hpke_team_chacha" = 1 ChaCha20-Poly1305 (AEAD 3) too; with "hpke_gpu_p256" = 1 the same under
 * DHKEM(P-256, HKDF-SHA256) (KEM 0x0010: k_p256_dh, then the same wave per report).  KEM 0x0010 or
 * AEAD 3 while its option is 0, or an unknown id, is PRIO3GPU_E_UNSUPPORTED with nothing launched;
 * n == 0 returns 0 and launches nothing.  sk is 32 bytes; pk and every enc are Nenc bytes, 32 for
 * X25519 and 65 for KEM 0x0010; another length is PRIO3GPU_E_ARG, and a P-256 keypair whose scalar
 * is not in [1, n) or whose public key is no point is PRIO3GPU_E_HPKE before any launch.
 * prio3gpu_hpke_open_long_batch has the arguments and contracts of prio3gpu_hpke_open_batch --
 * host or device pointers, status in/out, zero-filled slots, zeros and status 4 for a failed
 * open, the handling of secrets -- and the same plaintexts, for every ciphertext length from 16
 * (an empty plaintext) up. */
int prio3gpu_hpke_open_long_batch(prio3gpu_ctx* ctx, uint16_t kem_id, uint16_t kdf_id,
                                  uint16_t aead_id, const uint8_t* sk, size_t sk_len,
                                  const uint8_t* pk, size_t pk_len, const uint8_t* info,
                                  size_t info_len, size_t n, const uint8_t* encs,
                                  const uint8_t* aads, const uint64_t* aad_offsets,
                                  const uint8_t* cts, const uint64_t* ct_offsets, uint8_t* pts,
                                  const uint64_t* pt_offsets, uint8_t* status);
/* Upload: open n Prio3 input shares sealed to this aggregator (handle_upload_generic's decrypt and
 * decode, aggregator.rs:1325-1497), the mirror of prio3gpu_seal_input_shares, a wave per report
 * and for the suites above (AEAD 3 with "hpke_team_chacha" = 1, PRIO3GPU_E_UNSUPPORTED without
 * it).  Report i's
 * encapsulated key (Nenc bytes: 32, or 65 for KEM 0x0010) is read from encs + i enc_pitch and
 * its payload, exactly
 * 6 + input_share_len + 16 bytes, from payloads + i payload_pitch, so both may be columns of one
 * fixed-stride Report buffer; its AAD is the InputShareAad of task_id, report_ids[16 i ..],
 * times[i] and public_shares[i public_share_len ..], never written to memory;
 * info = "dap-07 input share" || Client || recipient_role.  The plaintext must be the
 * PlaintextInputShare with no extensions -- 00 00, input_share_len as u32 big-endian, the share
 * -- and the share goes to out_shares + i share_pitch; no other byte of out_shares is written.
 * out_shares may be device memory at a 128-byte-aligned pitch: after
 * prio3gpu_state_set_input_pitch, prio3gpu_prepare_init reads the rows in place.  A pitch of 0 is
 * the packed one (the row's own length); a pitch shorter than its row is PRIO3GPU_E_ARG.
 * status in/out: non-zero on entry = skipped (the row is zeroed); a failed open (bad tag, an
 * all-zero X25519 DH value, a P-256 enc that is no valid point) sets 4 and writes zeros; an authentic plaintext with any other six leading
 * bytes -- extensions, another length: at this payload length either means a share of the wrong
 * size -- sets 8 (InvalidMessage, "Leader input share decoding failed") and writes zeros.
 * task_id, sk and pk are host memory; every other pointer may be host or device (detected).
 * Secrets: the private key reaches the GPU only as a kernel argument; the buffer of the DH values
 * and the engine's staged copy of the opened rows (host out_shares) are zeroed before the call
 * returns; keys, nonces and round keys never leave registers.
 * Output contract: no unauthenticated plaintext is in out_shares once the call's work on the
 * context's stream is done -- in an async context before anything queued later on the stream runs,
 * for a host out_shares before the copy-out.  With "hpke_team_split" >= 2 a report may get several
 * waves: the rows then hold plaintext without a verdict between the call's own kernels (segments,
 * then the verdicts per report, then zeros over every row whose status is not 0, queued back to
 * back), and nowhere else; the segments' sums and header flags in the engine's scratch are
 * key-derived and zeroed before the call returns, on its error paths too. */
int prio3gpu_open_input_shares(prio3gpu_ctx* ctx, const uint8_t* task_id, uint16_t kem_id,
                               uint16_t kdf_id, uint16_t aead_id, const uint8_t* sk, size_t sk_len,
                               const uint8_t* pk, size_t pk_len, uint8_t recipient_role, size_t n,
                               const uint8_t* report_ids, const uint64_t* times,
                               const uint8_t* public_shares, uint32_t public_share_len,
                               const uint8_t* encs, size_t enc_pitch, const uint8_t* payloads,
                               size_t payload_pitch, uint32_t input_share_len,
                               uint8_t* out_shares, size_t share_pitch, uint8_t* status);

/* ---- HPKE seal of long plaintexts on the GPU (janus_amd/csrc/hpke_seal_team.h) ------------------
 * n seals to ONE recipient key, one GPU WAVE per report, each under its own ephemeral key: what a
 * client does with the leader's input share of a hundred kilobytes, where a lane per report would
 * walk each plaintext alone; the mirror of prio3gpu_hpke_open_long_batch.  Suites:
 * DHKEM(X25519, HKDF-SHA256) (KEM 0x0020) with KDF 1-3 and AES-128-GCM / AES-256-GCM (AEAD 1, 2),
 * no context option needed, and with the context option "hpke_team_chacha" = 1
 * ChaCha20-Poly1305 (AEAD 3) too; with "hpke_gpu_p256" = 1 the same under DHKEM(P-256,
 * HKDF-SHA256) (KEM 0x0010), pk and encs as prio3gpu_hpke_seal_batch takes them.  AEAD 3 while its
 * option is 0 (it stays on prio3gpu_hpke_seal_batch), KEM 0x0010 while its option is 0, or an
 * unknown id is PRIO3GPU_E_UNSUPPORTED with nothing launched; n == 0 returns 0 and launches nothing.
 * prio3gpu_hpke_seal_long_batch has the arguments and contracts of prio3gpu_hpke_seal_batch --
 * host or device pointers, status in/out, zero-filled slots, zeros and status 4 for a report that
 * is not sealed, the handling of secrets (round keys too never leave registers; the wave's table
 * of powers of H in LDS is zeroed before the wave ends) -- and the same bytes, for every plaintext
 * length from 0 up and a ciphertext slot at any alignment. */
int prio3gpu_hpke_seal_long_batch(prio3gpu_ctx* ctx, uint16_t kem_id, uint16_t kdf_id,
                                  uint16_t aead_id, const uint8_t* pk, size_t pk_len,
                                  const uint8_t* info, size_t info_len, size_t n,
                                  const uint8_t* sk_es, const uint8_t* aads,
                                  const uint64_t* aad_offsets, const uint8_t* pts,
                                  const uint64_t* pt_offsets, uint8_t* encs, uint8_t* cts,
                                  const uint64_t* ct_offsets, uint8_t* status);
/* Client: prio3gpu_seal_input_shares with a wave per report, for the suites above (AEAD 3 with
 * "hpke_team_chacha" = 1, PRIO3GPU_E_UNSUPPORTED without it): the same
 * arguments, pitches (0 = packed; shorter than the row = PRIO3GPU_E_ARG), statuses, handling of
 * secrets and bytes.  The enc and payload columns may sit at any alignment (a whole 16-byte block
 * leaves as the widest naturally aligned pieces its address allows); no byte outside the two
 * columns is written.  With "hpke_team_split" >= 2 a report may get several waves (the option's
 * comment): the same bytes and statuses; the segments' sums in the engine's scratch are zeroed
 * before the call returns like the ladders' output. */
int prio3gpu_seal_input_shares_long(prio3gpu_ctx* ctx, const uint8_t* task_id, uint16_t kem_id,
                                    uint16_t kdf_id, uint16_t aead_id, const uint8_t* pk,
                                    size_t pk_len, uint8_t recipient_role, size_t n,
                                    const uint8_t* report_ids, const uint64_t* times,
                                    const uint8_t* public_shares, uint32_t public_share_len,
                                    const uint8_t* input_shares, uint32_t input_share_len,
                                    size_t input_share_pitch, const uint8_t* sk_es,
                                    uint8_t* out_encs, size_t enc_pitch, uint8_t* out_payloads,
                                    size_t payload_pitch, uint8_t* status);

/* ---- Helper aggregate-init from the request's bytes (janus_amd/csrc/helper_request.h) -----------
 * One call per aggregation job, on one context: the decoded AggregationJobInitializeReq in, prep
 * messages out.  Equivalent, with agg_id = 1, to
 *   prio3gpu_gather_prepare_inits -> prio3gpu_hpke_open_report_shares_gpu ->
 *   prio3gpu_decode_plaintext_input_shares -> prio3gpu_apply_faults -> prio3gpu_helper_init
 * with the same per-report statuses and precedence (HPKE 3 / 4, then plaintext or input-share
 * decode 8, then public-share length 8, then ping-pong 5; aggregator.rs:1663-1797) and
 * byte-identical prep messages, aggregate shares and counts.
 *   msg, msg_len   the request: host memory (pinned or pageable) or device memory (detected).  It
 *                  crosses PCIe once; no packed enc / aad / ciphertext arrays are built on the
 *                  host for the reports the GPU opens, and their plaintexts and decoded input
 *                  shares never leave the device.
 *   views, n       prio3gpu_decode_agg_init_req's views, host memory.  Every offset and length is
 *                  checked against msg_len before anything reads through it: a view that does not
 *                  fit is PRIO3GPU_E_ARG for the call with nothing launched, and no kernel reads
 *                  past msg.  n == 0 returns 0 and launches nothing.
 *   status         n bytes, host memory, in/out as in prio3gpu_hpke_open_report_shares: a report
 *                  whose status is non-zero on entry is skipped and keeps that status.
 *   out_nonces     n x 16 report IDs (may be NULL); out_prep_msgs n x prep_msg (may be NULL); host
 *                  or device memory.  batch_slots / agg as in prio3gpu_helper_init.
 * Reports whose first-choice key (task key by config id, else global key) is X25519 / HKDF-SHA256
 * / AES-128-GCM -- or, with the context option "hpke_gpu_suites" = 1, any X25519 suite (KDF 1-3 x
 * AEAD 1-3), and with "hpke_gpu_p256" = 1 the same under DHKEM(P-256, HKDF-SHA256) -- are opened
 * and decoded on the GPU, one kernel pair per key.  The host path
 * (prio3gpu_hpke_open_report_shares + prio3gpu_decode_plaintext_input_shares on `threads`
 * threads) takes, inside the call, the reports whose first choice is another suite or a malformed
 * key, the global-key second trial after a failed task-key open, and the plaintexts whose
 * extension list is longer than 256 bytes (the device parser's duplicate check is quadratic in
 * the item count, so a lane is never given more than 64 items); only those reports' input shares
 * and statuses are uploaded.  A job with no such report does no host crypto.
 * Secrets: a private key reaches the GPU only as a kernel argument; the device buffers that held
 * the DH values and the plaintexts are zeroed before the call returns, on the error paths too.
 * Scratch belongs to the context and grows to the largest job seen (PRIO3GPU_E_CAPACITY if the
 * device cannot hold it).  `st` is a helper (agg_id 1) state of capacity >= n.  Synchronous. */
int prio3gpu_helper_init_request(prio3gpu_ctx* ctx, prio3gpu_state* st, const uint8_t* task_id,
                                 const prio3gpu_hpke_keypair* task_keys, size_t n_task_keys,
                                 const prio3gpu_hpke_keypair* global_keys, size_t n_global_keys,
                                 uint8_t sender_role, uint8_t recipient_role, const uint8_t* msg,
                                 size_t msg_len, const prio3gpu_prepare_init_view* views, size_t n,
                                 const uint32_t* batch_slots, uint8_t* out_nonces,
                                 uint8_t* out_prep_msgs, uint8_t* status, prio3gpu_agg* agg,
                                 int threads);

/* Last error message for this thread (static storage). */
const char* prio3gpu_last_error(void);
/* Build identity: the SHA-256 (hex) of the sources, headers and compiler flags the library was
 * built from ("unhashed" for a build outside janus_amd/_lib.py).  A caller (the Rust build.rs,
 * janus_amd/_lib.py) rejects a library whose hash is not that of the sources it ships with. */
const char* prio3gpu_build_hash(void);

#ifdef __cplusplus
}
#endif
#endif /* PRIO3GPU_H */
