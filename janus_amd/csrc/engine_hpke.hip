// Host side of the GPU HPKE paths (include/prio3gpu.h) and the test hooks that launch only their
// kernels.  The opens: prio3gpu_hpke_open_batch (a lane per report) and prio3gpu_hpke_open_long_
// batch (a wave per report) share hpke_open_batch_entry; prio3gpu_open_input_shares opens share
// rows in place; prio3gpu_hpke_open_report_shares_gpu packs a request's key groups for the first.
// The seals: prio3gpu_hpke_seal_batch / _long_batch share hpke_seal_batch_entry, prio3gpu_seal_
// input_shares / _long share seal_input_shares_entry.  With the "hpke_team_split" option the two
// share-row calls may give a report several waves: share_split decides.  prio3gpu_helper_init_
// request is the helper's aggregate-init from the request's bytes, in steps req_plan ...
// req_host_fallback.  Every call refuses in one order: null context, suite, keys, n == 0, null
// arguments, pitches.  This unit is the host side alone: the checks, the staging, the secrets and
// the entry points.  No kernel is in scope here: every launch is a call into one of the kernel
// units engine_hpke_*.hip through hpke_launch.h, and the request path hands over to the Prio3
// side (engine.hip) through the public prio3gpu_helper_init alone.  The context's scratch is named
// in engine_internal.h; a call's per-report secrets in it belong to one CallSecrets (below), which
// states what every path keeps about them.  The suite predicates and the column geometry are
// plan_hpke.h's (no HIP, tested on the CPU).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cassert>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/prio3gpu.h"
#include "../../include/prio3gpu_test.h"
#include "engine_internal.h"
#include "plan_hpke.h"
#include "hpke_launch.h"

using namespace p3g;
using namespace p3g::eng;

// ---- batched HPKE open on the GPU (hpke_gpu.h) --------------------------------------------------
namespace {

// stage_in's min_bytes for the HPKE inputs: a host buffer is copied into the context's scratch
// (grown on demand), an empty one included; a device buffer is used where it is.
constexpr size_t kHpkeMinStage = 16;

int hpke_fetch_u64(prio3gpu_ctx* c, const uint64_t* p, uint64_t* out) {
  if (is_device_ptr(p)) {
    HIPCHK(hipMemcpyAsync(out, p, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  } else {
    *out = *p;
  }
  return 0;
}

// The per-report secrets of the current call that lie in the engine's own memory, and their end:
// regions of the context's scratch and host vectors.  What every GPU HPKE call keeps:
//  I1. A region is added before the copy or kernel that fills it is queued, and from then on
//      every way out of the call goes through finish(), which zeroes it on the stream: after a
//      failed launch and a failed later step too.
//  I2. A caller's own device buffer, read in place, is never added and so never written:
//      stage_secret adds a region only when the engine's buffer was used.
//  I3. finish() comes before any copy-out to the caller, so DH values, ephemeral keys and staged
//      plaintext inputs are cleared first.  Only staged output rows (prio3gpu_open_input_shares,
//      the DH test hooks) are added for a second finish() after their copy.
//  I4. With a non-zero rc the stream is synchronised before finish() returns, and rc and its
//      message stay the first error's; a failed clear on an otherwise good call is
//      PRIO3GPU_E_HIP.
struct CallSecrets {
  struct Span {
    void* p;
    size_t bytes;
  };
  // the most a call adds: four device spans (the split seal from host memory: the staged share
  // rows, the ladders' output, the staged ephemeral keys, the segments' sums) and three host
  // vectors (the request path); a call that needs more widens these
  Span dev[4];
  std::vector<uint8_t>* host[3];
  int n_dev = 0, n_host = 0;
  void add(void* p, size_t bytes) {
    assert(n_dev < 4);
    if (p && bytes) dev[n_dev++] = {p, bytes};
  }
  void add(std::vector<uint8_t>& v) {
    assert(n_host < 3);
    host[n_host++] = &v;
  }
  // Ends what was added, after the call's steps so far ended with rc; nothing is left added.
  int finish(prio3gpu_ctx* c, int rc) {
    bool cleared = true, host_read = false;
    for (int i = 0; i < n_dev; ++i)
      cleared &= hipMemsetAsync(dev[i].p, 0, dev[i].bytes, c->stream) == hipSuccess;
    if (!cleared && !rc) {
      set_err("clearing the call's per-report secrets on the device failed");
      rc = PRIO3GPU_E_HIP;
    }
    for (int i = 0; i < n_host; ++i) host_read |= !host[i]->empty();  // queued copies read them
    if (rc || host_read) (void)hipStreamSynchronize(c->stream);
    for (int i = 0; i < n_host; ++i) wipe(host[i]->data(), host[i]->size());
    n_dev = n_host = 0;
    return rc;
  }
};

// stage_in of a secret input: the engine's copy of it (none where the caller's device buffer is
// read in place, I2) is the call's to clear.
int stage_secret(prio3gpu_ctx* c, CallSecrets& sec, DevBuf& buf, const void* src, size_t bytes,
                 const uint8_t** out) {
  *out = nullptr;
  const int rc = stage_in(c, buf, src, bytes, out, kHpkeMinStage);
  if (*out && *out == buf.u8()) sec.add(buf.p, bytes);
  return rc;
}

// The open's DH scratch of n reports: 32 bytes each (X25519: the DH value; P-256: the shared
// secret), then for P-256 one validity byte each.
size_t dh_bytes(size_t n, bool p256) { return n * (p256 ? 33 : 32); }
uint8_t* dh_ok_at(void* d_dh, size_t n) { return static_cast<uint8_t*>(d_dh) + n * 32; }

// The seal ladders' output for n reports: X25519 n encapsulated keys, then n DH values, 32 bytes
// each; P-256 kP256EphBytes' layout, whose validity bytes follow the 96 n bytes of both.
size_t eph_bytes(size_t n, bool p256) { return n * (p256 ? kP256EphBytes : 64); }
uint8_t* p256_eph_ok_at(void* d_eph, size_t n) { return static_cast<uint8_t*>(d_eph) + n * 96; }

// f(i) for i in [0, n) on up to `threads` host threads (<= 0: all cores), contiguous ranges.
template <class F>
void host_parallel(size_t n, int threads, F&& f) {
  size_t t = threads > 0 ? size_t(threads) : std::max(1u, std::thread::hardware_concurrency());
  t = std::min(t, (n + 1023) / 1024);
  if (t <= 1) {
    for (size_t i = 0; i < n; ++i) f(i);
    return;
  }
  const size_t per = (n + t - 1) / t;
  std::vector<std::thread> pool;
  for (size_t k = 1; k < t; ++k)
    pool.emplace_back([&f, k, per, n] {
      for (size_t i = k * per; i < std::min(n, (k + 1) * per); ++i) f(i);
    });
  for (size_t i = 0; i < std::min(n, per); ++i) f(i);
  for (auto& th : pool) th.join();
}

// The DH step of an open under one keypair: the n packed encapsulated keys at d_points to the
// context's DH scratch (*d_dh), which is the call's secret from here on.  P-256: the shared
// secrets (raw: the x coordinates) and the validity bytes, which bc.dh_ok points at.
int open_dh(prio3gpu_ctx* c, CallSecrets& sec, uint16_t kem_id, const uint8_t* sk,
            const uint8_t* pk, HpkeBatchConsts& bc, bool raw, size_t n, const uint8_t* d_points,
            uint32_t** d_dh) {
  const bool p256 = kem_id == 0x0010;
  CHK(c->hpke.dh.ensure(dh_bytes(n, p256)));
  *d_dh = static_cast<uint32_t*>(c->hpke.dh.p);
  sec.add(*d_dh, dh_bytes(n, p256));
  if (!p256) return launch_x25519(c, sk, n, d_points, *d_dh);
  uint8_t* d_ok = dh_ok_at(*d_dh, n);
  bc.dh_ok = d_ok;
  return launch_p256_dh(c, sk, pk, bc, raw, n, d_points, *d_dh, d_ok);
}

// check_request_views (plan_hpke.h) with its message in the thread's error string.
int check_views(const Cfg& g, const prio3gpu_prepare_init_view* views, size_t n, size_t msg_len) {
  std::string err;
  const int rc = check_request_views(g, views, n, msg_len, &err);
  if (rc) set_err("%s", err.c_str());
  return rc;
}

// The context's options as plan_hpke.h's mask, and the suite check of an entry point under them:
// a wave per report (`team`) is hpke_team_suite's for opens and seals alike; a lane per report is
// hpke_gpu_suite's for an open and hpke_seal_suite's for a seal.
unsigned hpke_gpu_opts(const prio3gpu_ctx* c) {
  return (c->hpke_gpu_suites ? HPKE_OPT_SUITES : 0u) | (c->hpke_gpu_p256 ? HPKE_OPT_P256 : 0u) |
         (c->hpke_team_chacha ? HPKE_OPT_TEAM_CHACHA : 0u);
}
int suite_check(const prio3gpu_ctx* c, const char* who, bool seal, bool team, uint16_t kem,
                uint16_t kdf, uint16_t aead) {
  const unsigned o = hpke_gpu_opts(c);
  if (team ? hpke_team_suite(o, kem, kdf, aead)
           : seal ? hpke_seal_suite(o, kem, kdf, aead) : hpke_gpu_suite(o, kem, kdf, aead))
    return 0;
  set_err("%s: HPKE suite 0x%04x/%u/%u is not taken %s on this context", who, kem, kdf, aead,
          team ? "a wave per report" : "a lane per report");
  return PRIO3GPU_E_UNSUPPORTED;
}

int hpke_open_batch_impl(prio3gpu_ctx* c, uint16_t kem_id, uint16_t kdf_id, uint16_t aead_id,
                         const uint8_t* sk,
                         const uint8_t* pk, const uint8_t* info, size_t info_len, size_t n,
                         const uint8_t* encs, const uint8_t* aads, const uint64_t* aad_offsets,
                         const uint8_t* cts, const uint64_t* ct_offsets, uint8_t* pts,
                         const uint64_t* pt_offsets, uint8_t* status, bool team = false) {
  HpkeBatchConsts bc;
  if (!hpke_batch_consts(kem_id, kdf_id, aead_id, pk, info, info_len, &bc)) {
    set_err("HPKE primitives unavailable");
    return PRIO3GPU_E_UNSUPPORTED;
  }
  HIPCHK(hipSetDevice(c->device));
  uint64_t aad_total = 0, ct_total = 0, pt_total = 0, pt_first = 0;
  CHK(hpke_fetch_u64(c, aad_offsets + n, &aad_total));
  CHK(hpke_fetch_u64(c, ct_offsets + n, &ct_total));
  CHK(hpke_fetch_u64(c, pt_offsets + n, &pt_total));
  CHK(hpke_fetch_u64(c, pt_offsets, &pt_first));
  if ((aad_total && !aads) || (ct_total && !cts) || (pt_total && !pts) || pt_first > pt_total) {
    set_err("HPKE open: null data buffer or offsets out of order");
    return PRIO3GPU_E_ARG;
  }
  const uint8_t *d_enc, *d_aad, *d_aoff, *d_ct, *d_coff, *d_poff, *d_st_in;
  CHK(stage_in(c, c->hpke.enc_in, encs, n * bc.nenc, &d_enc, kHpkeMinStage));
  CHK(stage_in(c, c->hpke.aad, aads, aad_total, &d_aad, kHpkeMinStage));
  CHK(stage_in(c, c->hpke.aad_off, aad_offsets, (n + 1) * 8, &d_aoff, kHpkeMinStage));
  CHK(stage_in(c, c->hpke.ct_in, cts, ct_total, &d_ct, kHpkeMinStage));
  CHK(stage_in(c, c->hpke.ct_off, ct_offsets, (n + 1) * 8, &d_coff, kHpkeMinStage));
  CHK(stage_in(c, c->hpke.pt_off, pt_offsets, (n + 1) * 8, &d_poff, kHpkeMinStage));
  CHK(stage_in(c, c->hpke.status, status, n, &d_st_in, kHpkeMinStage));
  uint8_t* d_st = const_cast<uint8_t*>(d_st_in);
  uint8_t* d_pt = pts;
  const bool pt_host = !(pts && is_device_ptr(pts));
  if (pt_host) {
    CHK(c->hpke.pt_out.ensure(std::max<uint64_t>(pt_total, 16)));
    d_pt = c->hpke.pt_out.u8();
    if (pt_total) HIPCHK(hipMemsetAsync(d_pt, 0, pt_total, c->stream));
  }
  // the per-report secrets: the DH values (keys and nonces never leave registers)
  CallSecrets sec;
  int rc = [&]() -> int {
    uint32_t* d_dh;
    CHK(open_dh(c, sec, kem_id, sk, pk, bc, /*raw=*/false, n, d_enc, &d_dh));
    // a lane per report, or (prio3gpu_hpke_open_long_batch) a wave per report
    const PackedOpenCall q{(uint32_t)n, bc, d_dh, d_enc, d_aad,
                           reinterpret_cast<const uint64_t*>(d_aoff), aad_total, d_ct,
                           reinterpret_cast<const uint64_t*>(d_coff), ct_total, d_pt,
                           reinterpret_cast<const uint64_t*>(d_poff), pt_total, d_st};
    return team ? launch_hpke_open_team(c, q) : launch_hpke_open(c, q);
  }();
  CHK(sec.finish(c, rc));
  if (pt_host && pt_total > pt_first)
    HIPCHK(hipMemcpyAsync(pts + pt_first, d_pt + pt_first, pt_total - pt_first,
                          hipMemcpyDeviceToHost, c->stream));
  if (d_st != status) HIPCHK(hipMemcpyAsync(status, d_st, n, hipMemcpyDeviceToHost, c->stream));
  return finish_call(c, {encs, aads, aad_offsets, cts, ct_offsets, pts, pt_offsets, status});
}

// The key check of an open entry point: a 32-byte private key, an Npk-byte public key, and for
// P-256 a keypair (a scalar outside [1, n) fails the host's open of every report with this code;
// a public key that is no point can have sealed nothing).
int open_key_check(const char* who, uint16_t kem_id, const uint8_t* sk, size_t sk_len,
                   const uint8_t* pk, size_t pk_len) {
  const size_t npk = hpke_kem_nenc(kem_id);
  if (!sk || sk_len != 32 || !pk || pk_len != npk) {
    set_err("%s: the private key is 32 bytes, the public key %zu", who, npk);
    return PRIO3GPU_E_ARG;
  }
  if (kem_id == 0x0010 && !p256_keypair_valid(sk, sk_len, pk, pk_len)) {
    set_err("%s: not a P-256 keypair", who);
    return PRIO3GPU_E_HPKE;
  }
  return 0;
}

// prio3gpu_hpke_open_batch and, with `team`, prio3gpu_hpke_open_long_batch.
int hpke_open_batch_entry(prio3gpu_ctx* c, uint16_t kem_id, uint16_t kdf_id, uint16_t aead_id,
                          const uint8_t* sk, size_t sk_len, const uint8_t* pk, size_t pk_len,
                          const uint8_t* info, size_t info_len, size_t n, const uint8_t* encs,
                          const uint8_t* aads, const uint64_t* aad_offsets, const uint8_t* cts,
                          const uint64_t* ct_offsets, uint8_t* pts, const uint64_t* pt_offsets,
                          uint8_t* status, bool team) {
  if (!c) {
    set_err("null context");
    return PRIO3GPU_E_ARG;
  }
  CHK(suite_check(c, "HPKE open", /*seal=*/false, team, kem_id, kdf_id, aead_id));
  if (info_len && !info) {  // with the key lengths: before the keypair's check
    set_err("HPKE open: null info");
    return PRIO3GPU_E_ARG;
  }
  CHK(open_key_check("HPKE open", kem_id, sk, sk_len, pk, pk_len));
  if (n == 0) return 0;
  if (!encs || !aad_offsets || !ct_offsets || !pt_offsets || !status || n > 0x7FFFFFFFu) {
    set_err("HPKE open: null argument");
    return PRIO3GPU_E_ARG;
  }
  return hpke_open_batch_impl(c, kem_id, kdf_id, aead_id, sk, pk, info, info_len, n, encs, aads,
                              aad_offsets, cts, ct_offsets, pts, pt_offsets, status, team);
}

// The packed inputs and outputs of one key group's batch, reused from group to group.
struct HpkeGroupBufs {
  std::vector<uint8_t> encs, aads, cts, pts, st;
  std::vector<uint64_t> aoff, coff, poff;
};

// One key group of prio3gpu_hpke_open_report_shares_gpu: pack its reports' fields, open them on
// the GPU, unpack.  An opened report gets its plaintext; a failed one the second trial on the host
// (st_retry 0) or its status.  The packed plaintexts are wiped on every way out.
int open_group_packed(prio3gpu_ctx* c, const HpkePlan& plan, size_t k, const uint8_t info[20],
                      const uint8_t* task_id, const uint8_t* msg,
                      const prio3gpu_prepare_init_view* views, int threads, HpkeGroupBufs& b,
                      uint8_t* plaintexts, const uint64_t* offsets, uint8_t* status,
                      uint8_t* st_retry, bool* any_retry) {
  struct WipeAtExit {
    std::vector<uint8_t>& v;
    ~WipeAtExit() { wipe(v.data(), v.size()); }
  } wipe_pts{b.pts};
  const prio3gpu_hpke_keypair* kp = plan.groups[k];
  const uint32_t* idx = plan.idx.data() + plan.gbeg[k];
  const size_t m = plan.gbeg[k + 1] - plan.gbeg[k];
  b.aoff.assign(m + 1, 0), b.coff.assign(m + 1, 0), b.poff.assign(m + 1, 0);
  for (size_t j = 0; j < m; ++j) {
    const prio3gpu_prepare_init_view& v = views[idx[j]];
    b.aoff[j + 1] = b.aoff[j] + 60 + v.public_share_len;  // InputShareAad
    b.coff[j + 1] = b.coff[j] + v.payload_len;
    b.poff[j + 1] = b.poff[j] + (v.payload_len - 16);
  }
  const size_t nenc = hpke_kem_nenc(kp->kem_id);  // every member's enc_len (strict plan)
  b.encs.resize(m * nenc), b.aads.resize(b.aoff[m]), b.cts.resize(b.coff[m]);
  // the fields of one report lie kilobytes apart in the request (its prep share is between
  // them): the gather is DRAM-latency-bound on one thread, so it runs on the host threads
  host_parallel(m, threads, [&](size_t j) {
    const prio3gpu_prepare_init_view& v = views[idx[j]];
    memcpy(&b.encs[j * nenc], msg + v.enc_off, nenc);
    uint8_t* a = &b.aads[b.aoff[j]];  // task id, report id, time, u32-prefixed public share
    memcpy(a, task_id, 32);
    memcpy(a + 32, msg + v.report_id_off, 16);
    for (int s = 0; s < 8; ++s) a[48 + s] = uint8_t(v.time >> (56 - 8 * s));
    for (int s = 0; s < 4; ++s) a[56 + s] = uint8_t(v.public_share_len >> (24 - 8 * s));
    memcpy(a + 60, msg + v.public_share_off, v.public_share_len);
    memcpy(&b.cts[b.coff[j]], msg + v.payload_off, v.payload_len);
  });
  b.pts.assign(std::max<size_t>(b.poff.back(), 1), 0);
  b.st.assign(m, 0);
  CHK(hpke_open_batch_impl(c, kp->kem_id, kp->kdf_id, kp->aead_id, kp->private_key,
                           kp->public_key, info, 20,
                           m, b.encs.data(), b.aads.data(), b.aoff.data(), b.cts.data(),
                           b.coff.data(), b.pts.data(), b.poff.data(), b.st.data()));
  for (size_t j = 0; j < m; ++j) {
    const size_t i = idx[j];
    if (b.st[j] == 0) {
      memcpy(plaintexts + offsets[i], b.pts.data() + b.poff[j], b.poff[j + 1] - b.poff[j]);
    } else if (wants_global_retry(plan, views, i)) {
      st_retry[i] = 0;
      *any_retry = true;
    } else {
      status[i] = PRIO3GPU_HPKE_DECRYPT_ERROR;
    }
  }
  return 0;
}

// ---- prio3gpu_helper_init_request, step by step -------------------------------------------------
// One call's arguments, plan and buffers.
struct ReqCall {
  prio3gpu_ctx* c;
  prio3gpu_state* st;
  const uint8_t* task_id;
  uint8_t sender_role, recipient_role;
  const uint8_t* msg;
  size_t msg_len;
  const prio3gpu_prepare_init_view* views;
  size_t n;
  int threads;
  HpkePlan plan;                     // request mode (plan_hpke.h)
  std::vector<uint64_t> poff;        // plaintext_offsets
  std::vector<uint8_t> dst;          // the device status image on the host
  std::vector<HpkeBatchConsts> bcs;  // per group
  ReqTaskId tid;
  size_t in_pitch;
  const uint8_t* d_msg;
  const ReqView* d_views;
  const uint32_t* d_idx;
  uint32_t* d_dh;
  uint8_t* d_pts;
  const uint64_t* d_poff;
  uint8_t *d_faults, *d_status, *d_in;
  std::vector<uint8_t> hp, hin, fb;  // host fallback: plaintexts, decoded rows, packed upload
  // the per-report secrets outside the engine's rows: the DH values and the plaintexts on the
  // device, the fallback's vectors on the host (ended after steps 3 to 6)
  CallSecrets sec;
};

// 1. Who opens which report, the status image the kernels start from, each group's constants.
int req_plan(ReqCall& q, const prio3gpu_hpke_keypair* task_keys, size_t n_task_keys,
             const prio3gpu_hpke_keypair* global_keys, size_t n_global_keys,
             const uint8_t* status) {
  q.poff.resize(q.n + 1);
  plaintext_offsets(q.views, q.n, q.poff.data());
  plan_hpke(task_keys, n_task_keys, global_keys, n_global_keys, q.views, status, q.n,
            hpke_gpu_opts(q.c), /*strict=*/false, &q.plan);
  q.dst.resize(q.n);
  request_status_image(q.plan, status, q.n, q.dst.data());
  uint8_t info[20];
  input_share_info(q.sender_role, q.recipient_role, info);
  q.bcs.resize(q.plan.groups.size());
  for (size_t k = 0; k < q.bcs.size(); ++k) {
    const prio3gpu_hpke_keypair* kp = q.plan.groups[k];
    if (!hpke_batch_consts(kp->kem_id, kp->kdf_id, kp->aead_id, kp->public_key, info,
                           sizeof info, &q.bcs[k])) {
      set_err("HPKE primitives unavailable");
      return PRIO3GPU_E_UNSUPPORTED;
    }
  }
  memcpy(q.tid.w, q.task_id, 32);  // little-endian host: byte j at bits 8 (j & 3) of word j >> 2
  return 0;
}

// 2. The staged buffers; the message goes to the device here (or is used where it is).
int req_reserve(ReqCall& q) {
  prio3gpu_ctx* c = q.c;
  prio3gpu_state* st = q.st;
  const Cfg& g = c->cfg;
  const size_t n = q.n;
  HIPCHK(hipSetDevice(c->device));
  q.in_pitch = input_pitch(st);
  CHK(c->req.views.ensure(n * sizeof(ReqView)));
  CHK(c->req.group_idx.ensure(std::max<size_t>(q.plan.idx.size(), 1) * 4));
  CHK(c->req.dh.ensure(dh_bytes(n, /*p256=*/true)));  // a group of either KEM fits
  CHK(c->req.pt.ensure(std::max<uint64_t>(q.poff[n], 16)));
  CHK(c->req.pt_off.ensure((n + 1) * 8));
  CHK(c->req.faults.ensure(n));
  CHK(st->status.ensure(n));
  CHK(st->nonces.ensure(n * 16));
  CHK(st->pub.ensure(std::max<size_t>(n * g.public_share_len, 16)));
  CHK(st->input.ensure((n - 1) * q.in_pitch + g.helper_share_len));
  CHK(c->io[0].ensure(std::max<size_t>(n * g.prep_share_len, 16)));
  {
    PROF(KID_REQ_COPY);
    CHK(stage_in(c, c->req.msg, q.msg, q.msg_len, &q.d_msg, 16));
  }
  q.d_views = static_cast<const ReqView*>(c->req.views.p);
  q.d_idx = static_cast<const uint32_t*>(c->req.group_idx.p);
  q.d_dh = static_cast<uint32_t*>(c->req.dh.p);
  q.d_pts = c->req.pt.u8();
  q.d_poff = static_cast<const uint64_t*>(c->req.pt_off.p);
  q.d_faults = c->req.faults.u8();
  q.d_status = st->status.u8();
  q.d_in = st->input.u8();
  q.sec.add(q.d_dh, dh_bytes(n, /*p256=*/true));
  q.sec.add(q.d_pts, q.poff[n]);
  q.sec.add(q.hp), q.sec.add(q.hin), q.sec.add(q.fb);
  return 0;
}

// 3. Views, group members, plaintext offsets and the status image up; nonces, public shares and
// leader prep shares gathered into the engine's rows.
int req_upload_gather(ReqCall& q) {
  prio3gpu_ctx* c = q.c;
  const size_t n = q.n;
  const std::vector<uint32_t>& idx = q.plan.idx;
  HIPCHK(hipMemcpyAsync(c->req.views.p, q.views, n * sizeof(ReqView), hipMemcpyHostToDevice,
                        c->stream));
  if (!idx.empty())
    HIPCHK(hipMemcpyAsync(c->req.group_idx.p, idx.data(), idx.size() * 4, hipMemcpyHostToDevice,
                          c->stream));
  HIPCHK(hipMemcpyAsync(c->req.pt_off.p, q.poff.data(), (n + 1) * 8, hipMemcpyHostToDevice,
                        c->stream));
  HIPCHK(hipMemcpyAsync(q.d_status, q.dst.data(), n, hipMemcpyHostToDevice, c->stream));
  return launch_req_gather(c, n, q.d_msg, q.msg_len, q.d_views, q.st->nonces.u8(), q.st->pub.u8(),
                           c->io[0].u8(), q.d_faults);
}

// 4. Per key group: the DH values, then the open into d_pts / d_status.
int req_open_groups(ReqCall& q) {
  for (size_t k = 0; k < q.plan.groups.size(); ++k) {
    const size_t m = q.plan.gbeg[k + 1] - q.plan.gbeg[k];
    const uint32_t* d_idx = q.d_idx + q.plan.gbeg[k];
    const prio3gpu_hpke_keypair* kp = q.plan.groups[k];
    if (kp->kem_id == 0x0010) {
      uint8_t* d_ok = dh_ok_at(q.d_dh, q.n);
      q.bcs[k].dh_ok = d_ok;
      CHK(launch_p256_dh_idx(q.c, kp->private_key, kp->public_key, q.bcs[k], m, d_idx, q.d_msg,
                             q.d_views, q.d_dh, d_ok));
    } else {
      CHK(launch_x25519_idx(q.c, kp->private_key, m, d_idx, q.d_msg, q.d_views, q.d_dh));
    }
    CHK(launch_hpke_open_req(q.c, q.bcs[k], q.tid, m, d_idx, q.d_dh, q.d_msg, q.d_views, q.d_pts,
                             q.d_poff, q.d_status));
  }
  return 0;
}

// 5. Plaintexts to input-share rows; the status image comes back for the host's classification.
int req_decode(ReqCall& q) {
  prio3gpu_ctx* c = q.c;
  CHK(launch_decode_plaintext_input_shares(c, q.n, q.d_pts, q.d_poff, c->cfg.helper_share_len,
                                           q.d_in, q.in_pitch, q.d_faults, q.d_status));
  HIPCHK(hipMemcpyAsync(q.dst.data(), q.d_status, q.n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// 6a. The fallback reports opened and decoded on the host: q.hp, q.hin and their statuses.
int req_host_open(ReqCall& q, const HpkeFallback& f, std::vector<uint8_t>& st_fb) {
  prio3gpu_ctx* c = q.c;
  const HpkePlan& p = q.plan;
  const size_t n = q.n;
  std::vector<uint8_t> host_msg;
  const uint8_t* h_msg = q.msg;
  if (is_device_ptr(q.msg)) {
    host_msg.resize(q.msg_len);
    HIPCHK(hipMemcpyAsync(host_msg.data(), q.msg, q.msg_len, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    h_msg = host_msg.data();
  }
  q.hp.assign(std::max<uint64_t>(q.poff[n], 1), 0);
  std::vector<uint64_t> offs(n + 1);
  st_fb.assign(n, 1);
  if (f.n_host) {
    st_fb = f.st_host;
    CHK(prio3gpu_hpke_open_report_shares(q.task_id, p.task_keys, p.n_task_keys, p.global_keys,
                                         p.n_global_keys, q.sender_role, q.recipient_role, h_msg,
                                         q.views, n, q.hp.data(), offs.data(), st_fb.data(),
                                         q.threads));
  }
  if (f.n_retry) {
    std::vector<uint8_t> s2(f.st_retry);
    CHK(prio3gpu_hpke_open_report_shares(q.task_id, nullptr, 0, p.global_keys, p.n_global_keys,
                                         q.sender_role, q.recipient_role, h_msg, q.views, n,
                                         q.hp.data(), offs.data(), s2.data(), q.threads));
    for (size_t i = 0; i < n; ++i)
      if (!f.st_retry[i]) st_fb[i] = s2[i];
  }
  q.hin.assign(n * (size_t)c->cfg.helper_share_len, 0);
  return prio3gpu_decode_plaintext_input_shares(&c->sz, q.hp.data(), offs.data(), n, 1,
                                                q.hin.data(), st_fb.data());
}

// 6. The host's share (classify_fallback, plan_hpke.h): opened and decoded on the host, packed
// into one upload, scattered into the rows and the status image.
int req_host_fallback(ReqCall& q) {
  prio3gpu_ctx* c = q.c;
  const uint32_t want = c->cfg.helper_share_len;
  HpkeFallback f;
  classify_fallback(q.plan, q.views, q.dst.data(), q.n, &f);
  if (f.n_host + f.n_retry == 0) return 0;
  std::vector<uint8_t> st_fb;
  CHK(req_host_open(q, f, st_fb));
  const FallbackLayout l = pack_fallback(f, q.n, q.hin.data(), st_fb.data(), want, &q.fb);
  CHK(c->req.fallback.ensure(l.bytes));
  uint8_t* d_fb = c->req.fallback.u8();
  HIPCHK(hipMemcpyAsync(d_fb, q.fb.data(), l.bytes, hipMemcpyHostToDevice, c->stream));
  CHK(launch_req_scatter(c, l.kf, reinterpret_cast<const uint32_t*>(d_fb), d_fb + l.o_rows,
                         d_fb + l.o_st, want, q.d_in, q.in_pitch, q.d_faults, q.d_status));
  HIPCHK(hipMemsetAsync(d_fb, 0, l.bytes, c->stream));  // input shares are secrets too
  return 0;
}

// ---- batched HPKE seal on the GPU (hpke_seal_gpu.h) ---------------------------------------------
// The recipient's public key of a seal entry point: 32 bytes for X25519; for P-256 the 65 bytes
// of a point DeserializePublicKey takes (p256.h's decoder), checked before anything is launched.
int seal_pk_check(uint16_t kem_id, const uint8_t* pk, size_t pk_len) {
  if (!pk || pk_len != hpke_kem_nenc(kem_id)) {
    set_err("HPKE seal: the public key is %u bytes", hpke_kem_nenc(kem_id));
    return PRIO3GPU_E_ARG;
  }
  if (kem_id == 0x0010) {
    uint32_t x[8], y[8];
    Fp256 X, Y;
    if (!p256_decode(pk, x, y, X, Y)) {
      set_err("HPKE seal: the public key is not a P-256 point");
      return PRIO3GPU_E_HPKE;
    }
  }
  return 0;
}

// Stage the n ephemeral keys and run both ladders of every report into the context's eph scratch
// (*d_eph), both the call's secrets from here on.  Under P-256 the KEM half follows
// (k_p256_eph_kem) and bc.dh_ok is set to the validity bytes.
int seal_ladders(prio3gpu_ctx* c, CallSecrets& sec, HpkeBatchConsts& bc, const uint8_t* pk,
                 size_t n, const uint8_t* sk_es, uint32_t** d_eph) {
  const bool p256 = bc.kem_lo == 0x10;
  CHK(c->seal.eph.ensure(eph_bytes(n, p256)));
  uint32_t* eph = *d_eph = static_cast<uint32_t*>(c->seal.eph.p);
  sec.add(eph, eph_bytes(n, p256));
  const uint8_t* d_sk;
  CHK(stage_secret(c, sec, c->seal.eph_sk, sk_es, n * 32, &d_sk));
  if (p256) {
    uint8_t* d_ok = p256_eph_ok_at(eph, n);
    bc.dh_ok = d_ok;
    CHK(launch_p256_eph(c, pk, n, d_sk, eph, d_ok));
    return launch_p256_eph_kem(c, pk, bc, n, eph, d_ok);
  }
  return launch_x25519_eph(c, pk, n, d_sk, eph);
}

// Where a seal writes an output of `bytes` bytes: the caller's buffer when it is device memory,
// else staging (zeroed, so what no lane writes reads as zero).
int seal_out(prio3gpu_ctx* c, DevBuf& buf, uint8_t* dst, size_t bytes, uint8_t** d_out) {
  if (dst && is_device_ptr(dst)) {
    *d_out = dst;
    return 0;
  }
  CHK(buf.ensure(std::max<size_t>(bytes, kHpkeMinStage)));
  *d_out = buf.u8();
  if (bytes) HIPCHK(hipMemsetAsync(*d_out, 0, bytes, c->stream));
  return 0;
}

// prio3gpu_hpke_seal_batch and, with `team`, prio3gpu_hpke_seal_long_batch.
int hpke_seal_batch_entry(prio3gpu_ctx* c, uint16_t kem_id, uint16_t kdf_id, uint16_t aead_id,
                          const uint8_t* pk, size_t pk_len, const uint8_t* info, size_t info_len,
                          size_t n, const uint8_t* sk_es, const uint8_t* aads,
                          const uint64_t* aad_offsets, const uint8_t* pts,
                          const uint64_t* pt_offsets, uint8_t* encs, uint8_t* cts,
                          const uint64_t* ct_offsets, uint8_t* status, bool team) {
  if (!c) {
    set_err("null context");
    return PRIO3GPU_E_ARG;
  }
  CHK(suite_check(c, "HPKE seal", /*seal=*/true, team, kem_id, kdf_id, aead_id));
  CHK(seal_pk_check(kem_id, pk, pk_len));
  if (info_len && !info) {
    set_err("HPKE seal: null info");
    return PRIO3GPU_E_ARG;
  }
  if (n == 0) return 0;
  if (!sk_es || !aad_offsets || !pt_offsets || !encs || !ct_offsets || !status ||
      n > 0x7FFFFFFFu) {
    set_err("HPKE seal: null argument");
    return PRIO3GPU_E_ARG;
  }
  HpkeBatchConsts bc;
  if (!hpke_batch_consts(kem_id, kdf_id, aead_id, pk, info, info_len, &bc)) {
    set_err("HPKE primitives unavailable");
    return PRIO3GPU_E_UNSUPPORTED;
  }
  HIPCHK(hipSetDevice(c->device));
  uint64_t aad_total = 0, pt_total = 0, ct_total = 0, ct_first = 0;
  CHK(hpke_fetch_u64(c, aad_offsets + n, &aad_total));
  CHK(hpke_fetch_u64(c, pt_offsets + n, &pt_total));
  CHK(hpke_fetch_u64(c, ct_offsets + n, &ct_total));
  CHK(hpke_fetch_u64(c, ct_offsets, &ct_first));
  if ((aad_total && !aads) || (pt_total && !pts) || (ct_total && !cts) || ct_first > ct_total) {
    set_err("HPKE seal: null data buffer or offsets out of order");
    return PRIO3GPU_E_ARG;
  }
  // the per-report secrets: the engine's copies of the ephemeral keys and of the plaintexts, and
  // the ladders' output
  CallSecrets sec;
  uint8_t *d_enc = nullptr, *d_ct = nullptr, *d_st = nullptr;
  int rc = [&]() -> int {
    const uint8_t *d_aad, *d_aoff, *d_poff, *d_coff, *d_st_in, *d_pt;
    uint32_t* d_eph;
    CHK(stage_in(c, c->hpke.aad, aads, aad_total, &d_aad, kHpkeMinStage));
    CHK(stage_in(c, c->hpke.aad_off, aad_offsets, (n + 1) * 8, &d_aoff, kHpkeMinStage));
    CHK(stage_in(c, c->seal.pt_off, pt_offsets, (n + 1) * 8, &d_poff, kHpkeMinStage));
    CHK(stage_in(c, c->hpke.ct_off, ct_offsets, (n + 1) * 8, &d_coff, kHpkeMinStage));
    CHK(stage_in(c, c->hpke.status, status, n, &d_st_in, kHpkeMinStage));
    d_st = const_cast<uint8_t*>(d_st_in);
    CHK(seal_out(c, c->seal.enc_packed, encs, n * bc.nenc, &d_enc));
    CHK(seal_out(c, c->seal.ct_out, cts, ct_total, &d_ct));
    CHK(stage_secret(c, sec, c->seal.pt_in, pts, pt_total, &d_pt));
    CHK(seal_ladders(c, sec, bc, pk, n, sk_es, &d_eph));
    // a lane per report, or (prio3gpu_hpke_seal_long_batch) a wave per report
    const PackedSealCall q{(uint32_t)n, bc, d_eph, d_aad,
                           reinterpret_cast<const uint64_t*>(d_aoff), aad_total, d_pt,
                           reinterpret_cast<const uint64_t*>(d_poff), pt_total, d_enc, d_ct,
                           reinterpret_cast<const uint64_t*>(d_coff), ct_total, d_st};
    return team ? launch_hpke_seal_team(c, q) : launch_hpke_seal(c, q);
  }();
  CHK(sec.finish(c, rc));
  CHK(copy_out(c, encs, d_enc, n * bc.nenc));
  if (d_ct != cts && ct_total > ct_first)
    HIPCHK(hipMemcpyAsync(cts + ct_first, d_ct + ct_first, ct_total - ct_first,
                          hipMemcpyDeviceToHost, c->stream));
  CHK(copy_out(c, status, d_st, n));
  return finish_call(c, {sk_es, aads, aad_offsets, pts, pt_offsets, encs, cts, ct_offsets, status});
}

// `rows` rows of `width` bytes from packed device rows (a seal's encs and payloads, an open's
// shares) to the caller's host rows `pitch` apart, through host memory: only the rows' own bytes
// are written.
int packed_rows_to_host(prio3gpu_ctx* c, uint8_t* dst, size_t pitch, const uint8_t* d_src,
                        size_t width, size_t rows) {
  if (pitch == width) {
    HIPCHK(hipMemcpyAsync(dst, d_src, rows * width, hipMemcpyDeviceToHost, c->stream));
    return 0;
  }
  std::vector<uint8_t> tmp(rows * width);
  HIPCHK(hipMemcpyAsync(tmp.data(), d_src, tmp.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < rows; ++i) memcpy(dst + i * pitch, tmp.data() + i * width, width);
  return 0;
}

// How a share-row call cuts its reports ("hpke_team_split", "hpke_team_split_blocks"): S = 1 means
// the one-wave kernels and nothing else.  Every report of the call has the same body.  A batch
// beyond the wipe kernel's grid (one y per report) could not split anyway: it fills the chip.
TeamSplit share_split(const prio3gpu_ctx* c, size_t n, uint32_t input_share_len,
                      uint16_t aead_id) {
  const uint64_t body = 6 + (uint64_t)input_share_len;
  if (c->hpke_team_split < 2 || n > 65535) return {1, (body + 15) / 16};
  return team_split_plan(n, body, aead_id == 3 ? 4 * kTeam : kTeam, c->hpke_team_split,
                         c->hpke_team_split_blocks,
                         (uint64_t)c->cus * 4 * split_waves_per_simd(aead_id));
}

// What a split call's kernels share (hpke_launch.h's SplitShareCall), with the call's scratch: the
// segments' sums and the header flags, the call's secret from here on.
int split_call(prio3gpu_ctx* c, CallSecrets& sec, const TeamSplit& sp, size_t n,
               const HpkeBatchConsts& bc, const ReqTaskId& tid, const uint8_t* d_rid,
               const uint8_t* d_time, const uint8_t* d_pub, uint32_t public_share_len,
               uint32_t input_share_len, uint8_t* d_st, SplitShareCall* q) {
  const size_t bytes = split_scratch_bytes(n, sp.S);
  CHK(c->hpke.split.ensure(bytes));
  sec.add(c->hpke.split.p, bytes);
  *q = SplitShareCall{(uint32_t)n, sp.S, sp.L, bc, tid, d_rid,
                      reinterpret_cast<const uint64_t*>(d_time), d_pub, public_share_len,
                      input_share_len, c->hpke.split.u8(), d_st};
  return 0;
}

// prio3gpu_seal_input_shares and, with `team`, prio3gpu_seal_input_shares_long.
int seal_input_shares_entry(prio3gpu_ctx* c, const uint8_t* task_id, uint16_t kem_id,
                            uint16_t kdf_id, uint16_t aead_id, const uint8_t* pk, size_t pk_len,
                            uint8_t recipient_role, size_t n, const uint8_t* report_ids,
                            const uint64_t* times, const uint8_t* public_shares,
                            uint32_t public_share_len, const uint8_t* input_shares,
                            uint32_t input_share_len, size_t input_share_pitch,
                            const uint8_t* sk_es, uint8_t* out_encs, size_t enc_pitch,
                            uint8_t* out_payloads, size_t payload_pitch, uint8_t* status,
                            bool team) {
  if (!c) {
    set_err("null context");
    return PRIO3GPU_E_ARG;
  }
  CHK(suite_check(c, "seal_input_shares", /*seal=*/true, team, kem_id, kdf_id, aead_id));
  CHK(seal_pk_check(kem_id, pk, pk_len));
  if (!task_id) {
    set_err("seal_input_shares: null task id");
    return PRIO3GPU_E_ARG;
  }
  if (n == 0) return 0;
  if (!report_ids || !times || (public_share_len && !public_shares) ||
      (input_share_len && !input_shares) || !sk_es || !out_encs || !out_payloads || !status ||
      n > 0x7FFFFFFFu) {
    set_err("seal_input_shares: null argument");
    return PRIO3GPU_E_ARG;
  }
  const ShareColumns g =
      share_columns(kem_id, input_share_len, enc_pitch, payload_pitch, input_share_pitch);
  if (!g.ok()) {
    set_err("seal_input_shares: a pitch is shorter than its row");
    return PRIO3GPU_E_ARG;
  }
  const size_t nenc = g.nenc, plen = g.plen;
  const size_t spitch = g.share_pitch, epitch = g.enc_pitch, ppitch = g.payload_pitch;
  uint8_t info[20];
  input_share_info(/*ROLE_CLIENT*/ 1, recipient_role, info);
  HpkeBatchConsts bc;
  if (!hpke_batch_consts(kem_id, kdf_id, aead_id, pk, info, sizeof info, &bc)) {
    set_err("HPKE primitives unavailable");
    return PRIO3GPU_E_UNSUPPORTED;
  }
  ReqTaskId tid;
  memcpy(tid.w, task_id, 32);  // little-endian host: byte j at bits 8 (j & 3) of word j >> 2
  HIPCHK(hipSetDevice(c->device));
  // the per-report secrets: the engine's copies of the ephemeral keys and of the share rows, and
  // the ladders' output
  CallSecrets sec;
  // host outputs are sealed into packed staging rows, device outputs in place at their pitches
  const bool enc_host = !is_device_ptr(out_encs), pay_host = !is_device_ptr(out_payloads);
  uint8_t *d_enc = nullptr, *d_pay = nullptr, *d_st = nullptr;
  int rc = [&]() -> int {
    const uint8_t *d_rid, *d_time, *d_pub, *d_st_in, *d_sh;
    uint32_t* d_eph;
    CHK(stage_in(c, c->seal.rid, report_ids, n * 16, &d_rid, kHpkeMinStage));
    CHK(stage_in(c, c->seal.time, times, n * 8, &d_time, kHpkeMinStage));
    CHK(stage_in(c, c->seal.pub, public_shares, n * (size_t)public_share_len, &d_pub,
                 kHpkeMinStage));
    CHK(stage_in(c, c->hpke.status, status, n, &d_st_in, kHpkeMinStage));
    d_st = const_cast<uint8_t*>(d_st_in);
    CHK(seal_out(c, c->seal.enc_packed, enc_host ? nullptr : out_encs, n * nenc, &d_enc));
    CHK(seal_out(c, c->seal.ct_out, pay_host ? nullptr : out_payloads, n * plen, &d_pay));
    CHK(stage_secret(c, sec, c->seal.pt_in, input_shares,
                     rows_span(n, spitch, input_share_len), &d_sh));
    CHK(seal_ladders(c, sec, bc, pk, n, sk_es, &d_eph));
    // a lane per report, or (prio3gpu_seal_input_shares_long) a wave per report
    const TeamSplit sp = team ? share_split(c, n, input_share_len, aead_id)
                              : TeamSplit{1, 0};
    if (sp.S >= 2) {  // several waves per report: the segments, then the tags and encs
      SplitShareCall q;
      CHK(split_call(c, sec, sp, n, bc, tid, d_rid, d_time, d_pub, public_share_len,
                     input_share_len, d_st, &q));
      return launch_seal_team_split(c, q, d_eph, d_sh, spitch, d_enc, enc_host ? nenc : epitch,
                                    d_pay, pay_host ? plen : ppitch);
    }
    const ShareSealCall q{(uint32_t)n, bc, tid, d_eph, d_rid,
                          reinterpret_cast<const uint64_t*>(d_time), d_pub, public_share_len,
                          d_sh, input_share_len, (uint64_t)spitch, d_enc,
                          (uint64_t)(enc_host ? nenc : epitch), d_pay,
                          (uint64_t)(pay_host ? plen : ppitch), d_st};
    return team ? launch_hpke_seal_team_shares(c, q) : launch_hpke_seal_shares(c, q);
  }();
  CHK(sec.finish(c, rc));
  if (enc_host) CHK(packed_rows_to_host(c, out_encs, epitch, d_enc, nenc, n));
  if (pay_host) CHK(packed_rows_to_host(c, out_payloads, ppitch, d_pay, plen, n));
  CHK(copy_out(c, status, d_st, n));
  return finish_call(c, {report_ids, times, public_shares, input_shares, sk_es, out_encs,
                         out_payloads, status});
}

}  // namespace

extern "C" {

int prio3gpu_hpke_seal_batch(prio3gpu_ctx* c, uint16_t kem_id, uint16_t kdf_id, uint16_t aead_id,
                             const uint8_t* pk, size_t pk_len, const uint8_t* info,
                             size_t info_len, size_t n, const uint8_t* sk_es, const uint8_t* aads,
                             const uint64_t* aad_offsets, const uint8_t* pts,
                             const uint64_t* pt_offsets, uint8_t* encs, uint8_t* cts,
                             const uint64_t* ct_offsets, uint8_t* status) {
  return hpke_seal_batch_entry(c, kem_id, kdf_id, aead_id, pk, pk_len, info, info_len, n, sk_es,
                               aads, aad_offsets, pts, pt_offsets, encs, cts, ct_offsets, status,
                               /*team=*/false);
}

int prio3gpu_hpke_seal_long_batch(prio3gpu_ctx* c, uint16_t kem_id, uint16_t kdf_id,
                                  uint16_t aead_id, const uint8_t* pk, size_t pk_len,
                                  const uint8_t* info, size_t info_len, size_t n,
                                  const uint8_t* sk_es, const uint8_t* aads,
                                  const uint64_t* aad_offsets, const uint8_t* pts,
                                  const uint64_t* pt_offsets, uint8_t* encs, uint8_t* cts,
                                  const uint64_t* ct_offsets, uint8_t* status) {
  return hpke_seal_batch_entry(c, kem_id, kdf_id, aead_id, pk, pk_len, info, info_len, n, sk_es,
                               aads, aad_offsets, pts, pt_offsets, encs, cts, ct_offsets, status,
                               /*team=*/true);
}

int prio3gpu_seal_input_shares(prio3gpu_ctx* c, const uint8_t* task_id, uint16_t kem_id,
                               uint16_t kdf_id, uint16_t aead_id, const uint8_t* pk,
                               size_t pk_len, uint8_t recipient_role, size_t n,
                               const uint8_t* report_ids, const uint64_t* times,
                               const uint8_t* public_shares, uint32_t public_share_len,
                               const uint8_t* input_shares, uint32_t input_share_len,
                               size_t input_share_pitch, const uint8_t* sk_es, uint8_t* out_encs,
                               size_t enc_pitch, uint8_t* out_payloads, size_t payload_pitch,
                               uint8_t* status) {
  return seal_input_shares_entry(c, task_id, kem_id, kdf_id, aead_id, pk, pk_len, recipient_role,
                                 n, report_ids, times, public_shares, public_share_len,
                                 input_shares, input_share_len, input_share_pitch, sk_es, out_encs,
                                 enc_pitch, out_payloads, payload_pitch, status, /*team=*/false);
}

int prio3gpu_seal_input_shares_long(prio3gpu_ctx* c, const uint8_t* task_id, uint16_t kem_id,
                                    uint16_t kdf_id, uint16_t aead_id, const uint8_t* pk,
                                    size_t pk_len, uint8_t recipient_role, size_t n,
                                    const uint8_t* report_ids, const uint64_t* times,
                                    const uint8_t* public_shares, uint32_t public_share_len,
                                    const uint8_t* input_shares, uint32_t input_share_len,
                                    size_t input_share_pitch, const uint8_t* sk_es,
                                    uint8_t* out_encs, size_t enc_pitch, uint8_t* out_payloads,
                                    size_t payload_pitch, uint8_t* status) {
  return seal_input_shares_entry(c, task_id, kem_id, kdf_id, aead_id, pk, pk_len, recipient_role,
                                 n, report_ids, times, public_shares, public_share_len,
                                 input_shares, input_share_len, input_share_pitch, sk_es, out_encs,
                                 enc_pitch, out_payloads, payload_pitch, status, /*team=*/true);
}

int prio3gpu_hpke_open_batch(prio3gpu_ctx* c, uint16_t kem_id, uint16_t kdf_id, uint16_t aead_id,
                             const uint8_t* sk, size_t sk_len, const uint8_t* pk, size_t pk_len,
                             const uint8_t* info, size_t info_len, size_t n, const uint8_t* encs,
                             const uint8_t* aads, const uint64_t* aad_offsets, const uint8_t* cts,
                             const uint64_t* ct_offsets, uint8_t* pts, const uint64_t* pt_offsets,
                             uint8_t* status) {
  return hpke_open_batch_entry(c, kem_id, kdf_id, aead_id, sk, sk_len, pk, pk_len, info, info_len,
                               n, encs, aads, aad_offsets, cts, ct_offsets, pts, pt_offsets,
                               status, /*team=*/false);
}

int prio3gpu_hpke_open_long_batch(prio3gpu_ctx* c, uint16_t kem_id, uint16_t kdf_id,
                                  uint16_t aead_id, const uint8_t* sk, size_t sk_len,
                                  const uint8_t* pk, size_t pk_len, const uint8_t* info,
                                  size_t info_len, size_t n, const uint8_t* encs,
                                  const uint8_t* aads, const uint64_t* aad_offsets,
                                  const uint8_t* cts, const uint64_t* ct_offsets, uint8_t* pts,
                                  const uint64_t* pt_offsets, uint8_t* status) {
  return hpke_open_batch_entry(c, kem_id, kdf_id, aead_id, sk, sk_len, pk, pk_len, info, info_len,
                               n, encs, aads, aad_offsets, cts, ct_offsets, pts, pt_offsets,
                               status, /*team=*/true);
}

int prio3gpu_open_input_shares(prio3gpu_ctx* c, const uint8_t* task_id, uint16_t kem_id,
                               uint16_t kdf_id, uint16_t aead_id, const uint8_t* sk, size_t sk_len,
                               const uint8_t* pk, size_t pk_len, uint8_t recipient_role, size_t n,
                               const uint8_t* report_ids, const uint64_t* times,
                               const uint8_t* public_shares, uint32_t public_share_len,
                               const uint8_t* encs, size_t enc_pitch, const uint8_t* payloads,
                               size_t payload_pitch, uint32_t input_share_len,
                               uint8_t* out_shares, size_t share_pitch, uint8_t* status) {
  if (!c) {
    set_err("null context");
    return PRIO3GPU_E_ARG;
  }
  CHK(suite_check(c, "open_input_shares", /*seal=*/false, /*team=*/true, kem_id, kdf_id, aead_id));
  if (!task_id) {  // with the key lengths: before the keypair's check
    set_err("open_input_shares: null task id");
    return PRIO3GPU_E_ARG;
  }
  CHK(open_key_check("open_input_shares", kem_id, sk, sk_len, pk, pk_len));
  if (n == 0) return 0;
  if (!report_ids || !times || (public_share_len && !public_shares) || !encs || !payloads ||
      (input_share_len && !out_shares) || !status || n > 0x7FFFFFFFu) {
    set_err("open_input_shares: null argument");
    return PRIO3GPU_E_ARG;
  }
  const ShareColumns g =
      share_columns(kem_id, input_share_len, enc_pitch, payload_pitch, share_pitch);
  if (!g.ok()) {
    set_err("open_input_shares: a pitch is shorter than its row");
    return PRIO3GPU_E_ARG;
  }
  const size_t nenc = g.nenc, plen = g.plen;
  const size_t epitch = g.enc_pitch, ppitch = g.payload_pitch, spitch = g.share_pitch;
  uint8_t info[20];
  input_share_info(/*ROLE_CLIENT*/ 1, recipient_role, info);
  HpkeBatchConsts bc;
  if (!hpke_batch_consts(kem_id, kdf_id, aead_id, pk, info, sizeof info, &bc)) {
    set_err("HPKE primitives unavailable");
    return PRIO3GPU_E_UNSUPPORTED;
  }
  ReqTaskId tid;
  memcpy(tid.w, task_id, 32);  // little-endian host: byte j at bits 8 (j & 3) of word j >> 2
  HIPCHK(hipSetDevice(c->device));
  // host rows are staged with their gaps, one span per column; a host output is opened into
  // packed staging rows (zeroed after the copy: they are input shares), a device one in place
  const bool out_host = !(out_shares && is_device_ptr(out_shares));
  const size_t out_bytes = n * (size_t)input_share_len;
  const uint8_t *d_rid, *d_time, *d_pub, *d_enc, *d_pay, *d_st_in;
  CHK(stage_in(c, c->seal.rid, report_ids, n * 16, &d_rid, kHpkeMinStage));
  CHK(stage_in(c, c->seal.time, times, n * 8, &d_time, kHpkeMinStage));
  CHK(stage_in(c, c->seal.pub, public_shares, n * (size_t)public_share_len, &d_pub,
               kHpkeMinStage));
  CHK(stage_in(c, c->hpke.enc_in, encs, rows_span(n, epitch, nenc), &d_enc, kHpkeMinStage));
  CHK(stage_in(c, c->hpke.ct_in, payloads, rows_span(n, ppitch, plen), &d_pay, kHpkeMinStage));
  CHK(stage_in(c, c->hpke.status, status, n, &d_st_in, kHpkeMinStage));
  uint8_t* d_st = const_cast<uint8_t*>(d_st_in);
  uint8_t* d_out = out_shares;
  if (out_host) {
    CHK(c->hpke.pt_out.ensure(std::max<size_t>(out_bytes, kHpkeMinStage)));
    d_out = c->hpke.pt_out.u8();
  }
  // the ladder reads packed encapsulated keys: a pitched column is gathered first
  const uint8_t* d_enc_packed = d_enc;
  if (epitch != nenc) {
    CHK(c->seal.enc_packed.ensure(n * nenc));
    HIPCHK(hipMemcpy2DAsync(c->seal.enc_packed.p, nenc, d_enc, epitch, nenc, n,
                            hipMemcpyDeviceToDevice, c->stream));
    d_enc_packed = c->seal.enc_packed.u8();
  }
  // the per-report secrets: the DH values (keys, nonces and round keys never leave registers)
  // and, after their copy, the staged share rows
  CallSecrets sec;
  int rc = [&]() -> int {
    uint32_t* d_dh;
    CHK(open_dh(c, sec, kem_id, sk, pk, bc, /*raw=*/false, n, d_enc_packed, &d_dh));
    const TeamSplit sp = share_split(c, n, input_share_len, aead_id);
    if (sp.S >= 2) {
      // several waves per report: the segments, the verdicts, and zeros over every failed row,
      // queued back to back -- nothing later on the stream sees unauthenticated plaintext
      SplitShareCall q;
      CHK(split_call(c, sec, sp, n, bc, tid, d_rid, d_time, d_pub, public_share_len,
                     input_share_len, d_st, &q));
      return launch_open_team_split(c, q, d_dh, d_enc, epitch, d_pay, ppitch, d_out,
                                    out_host ? input_share_len : spitch);
    }
    return launch_hpke_open_team_shares(
        c, ShareOpenCall{(uint32_t)n, bc, tid, d_dh, d_rid,
                         reinterpret_cast<const uint64_t*>(d_time), d_pub, public_share_len,
                         d_enc, (uint64_t)epitch, d_pay, (uint64_t)ppitch, input_share_len,
                         d_out, (uint64_t)(out_host ? input_share_len : spitch), d_st});
  }();
  rc = sec.finish(c, rc);
  if (out_host && out_bytes) {
    sec.add(d_out, out_bytes);
    if (!rc) rc = packed_rows_to_host(c, out_shares, spitch, d_out, input_share_len, n);
    rc = sec.finish(c, rc);
  }
  if (rc) return rc;
  CHK(copy_out(c, status, d_st, n));
  return finish_call(c, {report_ids, times, public_shares, encs, payloads, out_shares, status});
}

int prio3gpu_hpke_open_report_shares_gpu(
    prio3gpu_ctx* c, const uint8_t* task_id, const prio3gpu_hpke_keypair* task_keys,
    size_t n_task_keys, const prio3gpu_hpke_keypair* global_keys, size_t n_global_keys,
    uint8_t sender_role, uint8_t recipient_role, const uint8_t* msg,
    const prio3gpu_prepare_init_view* views, size_t n, uint8_t* plaintexts, uint64_t* offsets,
    uint8_t* status, int threads) {
  if (!c) {
    set_err("null context");
    return PRIO3GPU_E_ARG;
  }
  if (n == 0 || !plaintexts)  // n = 0 and the sizing call: offsets only
    return prio3gpu_hpke_open_report_shares(task_id, task_keys, n_task_keys, global_keys,
                                            n_global_keys, sender_role, recipient_role, msg, views,
                                            n, plaintexts, offsets, status, threads);
  if (!msg || !views || !offsets || !task_id || !status) return PRIO3GPU_E_ARG;
  plaintext_offsets(views, n, offsets);
  // The plan's groups go to the GPU, one batch per key; everything else (other suites, malformed
  // keys or encapsulated keys, unknown ids) is the host path's, untouched.
  HpkePlan plan;
  plan_hpke(task_keys, n_task_keys, global_keys, n_global_keys, views, status, n,
            hpke_gpu_opts(c), /*strict=*/true, &plan);
  uint8_t info[20];
  input_share_info(sender_role, recipient_role, info);
  // the status arrays of the two host passes: 0 selects a report
  std::vector<uint8_t> st_host(status, status + n), st_retry(n, 1);
  bool any_host = false, any_retry = false;
  for (size_t i = 0; i < n; ++i) {
    if (plan.route[i] >= 0) st_host[i] = 1;
    any_host |= plan.route[i] == ROUTE_HOST;
  }
  HpkeGroupBufs bufs;
  for (size_t k = 0; k < plan.groups.size(); ++k)
    CHK(open_group_packed(c, plan, k, info, task_id, msg, views, threads, bufs, plaintexts,
                          offsets, status, st_retry.data(), &any_retry));
  if (any_host) {
    CHK(prio3gpu_hpke_open_report_shares(task_id, task_keys, n_task_keys, global_keys,
                                         n_global_keys, sender_role, recipient_role, msg, views, n,
                                         plaintexts, offsets, st_host.data(), threads));
    for (size_t i = 0; i < n; ++i)
      if (plan.route[i] < 0) status[i] = st_host[i];
  }
  if (any_retry) {  // the global key of the same id gets the second trial, on the host
    std::vector<uint8_t> was_retry(st_retry);
    CHK(prio3gpu_hpke_open_report_shares(task_id, nullptr, 0, global_keys, n_global_keys,
                                         sender_role, recipient_role, msg, views, n, plaintexts,
                                         offsets, st_retry.data(), threads));
    for (size_t i = 0; i < n; ++i)
      if (!was_retry[i]) status[i] = st_retry[i];
  }
  return 0;
}

int prio3gpu_helper_init_request(
    prio3gpu_ctx* c, prio3gpu_state* st, const uint8_t* task_id,
    const prio3gpu_hpke_keypair* task_keys, size_t n_task_keys,
    const prio3gpu_hpke_keypair* global_keys, size_t n_global_keys, uint8_t sender_role,
    uint8_t recipient_role, const uint8_t* msg, size_t msg_len,
    const prio3gpu_prepare_init_view* views, size_t n, const uint32_t* batch_slots,
    uint8_t* out_nonces, uint8_t* out_prep_msgs, uint8_t* status, prio3gpu_agg* agg, int threads) {
  CHK(check_state(c, st, n));
  if (st->agg_id != 1) {
    set_err("helper_init_request needs a helper (agg_id 1) state");
    return PRIO3GPU_E_ARG;
  }
  if (st->vk_num != 0) {  // one task id, one request: the state's key table has no meaning here
    set_err("helper_init_request on a state with verify keys set (prio3gpu_state_set_verify_keys)");
    return PRIO3GPU_E_ARG;
  }
  if (n == 0) return 0;
  if (!task_id || !msg || !views || !status || (n_task_keys && !task_keys) ||
      (n_global_keys && !global_keys) || n > 0x7FFFFFFFu) {
    set_err("helper_init_request: null argument");
    return PRIO3GPU_E_ARG;
  }
  if (agg && agg->ctx != c) {
    set_err("aggregate belongs to another context");
    return PRIO3GPU_E_ARG;
  }
  if (is_device_ptr(views) || is_device_ptr(status)) {
    set_err("helper_init_request: views and status are host memory");
    return PRIO3GPU_E_ARG;
  }
  CHK(check_views(c->cfg, views, n, msg_len));
  ReqCall q{};
  q.c = c, q.st = st, q.task_id = task_id;
  q.sender_role = sender_role, q.recipient_role = recipient_role;
  q.msg = msg, q.msg_len = msg_len, q.views = views, q.n = n, q.threads = threads;
  CHK(req_plan(q, task_keys, n_task_keys, global_keys, n_global_keys, status));
  CHK(req_reserve(q));
  int rc = req_upload_gather(q);
  if (!rc) rc = req_open_groups(q);
  if (!rc) rc = req_decode(q);
  if (!rc) rc = req_host_fallback(q);
  CHK(q.sec.finish(c, rc));
  CHK(copy_out(c, out_nonces, st->nonces.u8(), n * 16));
  rc = prio3gpu_helper_init(c, st, n, st->nonces.u8(), st->pub.u8(), q.d_in, c->io[0].u8(),
                            batch_slots, out_prep_msgs, q.d_status, agg);
  if (rc) {
    (void)hipStreamSynchronize(c->stream);
    return rc;
  }
  HIPCHK(hipMemcpyAsync(status, q.d_status, n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int prio3gpu_test_req_gather(prio3gpu_ctx* c, const uint8_t* msg, size_t msg_len,
                             const prio3gpu_prepare_init_view* views, size_t n, uint8_t* nonces,
                             uint8_t* public_shares, uint8_t* leader_prep_shares,
                             uint8_t* faults) {
  if (!c || (n && (!msg || !views || !nonces || !public_shares || !leader_prep_shares ||
                   !faults)) || n > 0x7FFFFFFFu) {
    set_err("null argument");
    return PRIO3GPU_E_ARG;
  }
  if (n == 0) return 0;
  const Cfg& g = c->cfg;
  CHK(check_views(g, views, n, msg_len));
  HIPCHK(hipSetDevice(c->device));
  const size_t nb_pub = n * (size_t)g.public_share_len, nb_lps = n * (size_t)g.prep_share_len;
  const uint8_t* d_msg;
  CHK(stage_in(c, c->req.msg, msg, msg_len, &d_msg, 16));
  CHK(c->req.views.ensure(n * sizeof(ReqView)));
  CHK(c->req.faults.ensure(n));
  CHK(c->io[0].ensure(std::max<size_t>(nb_lps, 16)));
  CHK(c->io[1].ensure(std::max<size_t>(nb_pub, 16)));
  CHK(c->io[2].ensure(n * 16));
  HIPCHK(hipMemcpyAsync(c->req.views.p, views, n * sizeof(ReqView), hipMemcpyHostToDevice,
                        c->stream));
  CHK(launch_req_gather(c, n, d_msg, msg_len, static_cast<const ReqView*>(c->req.views.p),
                        c->io[2].u8(), c->io[1].u8(), c->io[0].u8(), c->req.faults.u8()));
  CHK(copy_out(c, nonces, c->io[2].u8(), n * 16));
  CHK(copy_out(c, public_shares, c->io[1].u8(), nb_pub));
  CHK(copy_out(c, leader_prep_shares, c->io[0].u8(), nb_lps));
  CHK(copy_out(c, faults, c->req.faults.u8(), n));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int prio3gpu_test_x25519_gpu(prio3gpu_ctx* c, const uint8_t* sk, const uint8_t* points, size_t n,
                             uint8_t* out) {
  if (!c || (n && (!sk || !points || !out)) || n > 0x7FFFFFFFu) {
    set_err("null argument");
    return PRIO3GPU_E_ARG;
  }
  if (n == 0) return 0;
  HIPCHK(hipSetDevice(c->device));
  const uint8_t* d_pts;
  CHK(stage_in(c, c->hpke.enc_in, points, n * 32, &d_pts, kHpkeMinStage));
  CallSecrets sec;  // the DH values are this hook's output: cleared after their copy
  HpkeBatchConsts bc{};
  uint32_t* d_dh;
  int rc = open_dh(c, sec, 0x0020, sk, nullptr, bc, /*raw=*/false, n, d_pts, &d_dh);
  if (!rc) rc = copy_out(c, out, d_dh, n * 32);
  rc = sec.finish(c, rc);
  HIPCHK(hipStreamSynchronize(c->stream));
  return rc;
}

int prio3gpu_test_p256_gpu(prio3gpu_ctx* c, const uint8_t* sk, const uint8_t* points, size_t n,
                           uint8_t* out_x, uint8_t* ok) {
  if (!c || !sk || (n && (!points || !out_x || !ok)) || n > 0x7FFFFFFFu) {
    set_err("null argument");
    return PRIO3GPU_E_ARG;
  }
  if (!p256_scalar_valid(sk)) {
    set_err("P-256 scalar outside [1, n)");
    return PRIO3GPU_E_HPKE;
  }
  if (n == 0) return 0;
  // the generator stands in for pkRm: a refused encoding's lane runs over it
  HpkeBatchConsts bc{};  // raw mode hashes nothing: the pad states are not read
  HIPCHK(hipSetDevice(c->device));
  const uint8_t* d_pts;
  CHK(stage_in(c, c->hpke.enc_in, points, n * 65, &d_pts, kHpkeMinStage));
  CallSecrets sec;  // the DH values are this hook's output: cleared after their copy
  uint32_t* d_dh;
  int rc = open_dh(c, sec, 0x0010, sk, kP256G, bc, /*raw=*/true, n, d_pts, &d_dh);
  if (!rc) rc = copy_out(c, out_x, d_dh, n * 32);
  if (!rc) rc = copy_out(c, ok, dh_ok_at(d_dh, n), n);
  rc = sec.finish(c, rc);
  HIPCHK(hipStreamSynchronize(c->stream));
  return rc;
}

int prio3gpu_test_p256_eph_gpu(prio3gpu_ctx* c, const uint8_t* pk, const uint8_t* sk_es, size_t n,
                               uint8_t* out_enc, uint8_t* out_dh_x, uint8_t* ok) {
  if (!c || !pk || (n && (!sk_es || !out_enc || !out_dh_x || !ok)) || n > 0x7FFFFFFFu) {
    set_err("null argument");
    return PRIO3GPU_E_ARG;
  }
  CHK(seal_pk_check(0x0010, pk, 65));
  if (n == 0) return 0;
  HIPCHK(hipSetDevice(c->device));
  const uint8_t* d_sk;
  const size_t nb = eph_bytes(n, /*p256=*/true);
  CHK(c->seal.eph.ensure(nb));
  uint8_t* d_eph = c->seal.eph.u8();
  std::vector<uint8_t> h(nb);
  CallSecrets sec;  // the ladders' output is this hook's: cleared after its copy
  sec.add(d_eph, nb);
  int rc = stage_secret(c, sec, c->seal.eph_sk, sk_es, n * 32, &d_sk);
  if (!rc)
    rc = launch_p256_eph(c, pk, n, d_sk, reinterpret_cast<uint32_t*>(d_eph),
                         p256_eph_ok_at(d_eph, n));
  if (!rc) rc = copy_out(c, h.data(), d_eph, nb);
  rc = sec.finish(c, rc);
  HIPCHK(hipStreamSynchronize(c->stream));
  if (rc) return rc;
  for (size_t i = 0; i < n; ++i) {  // enc = 0x04 || x || y; all zeros for a refused scalar
    ok[i] = p256_eph_ok_at(h.data(), n)[i];
    out_enc[i * 65] = ok[i] ? 0x04 : 0x00;
    memcpy(out_enc + i * 65 + 1, &h[i * 64], 64);
    memcpy(out_dh_x + i * 32, &h[n * 64 + i * 32], 32);
  }
  wipe(h.data(), h.size());
  return 0;
}

int prio3gpu_test_poly1305_gpu(prio3gpu_ctx* c, const uint8_t* keys, const uint8_t* msgs,
                               const uint64_t* msg_offsets, size_t n, uint8_t* tags) {
  if (!c || (n && (!keys || !msg_offsets || !tags)) || n > 0x7FFFFFFFu) {
    set_err("null argument");
    return PRIO3GPU_E_ARG;
  }
  if (n == 0) return 0;
  const uint64_t total = msg_offsets[n];
  for (size_t i = 0; i < n; ++i)
    if (msg_offsets[i] > msg_offsets[i + 1]) {
      set_err("message offsets out of order");
      return PRIO3GPU_E_ARG;
    }
  if (total && !msgs) {
    set_err("null argument");
    return PRIO3GPU_E_ARG;
  }
  HIPCHK(hipSetDevice(c->device));
  const uint8_t *d_keys, *d_msgs, *d_off;
  CHK(stage_in(c, c->hpke.enc_in, keys, n * 32, &d_keys, kHpkeMinStage));
  CHK(stage_in(c, c->hpke.aad, msgs, total, &d_msgs, kHpkeMinStage));
  CHK(stage_in(c, c->hpke.aad_off, msg_offsets, (n + 1) * 8, &d_off, kHpkeMinStage));
  CHK(c->hpke.pt_out.ensure(n * 16));
  CHK(launch_test_poly1305(c, n, d_keys, d_msgs, reinterpret_cast<const uint64_t*>(d_off),
                           c->hpke.pt_out.u8()));
  HIPCHK(hipMemcpyAsync(tags, c->hpke.pt_out.u8(), n * 16, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

}  // extern "C"
