// Host planning of the helper's HPKE open and of the fused aggregate-init from the request's bytes,
// no HIP: which key opens a report, which reports the GPU opens (one group per keypair) and which
// the host, the second trial with a global key, the host fallback's packed upload, and the checks
// of a request's views.  Included by engine_hpke.hip, engine_hpke_team.hip (req_gather_blocks)
// and hpke.cpp; built alone with g++ by tests/test_hpke_plan.py.  A plan points at the caller's
// keypairs and never copies key bytes.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/prio3gpu.h"
#include "cfg.h"
#include "p256.h"
#include "request_parse.h"

namespace p3g {

// The first keypair of the list with this config id, or null.
inline const prio3gpu_hpke_keypair* find_keypair(const prio3gpu_hpke_keypair* keys, size_t n,
                                                 uint8_t config_id) {
  for (size_t k = 0; k < n; ++k)
    if (keys[k].config_id == config_id) return &keys[k];
  return nullptr;
}

// HpkeApplicationInfo of an input share: Label::InputShare || sender || recipient (hpke.rs:52-77).
inline void input_share_info(uint8_t sender_role, uint8_t recipient_role, uint8_t out[20]) {
  memcpy(out, "dap-07 input share", 18);
  out[18] = sender_role;
  out[19] = recipient_role;
}

// out[i]: where report i's plaintext lies in the packed plaintexts (a payload less its 16-byte
// tag; nothing for a payload shorter than a tag); out[n]: their total.
inline void plaintext_offsets(const prio3gpu_prepare_init_view* views, size_t n, uint64_t* out) {
  out[0] = 0;
  for (size_t i = 0; i < n; ++i)
    out[i + 1] = out[i] + (views[i].payload_len >= 16 ? views[i].payload_len - 16 : 0);
}

// The context options that widen what the GPU opens, as a bit mask (a plain `true` is
// HPKE_OPT_SUITES, what the parameter meant while it was a bool).
constexpr unsigned HPKE_OPT_SUITES = 1u;  // "hpke_gpu_suites": every KDF and AEAD
constexpr unsigned HPKE_OPT_P256 = 2u;    // "hpke_gpu_p256": DHKEM(P-256, HKDF-SHA256) too
// "hpke_team_chacha": the wave-per-report opens and seals take ChaCha20-Poly1305 (no part in what
// hpke_gpu_suite, and so plan_hpke, answers)
constexpr unsigned HPKE_OPT_TEAM_CHACHA = 4u;

// The suites the GPU opens: DHKEM(X25519, HKDF-SHA256) / HKDF-SHA256 / AES-128-GCM always; with
// HPKE_OPT_P256 the same under DHKEM(P-256, HKDF-SHA256); with HPKE_OPT_SUITES every KDF and AEAD
// Janus accepts, under the KEMs the other bit allows.
inline bool hpke_gpu_suite(unsigned opts, uint16_t kem, uint16_t kdf, uint16_t aead) {
  if (kem != 0x0020 && !(kem == 0x0010 && (opts & HPKE_OPT_P256))) return false;
  if (kdf == 1 && aead == 1) return true;
  return (opts & HPKE_OPT_SUITES) && kdf >= 1 && kdf <= 3 && aead >= 1 && aead <= 3;
}

// The suites the GPU seals a lane per report (the seal has entry points of its own, so no option
// but the KEM's): DHKEM(X25519, HKDF-SHA256) with KDF 1-3 and AEAD 1-3, and with HPKE_OPT_P256
// the same under DHKEM(P-256, HKDF-SHA256).
inline bool hpke_seal_suite(unsigned opts, uint16_t kem, uint16_t kdf, uint16_t aead) {
  return (kem == 0x0020 || (kem == 0x0010 && (opts & HPKE_OPT_P256))) && kdf >= 1 && kdf <= 3 &&
         aead >= 1 && aead <= 3;
}

// The suites the wave-per-report opens and seals take (hpke_open_team.h, hpke_seal_team.h):
// hpke_seal_suite's, ChaCha20-Poly1305 (AEAD 3) only with HPKE_OPT_TEAM_CHACHA.
inline bool hpke_team_suite(unsigned opts, uint16_t kem, uint16_t kdf, uint16_t aead) {
  return hpke_seal_suite(opts, kem, kdf, aead) && (aead != 3 || (opts & HPKE_OPT_TEAM_CHACHA));
}

// Nenc = Npk of a KEM the GPU opens (RFC 9180 §7.1): 32 for X25519, 65 for P-256.
inline uint32_t hpke_kem_nenc(uint16_t kem) { return kem == 0x0010 ? 65u : 32u; }

// The three columns of prio3gpu_seal_input_shares[_long] and prio3gpu_open_input_shares: rows of
// nenc (encapsulated key), plen (payload: the 6 bytes around an extension-free share, the share,
// the 16-byte tag) and input_share_len bytes, each `pitch` bytes apart; a pitch of 0 means
// packed, the row's own width.  *_ok: the pitch holds its row.
struct ShareColumns {
  uint64_t nenc, plen;
  uint64_t enc_pitch, payload_pitch, share_pitch;  // effective
  bool enc_ok, payload_ok, share_ok;
  bool ok() const { return enc_ok && payload_ok && share_ok; }
};
inline ShareColumns share_columns(uint16_t kem, uint32_t input_share_len, uint64_t enc_pitch,
                                  uint64_t payload_pitch, uint64_t share_pitch) {
  ShareColumns g{};
  g.nenc = hpke_kem_nenc(kem);
  g.plen = 6 + (uint64_t)input_share_len + 16;
  g.enc_pitch = enc_pitch ? enc_pitch : g.nenc;
  g.payload_pitch = payload_pitch ? payload_pitch : g.plen;
  g.share_pitch = share_pitch ? share_pitch : input_share_len;
  g.enc_ok = g.enc_pitch >= g.nenc;
  g.payload_ok = g.payload_pitch >= g.plen;
  g.share_ok = g.share_pitch >= input_share_len;
  return g;
}

// Bytes from the first row's start to the last row's end: n >= 1 rows of `width` bytes.
inline uint64_t rows_span(uint64_t n, uint64_t pitch, uint64_t width) {
  return (n - 1) * pitch + width;
}

// Several waves per report ("hpke_team_split"): a body of body_bytes (nb 16-byte blocks) is cut
// into S segments of L blocks, segment s covering blocks [s L, min((s + 1) L, nb)), each run by a
// wave of its own (hpke_team_split.h).  n reports in the call; `unit` one team stripe in blocks
// (64 for AES-GCM, 256 for ChaCha20-Poly1305: L is a multiple, so a segment starts on a stripe);
// cap the option's value; min_blocks "hpke_team_split_blocks", the smallest segment worth a wave;
// wave_slots the waves the chip holds at once.  S = 1 (L = nb) means no split: the one-wave
// kernels run.  A call that fills the chip by itself (n >= wave_slots) never splits.
struct TeamSplit {
  uint32_t S;
  uint64_t L;
};
inline TeamSplit team_split_plan(uint64_t n, uint64_t body_bytes, uint32_t unit, uint32_t cap,
                                 uint64_t min_blocks, uint64_t wave_slots) {
  const uint64_t nb = (body_bytes + 15) / 16;
  if (n == 0 || unit == 0 || min_blocks == 0) return {1, nb};
  const uint64_t want = (wave_slots + n - 1) / n;
  const uint64_t s0 = std::min<uint64_t>(std::min<uint64_t>(cap, want), nb / min_blocks);
  if (s0 < 2) return {1, nb};
  const uint64_t per = (nb + s0 - 1) / s0;
  const uint64_t L = (per + unit - 1) / unit * unit;
  const uint64_t S = (nb + L - 1) / L;
  if (S < 2) return {1, nb};
  return {(uint32_t)S, L};
}

// P-256 order n, big-endian
constexpr uint8_t kP256Order[32] = {0xff, 0xff, 0xff, 0xff, 0x00, 0x00, 0x00, 0x00, 0xff, 0xff, 0xff,
                                    0xff, 0xff, 0xff, 0xff, 0xff, 0xbc, 0xe6, 0xfa, 0xad, 0xa7, 0x17,
                                    0x9e, 0x84, 0xf3, 0xb9, 0xca, 0xc2, 0xfc, 0x63, 0x25, 0x51};

// 1 <= sk < n for a 32-byte big-endian scalar (no secret-dependent early exit).
inline bool p256_scalar_valid(const uint8_t sk[32]) {
  int borrow = 0;
  uint8_t nz = 0;
  for (int i = 31; i >= 0; --i) {
    borrow = ((int)sk[i] - (int)kP256Order[i] - borrow) < 0;
    nz |= sk[i];
  }
  return borrow && nz;
}

// A P-256 keypair the kernels may run under: the scalar in [1, n), the public key a valid point
// (p256.h's own DeserializePublicKey).  Checked on the host before anything is launched.
inline bool p256_keypair_valid(const uint8_t* sk, size_t sk_len, const uint8_t* pk, size_t pk_len) {
  if (!sk || sk_len != 32 || !pk || pk_len != 65 || !p256_scalar_valid(sk)) return false;
  uint32_t x[8], y[8];
  Fp256 X, Y;
  return p256_decode(pk, x, y, X, Y);
}

// What plan_hpke asks of a keypair before it gives it a group: 32-byte keys for X25519; for
// P-256 a keypair that passes p256_keypair_valid (a malformed one is the host's, whose open
// gives each report its status).
inline bool hpke_gpu_keypair(const prio3gpu_hpke_keypair& kp) {
  if (kp.kem_id == 0x0010)
    return p256_keypair_valid(kp.private_key, kp.private_key_len, kp.public_key,
                              kp.public_key_len);
  return kp.private_key && kp.private_key_len == 32 && kp.public_key && kp.public_key_len == 32;
}

// Where one report goes: a GPU group (>= 0) or one of these.
constexpr int32_t ROUTE_FAILED = -1;   // nonzero incoming status: nobody opens it
constexpr int32_t ROUTE_UNKNOWN = -2;  // no key has its config id (request mode only)
constexpr int32_t ROUTE_HOST = -3;     // the host path opens it

// The first-choice key of a report is the task key of its config id, else the global key.  A
// first choice of a suite the GPU opens, with well-formed keys (hpke_gpu_keypair), puts the report
// into that keypair's group (keypairs are told apart by address); any other key is the host's.
// The two callers differ in what they keep away from the kernels:
//  * strict (prio3gpu_hpke_open_report_shares_gpu, which packs fixed Nenc-byte encapsulated keys,
//    32 for X25519 and 65 for P-256): enc_len != Nenc or payload_len < 16 is the host's, and so
//    is an unknown id (the host pass gives it its status);
//  * request mode (prio3gpu_helper_init_request): such a report stays in its group and the kernel
//    rejects it; an unknown id is ROUTE_UNKNOWN and the caller sets its status.
struct HpkePlan {
  const prio3gpu_hpke_keypair *task_keys = nullptr, *global_keys = nullptr;
  size_t n_task_keys = 0, n_global_keys = 0;
  std::vector<int32_t> route;                        // per report
  std::vector<const prio3gpu_hpke_keypair*> groups;  // in order of first appearance
  std::vector<uint8_t> is_task_key;                  // per group: the keypair lies in task_keys
  std::vector<uint32_t> idx;                         // members, group by group, ascending
  std::vector<size_t> gbeg;                          // groups + 1 offsets into idx
};

inline void plan_hpke(const prio3gpu_hpke_keypair* task_keys, size_t n_task_keys,
                      const prio3gpu_hpke_keypair* global_keys, size_t n_global_keys,
                      const prio3gpu_prepare_init_view* views, const uint8_t* status, size_t n,
                      unsigned gpu_opts, bool strict, HpkePlan* out) {
  HpkePlan& p = *out;
  p = HpkePlan{};
  p.task_keys = task_keys, p.n_task_keys = n_task_keys;
  p.global_keys = global_keys, p.n_global_keys = n_global_keys;
  p.route.assign(n, ROUTE_FAILED);
  std::vector<size_t> count;
  std::vector<const prio3gpu_hpke_keypair*> refused;  // keypairs found unfit, checked once each
  for (size_t i = 0; i < n; ++i) {
    if (status[i]) continue;
    const prio3gpu_prepare_init_view& v = views[i];
    const prio3gpu_hpke_keypair* kp = find_keypair(task_keys, n_task_keys, v.hpke_config_id);
    if (!kp) kp = find_keypair(global_keys, n_global_keys, v.hpke_config_id);
    if (!kp) {
      p.route[i] = strict ? ROUTE_HOST : ROUTE_UNKNOWN;
      continue;
    }
    const size_t k = std::find(p.groups.begin(), p.groups.end(), kp) - p.groups.begin();
    if (k == p.groups.size()) {  // not yet a group: is the keypair fit for one?
      bool fit = std::find(refused.begin(), refused.end(), kp) == refused.end();
      if (fit && !(hpke_gpu_suite(gpu_opts, kp->kem_id, kp->kdf_id, kp->aead_id) &&
                   hpke_gpu_keypair(*kp))) {
        refused.push_back(kp);
        fit = false;
      }
      if (!fit) {
        p.route[i] = ROUTE_HOST;
        continue;
      }
    }
    if (strict && (v.enc_len != hpke_kem_nenc(kp->kem_id) || v.payload_len < 16)) {
      p.route[i] = ROUTE_HOST;
    } else {
      if (k == p.groups.size()) {
        p.groups.push_back(kp);
        p.is_task_key.push_back(kp >= task_keys && kp < task_keys + n_task_keys);
        count.push_back(0);
      }
      p.route[i] = (int32_t)k;
      ++count[k];
    }
  }
  p.gbeg.assign(p.groups.size() + 1, 0);
  for (size_t k = 0; k < p.groups.size(); ++k) p.gbeg[k + 1] = p.gbeg[k] + count[k];
  p.idx.resize(p.gbeg.back());
  std::copy(p.gbeg.begin(), p.gbeg.end() - 1, count.begin());  // each group's write cursor
  for (size_t i = 0; i < n; ++i)
    if (p.route[i] >= 0) p.idx[count[p.route[i]]++] = (uint32_t)i;
}

// After a failed open of report i on the GPU: does the global key of the same id get a second
// trial (on the host)?  Only a task key has a second choice.
inline bool wants_global_retry(const HpkePlan& p, const prio3gpu_prepare_init_view* views,
                               size_t i) {
  return p.route[i] >= 0 && p.is_task_key[p.route[i]] &&
         find_keypair(p.global_keys, p.n_global_keys, views[i].hpke_config_id);
}

// The fused call's device status image before any kernel: the incoming status, PrepareError::
// HpkeUnknownConfigId (3) for an unknown id, REQ_HOST for the host's reports.
inline void request_status_image(const HpkePlan& p, const uint8_t* status, size_t n, uint8_t* out) {
  for (size_t i = 0; i < n; ++i)
    out[i] = p.route[i] == ROUTE_UNKNOWN ? PRIO3GPU_HPKE_UNKNOWN_CONFIG_ID
             : p.route[i] == ROUTE_HOST  ? REQ_HOST
                                         : status[i];
}

// The host's share of the fused call, from the status image the kernels left: other suites and
// malformed keys (REQ_HOST) and long extension lists (REQ_DEFER), opened with the full key order;
// and the second trial after a failed task-key open, with the global keys alone.  Both are status
// arrays for the host open: 0 selects a report, 1 skips it.
struct HpkeFallback {
  std::vector<uint8_t> st_host, st_retry;
  size_t n_host = 0, n_retry = 0;
};
inline void classify_fallback(const HpkePlan& p, const prio3gpu_prepare_init_view* views,
                              const uint8_t* image, size_t n, HpkeFallback* out) {
  out->st_host.assign(n, 1), out->st_retry.assign(n, 1);
  out->n_host = out->n_retry = 0;
  for (size_t i = 0; i < n; ++i) {
    if (image[i] == REQ_HOST || image[i] == REQ_DEFER) {
      out->st_host[i] = 0;
      ++out->n_host;
    } else if (image[i] == PRIO3GPU_HPKE_DECRYPT_ERROR && wants_global_retry(p, views, i)) {
      out->st_retry[i] = 0;
      ++out->n_retry;
    }
  }
}

// The fallback reports' upload for k_req_scatter: indices | rows | statuses, ascending by report.
// rows: n x want decoded input shares; st: their n statuses.
struct FallbackLayout {
  size_t kf, o_rows, o_st, bytes;
};
inline FallbackLayout pack_fallback(const HpkeFallback& f, size_t n, const uint8_t* rows,
                                    const uint8_t* st, uint32_t want, std::vector<uint8_t>* fb) {
  FallbackLayout l{};
  l.kf = f.n_host + f.n_retry;
  l.o_rows = (l.kf * 4 + 15) / 16 * 16;
  l.o_st = l.o_rows + l.kf * want;
  l.bytes = l.o_st + l.kf;
  fb->assign(l.bytes, 0);
  size_t j = 0;
  for (size_t i = 0; i < n; ++i) {
    if (f.st_host[i] && f.st_retry[i]) continue;
    const uint32_t r = (uint32_t)i;
    memcpy(&(*fb)[4 * j], &r, 4);
    memcpy(&(*fb)[l.o_rows + j * want], rows + i * (size_t)want, want);
    (*fb)[l.o_st + j] = st[i];
    ++j;
  }
  return l;
}

inline bool span_fits(uint64_t off, uint64_t len, uint64_t total) {
  return off <= total && len <= total - off;
}

// k_req_gather's grid x: 256 lanes move 16-byte pieces, max_ppr pieces per report.
inline uint64_t req_gather_blocks(const Cfg& g, size_t n) {
  const uint64_t max_ppr =
      std::max<uint64_t>(1, (std::max(g.public_share_len, g.prep_share_len) + 15u) / 16u);
  return ((uint64_t)n * max_ppr + 255) / 256;
}

// Every offset a kernel (or the host fallback) reads through, against the message length; and
// the gather's grid, which must fit one launch.
inline int check_request_views(const Cfg& g, const prio3gpu_prepare_init_view* views, size_t n,
                               size_t msg_len, std::string* err) {
  for (size_t i = 0; i < n; ++i) {
    const prio3gpu_prepare_init_view& v = views[i];
    if (!span_fits(v.report_id_off, 16, msg_len) ||
        !span_fits(v.public_share_off, v.public_share_len, msg_len) ||
        !span_fits(v.enc_off, v.enc_len, msg_len) ||
        !span_fits(v.payload_off, v.payload_len, msg_len) ||
        !span_fits(v.prep_share_off, v.prep_share_len, msg_len) ||
        !span_fits(v.prep_msg_off, v.prep_msg_len, msg_len)) {
      *err = "view " + std::to_string(i) + " does not fit the " + std::to_string(msg_len) +
             "-byte message";
      return PRIO3GPU_E_ARG;
    }
  }
  if (req_gather_blocks(g, n) > 0x7FFFFFFFull) {
    *err = "job too large for one gather launch";
    return PRIO3GPU_E_CAPACITY;
  }
  return 0;
}

}  // namespace p3g
