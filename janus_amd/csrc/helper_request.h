// The helper's aggregate-init straight from the request's bytes (prio3gpu_helper_init_request):
// the kernels between the AggregationJobInitializeReq in device memory and the report-major rows
// prio3gpu_helper_init reads.  Nothing here builds packed copies of enc / aad / ciphertext: every
// kernel reads the request through the decoded views (prio3gpu_prepare_init_view), whose offsets
// the host has checked against the message length.
//   k_req_gather        nonces, public shares, leader prep shares -> rows; faults[i]
//   k_hpke_open_req     hpke_open_lane (of the group's suite) over a key group (a list of report
//                       indices): enc and ciphertext in place, the InputShareAad assembled from
//                       its five pieces (hpke_lane.h's ReqAad), never materialised
//   k_decode_plaintext_input_shares   PlaintextInputShare -> helper input share row, then faults
//   k_req_scatter       host-fallback reports' rows and statuses into place
// A key group's DH values are hpke_dh_gpu.h's k_x25519_idx and k_p256_dh_idx, enc read in place.
// Included by engine_hpke_team.hip alone, after include/prio3gpu.h.
#pragma once
#include "hpke_kernel_args.h"
#include "hpke_lane.h"
#include "request_parse.h"

namespace p3g {

// ---- gather ------------------------------------------------------------------------------------
// One lane per 16-byte piece of a destination row; blockIdx.y picks the row kind (0 nonces,
// 1 public shares, 2 leader prep shares), so consecutive lanes read consecutive 16-byte pieces of
// one report's field and store consecutive pieces of its row.  A source offset has any byte
// alignment: the lane reads the aligned words that cover its piece and funnel-shifts them
// (v_alignbyte_b32); rows that are 16-byte aligned get one 16-byte store per piece.  The aligned
// window may reach up to 3 bytes before and after the piece, so it is taken only where it lies
// inside [msg, msg + msg_len); the head and tail pieces of the message, a row's short last piece
// and unaligned rows go byte by byte.  The nonce lane of a report also records its fault
// (prepare_init_fault); the public-share and prep-share rows of a faulty report are zeroed.
__global__ void __launch_bounds__(256) k_req_gather(uint32_t n, const uint8_t* msg,
                                                    uint64_t msg_len, const ReqView* views,
                                                    uint32_t pub_len, uint32_t prep_len,
                                                    uint8_t* nonces, uint8_t* pub, uint8_t* lps,
                                                    uint8_t* faults) {
  const uint32_t kind = blockIdx.y;
  const uint32_t row_len = kind == 0 ? 16u : kind == 1 ? pub_len : prep_len;
  const uint64_t ppr = (row_len + 15u) / 16u;  // pieces per row
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ppr * n) return;
  const uint32_t r = (uint32_t)(g / ppr);
  const uint64_t o = (g % ppr) * 16;
  const ReqView& v = views[r];
  const uint8_t fault =
      prepare_init_fault(v.public_share_len, v.prep_share_len, v.message_type, pub_len, prep_len);
  if (kind == 0) faults[r] = fault;
  const uint64_t src_off = kind == 0 ? v.report_id_off : kind == 1 ? v.public_share_off
                                                                   : v.prep_share_off;
  uint8_t* d = (kind == 0 ? nonces : kind == 1 ? pub : lps) + (uint64_t)r * row_len + o;
  const uint32_t nb = row_len - o < 16 ? (uint32_t)(row_len - o) : 16u;
  const bool zero = kind != 0 && fault != REQ_OK;
  uint32_t w[4] = {0, 0, 0, 0};
  if (!zero) {
    const uint8_t* s = msg + src_off + o;
    const uint32_t sh = (uint32_t)((uintptr_t)s & 3u);
    const uint8_t* q = s - sh;
    if (nb == 16 && q >= msg && q + (sh ? 20 : 16) <= msg + msg_len) {
      const uint32_t* qw = reinterpret_cast<const uint32_t*>(q);
      uint32_t x[5];
#pragma unroll
      for (int i = 0; i < 4; ++i) x[i] = qw[i];
      x[4] = sh ? qw[4] : 0u;
#pragma unroll
      for (int i = 0; i < 4; ++i) w[i] = __builtin_amdgcn_alignbyte(x[i + 1], x[i], sh);
    } else {
      for (uint32_t j = 0; j < nb; ++j) w[j >> 2] |= (uint32_t)s[j] << (8 * (j & 3));
    }
  }
  if (nb == 16 && ((uintptr_t)d & 15u) == 0) {
    *reinterpret_cast<uint4*>(d) = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
    for (uint32_t j = 0; j < nb; ++j) d[j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
  }
}

// ---- the open, in place ------------------------------------------------------------------------
// One lane per report of a key group: hpke_open_lane with enc, ciphertext and AAD read where the
// request has them; report r's plaintext goes to pts[pt_off[r] .. pt_off[r + 1]).  An enc_len
// other than the KEM's Nenc (32; 65 for P-256), a payload shorter than the tag or longer than its slot: status 4, nothing read.
// (KDF, AEAD) is the group's suite, as for k_hpke_open.
template <int KDF, int AEAD>
__global__ void __launch_bounds__(256) k_hpke_open_req(
    uint32_t m, HpkeBatchConsts bc, ReqTaskId tid, const uint32_t* idx, const uint32_t* dh,
    const uint8_t* msg, const ReqView* views, uint8_t* pts, const uint64_t* pt_off,
    uint8_t* status) {
  const uint8_t* sbox = nullptr;
  if constexpr (AEAD != 3) {
    __shared__ uint8_t sbox_lds[256];
    aes_sbox_fill(sbox_lds, threadIdx.x, blockDim.x);
    __syncthreads();
    sbox = sbox_lds;
  }
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const uint32_t r = idx[j];
  const ReqView& v = views[r];
  const uint64_t p0 = pt_off[r], pt_cap = pt_off[r + 1] - p0;
  uint8_t* pt = pts + p0;
  const bool skip = status[r] != 0;
  const uint32_t clen = v.payload_len;
  if (skip || v.enc_len != bc.nenc || clen < 16 || clen - 16 > pt_cap) {
    hpke_open_reject(pt, pt_cap, status + r, skip);
    return;
  }
  const ReqAad aad{tid, msg + v.report_id_off, v.time, v.public_share_len,
                   msg + v.public_share_off};
  hpke_open_lane<KDF, AEAD>(sbox, bc, dh + (size_t)r * 8, bc.dh_ok ? bc.dh_ok[r] : 1u,
                            msg + v.enc_off, aad,
                            msg + v.payload_off, (uint64_t)clen - 16, pt, pt_cap, status + r);
}

// ---- decode ------------------------------------------------------------------------------------
// One lane per report: parse_plaintext_input_share (request_parse.h) over the opened plaintext,
// the payload copied to the report's helper input share row (zeroed otherwise), then the
// report's structural fault if it is still OK.  A report whose status is non-zero keeps it
// (REQ_HOST: the host path fills its row later); an extension list past kReqMaxExtList marks the
// report REQ_DEFER for the host decode.
__global__ void __launch_bounds__(256) k_decode_plaintext_input_shares(
    uint32_t n, const uint8_t* pts, const uint64_t* pt_off, uint32_t want, uint8_t* rows,
    uint64_t pitch, const uint8_t* faults, uint8_t* status) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  uint8_t* row = rows + (uint64_t)r * pitch;
  uint8_t st = status[r];
  const uint8_t* p = pts + pt_off[r];
  PlaintextParse pp{REQ_INVALID, 0};
  if (st == REQ_OK) {
    pp = parse_plaintext_input_share(p, pt_off[r + 1] - pt_off[r], want);
    st = pp.status;
  }
  if (st == REQ_OK) {
    for (uint32_t j = 0; j < want; ++j) row[j] = p[pp.payload_off + j];
  } else {
    for (uint32_t j = 0; j < want; ++j) row[j] = 0;
  }
  status[r] = apply_fault(st, faults[r]);
}

// The k reports the host path opened and decoded: report idx[j] gets row j of the compact rows
// and status sts[j] (then its fault, like every other report).
__global__ void __launch_bounds__(256) k_req_scatter(uint32_t k, const uint32_t* idx,
                                                     const uint8_t* crows, const uint8_t* sts,
                                                     uint32_t want, uint8_t* rows, uint64_t pitch,
                                                     const uint8_t* faults, uint8_t* status) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= k) return;
  const uint32_t r = idx[j];
  uint8_t* row = rows + (uint64_t)r * pitch;
  for (uint32_t b = 0; b < want; ++b) row[b] = crows[(uint64_t)j * want + b];
  status[r] = apply_fault(sts[j], faults[r]);
}

}  // namespace p3g
