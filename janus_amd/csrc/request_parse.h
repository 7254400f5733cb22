// The per-report rules of the fused helper aggregate-init (helper_request.h), free of HIP so the
// device kernels and a CPU test (tests/native/request_parse_host.cpp) run the same code:
//   parse_plaintext_input_share  PlaintextInputShare -> where its payload lies, or why it is bad;
//                                mirrors prio3gpu_decode_plaintext_input_shares (codec.cpp)
//   prepare_init_fault           the structural fault of one PrepareInit; mirrors
//                                prio3gpu_gather_prepare_inits
//   apply_fault                  prio3gpu_apply_faults for one report
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define P3G_RQ __host__ __device__ inline
#else
#define P3G_RQ inline
#endif

namespace p3g {

// The duplicate-extension check rescans the list once per item: quadratic in the item count.  A
// list of at most this many bytes holds at most 64 items (4 bytes each at least), 2,016 compares;
// a longer list is not parsed by a GPU lane but deferred to the host decode (same answer).
constexpr uint32_t kReqMaxExtList = 256;

constexpr uint8_t REQ_OK = 0;
constexpr uint8_t REQ_INVALID = 8;  // PrepareError::InvalidMessage
constexpr uint8_t REQ_VDAF_PREP = 5;  // PrepareError::VdafPrepError
// Private markers of the fused call's device status array (never returned to a caller):
constexpr uint8_t REQ_DEFER = 0xFE;  // extension list longer than kReqMaxExtList: host decode
constexpr uint8_t REQ_HOST = 0xFF;   // opened and decoded on the host path

struct PlaintextParse {
  uint8_t status;        // REQ_OK, REQ_INVALID or REQ_DEFER
  uint32_t payload_off;  // REQ_OK: the `want` payload bytes start here
};

P3G_RQ uint32_t req_be(const uint8_t* p, int nbytes) {
  uint32_t v = 0;
  for (int i = 0; i < nbytes; ++i) v = (v << 8) | p[i];
  return v;
}

// PlaintextInputShare (messages/src/lib.rs:1253-1300): u16-prefixed list of Extension{u16 type,
// u16-prefixed data}, then the u32-prefixed payload, which must be exactly `want` bytes and end
// the plaintext.  An item running past the list, a duplicate type, a wrong payload length or a
// trailing byte is REQ_INVALID.
P3G_RQ PlaintextParse parse_plaintext_input_share(const uint8_t* p, uint64_t len, uint32_t want) {
  PlaintextParse r{REQ_INVALID, 0};
  if (len < 2) return r;
  const uint64_t ext_len = req_be(p, 2);
  if (ext_len > kReqMaxExtList) {
    r.status = REQ_DEFER;
    return r;
  }
  const uint64_t ext_end = 2 + ext_len;
  if (ext_end > len) return r;
  uint64_t off = 2;
  while (off < ext_end) {
    if (ext_end - off < 4) return r;
    const uint32_t t = req_be(p + off, 2);
    const uint64_t next = off + 4 + req_be(p + off + 2, 2);
    if (next > ext_end) return r;
    for (uint64_t q = 2; q < off; q += 4 + (uint64_t)req_be(p + q + 2, 2))
      if (req_be(p + q, 2) == t) return r;  // duplicate extension
    off = next;
  }
  if (len - off < 4) return r;
  const uint64_t pl = req_be(p + off, 4);
  if (pl != want || len - off - 4 != pl) return r;
  r.status = REQ_OK;
  r.payload_off = (uint32_t)(off + 4);
  return r;
}

// What a PrepareInit's framing alone rejects (aggregator.rs:1755-1797): a public share of the
// wrong length is InvalidMessage, anything but Initialize{prep share of the right length} is
// VdafPrepError.
P3G_RQ uint8_t prepare_init_fault(uint32_t public_share_len, uint32_t prep_share_len,
                                  uint8_t message_type, uint32_t want_public, uint32_t want_prep) {
  if (public_share_len != want_public) return REQ_INVALID;
  if (message_type != 0 || prep_share_len != want_prep) return REQ_VDAF_PREP;
  return REQ_OK;
}

// The helper loop's precedence: a fault counts only for a report every earlier stage accepted.
P3G_RQ uint8_t apply_fault(uint8_t status, uint8_t fault) { return status ? status : fault; }

}  // namespace p3g
