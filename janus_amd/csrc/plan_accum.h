// Host planning of the segmented accumulation (k_accum_partial / k_accum_spec / k_accum_merge),
// no HIP: which measurement elements k_jr column-sums, the chunk plan of one batch, and where
// each host array lies in the two packed device buffers.  Included by engine_internal.h (the
// context keeps its last plan) and engine.hip; built alone with g++ by tests/test_host_plan.py.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/prio3gpu.h"
#include "cfg.h"

namespace p3g {

// Measurement-share words that k_jr absorbs through its LDS window ("fast" blocks 1..lf cover
// words [16, 21 (lf+1) - 5)); elements [e0, e1) lie entirely inside.  Field128 types with JR only.
inline bool spec_range(const Cfg& g, uint32_t& nd, uint32_t& e0, uint32_t& e1) {
  if (g.es != 16 || g.jr_len == 0) return false;
  const int64_t nbytes = (int64_t)g.meas_len * 16;
  const int64_t ndw = nbytes / 8, padw = (42 + nbytes) >> 3;
  auto is_fast = [&](int64_t b) { return b >= 1 && 21 * b + 15 < ndw && 21 * b + 20 < padw; };
  int64_t lf = 0;
  while (is_fast(lf + 1)) ++lf;
  if (lf < 1) return false;
  const int64_t f1 = (21 * (lf + 1) - 5) & ~(int64_t)1;
  nd = (uint32_t)ndw;
  e0 = 8;
  e1 = (uint32_t)(f1 / 2);
  return e1 > e0;
}

// What a plan depends on besides the per-report slots: a call without per-report slots whose key
// equals the last plan's reuses that plan on the device.  (nd, e0, e1) are zero when !spec.
struct AccumKey {
  size_t n = 0;
  uint32_t slots = 0;
  bool spec = false;
  uint32_t nd = 0, e0 = 0, e1 = 0;
  bool operator==(const AccumKey& o) const {
    return n == o.n && slots == o.slots && spec == o.spec && nd == o.nd && e0 == o.e0 && e1 == o.e1;
  }
};

// Chunks (runs of reports of one slot, contiguous per slot in chunk order) of two kinds:
//  * direct: k_accum_partial sums every measurement element of the chunk's reports;
//  * speculative (whole waves of 64 reports whose slots agree, when k_jr left column sums):
//    k_accum_spec folds the per-wave sums of elements [e0, e1) and corrects the rejected
//    rows, k_accum_partial adds the few edge elements outside that range.
struct AccumPlan {
  std::vector<uint32_t> perm;          // report indices, chunk by chunk
  std::vector<uint32_t> chunk_begin;   // nch + 1 offsets into perm
  std::vector<uint32_t> chunk_slot;    // nch
  std::vector<uint32_t> dir_ids;       // ndir chunk ids
  std::vector<uint32_t> spec_ids;      // nspec chunk ids
  std::vector<uint32_t> spec_wave_begin;  // nspec + 1 offsets into wave_list
  std::vector<uint32_t> wave_list;     // the 64-report waves of the speculative chunks
  uint32_t ndir = 0, nspec = 0, nch = 0;
};

constexpr size_t kAccumWCH = 32;  // waves per speculative chunk

// Elements per k_accum_partial block, and blocks (tiles) per chunk.
inline uint32_t accum_epb(uint32_t meas_len) {
  return std::min<uint32_t>(256, std::max<uint32_t>(1, meas_len));
}
inline uint32_t accum_tiles(uint32_t meas_len) {
  const uint32_t epb = accum_epb(meas_len);
  return (meas_len + epb - 1) / epb;
}
// CH, reports per direct chunk: about 2048 / tiles chunks per batch, at least four report groups.
inline size_t accum_direct_chunk(size_t n, uint32_t meas_len) {
  const uint32_t G = 256 / accum_epb(meas_len);
  const size_t target_chunks = std::max<size_t>(1, 2048 / accum_tiles(meas_len));
  return std::max<size_t>((size_t)G * 4, (n + target_chunks - 1) / target_chunks);
}

// The plan of n reports over S aggregate slots (`slots` null: every report in slot 0).  A slot
// >= S is PRIO3GPU_E_ARG with *err set.  n == 0 gives nch == 0.
inline int plan_accumulate(size_t n, const uint32_t* slots, uint32_t S, uint32_t meas_len,
                           bool spec, AccumPlan* out, std::string* err) {
  auto slot_of = [&](size_t r) -> uint32_t { return slots ? slots[r] : 0u; };
  for (size_t r = 0; r < n; ++r) {
    if (slot_of(r) >= S) {
      *err = "batch slot " + std::to_string(slot_of(r)) + " out of range (" + std::to_string(S) +
             " slots)";
      return PRIO3GPU_E_ARG;
    }
  }
  const size_t nw = (n + 63) / 64;
  std::vector<std::vector<uint32_t>> spec_w(S), direct_r(S);
  if (spec) {
    for (size_t w = 0; w < nw; ++w) {
      const size_t r0 = 64 * w, r1 = std::min(n, r0 + 64);
      const uint32_t s = slot_of(r0);
      bool uni = true;
      for (size_t r = r0 + 1; r < r1 && uni; ++r) uni = slot_of(r) == s;
      if (uni) {
        spec_w[s].push_back((uint32_t)w);
      } else {
        for (size_t r = r0; r < r1; ++r) direct_r[slot_of(r)].push_back((uint32_t)r);
      }
    }
  } else {
    for (size_t r = 0; r < n; ++r) direct_r[slot_of(r)].push_back((uint32_t)r);
  }
  const size_t CH = accum_direct_chunk(n, meas_len);
  AccumPlan& p = *out;
  p = AccumPlan{};
  auto& perm = p.perm;
  auto& cb = p.chunk_begin;
  auto& cs = p.chunk_slot;
  auto& wl = p.wave_list;
  for (uint32_t s = 0; s < S; ++s) {
    const auto& sw = spec_w[s];
    for (size_t i = 0; i < sw.size(); i += kAccumWCH) {
      p.spec_ids.push_back((uint32_t)cs.size());
      cb.push_back((uint32_t)perm.size());
      cs.push_back(s);
      p.spec_wave_begin.push_back((uint32_t)wl.size());
      for (size_t q = i; q < std::min(sw.size(), i + kAccumWCH); ++q) {
        wl.push_back(sw[q]);
        for (size_t r = 64 * (size_t)sw[q]; r < std::min(n, 64 * (size_t)sw[q] + 64); ++r)
          perm.push_back((uint32_t)r);
      }
    }
    const auto& dr = direct_r[s];
    for (size_t i = 0; i < dr.size(); i += CH) {
      p.dir_ids.push_back((uint32_t)cs.size());
      cb.push_back((uint32_t)perm.size());
      cs.push_back(s);
      perm.insert(perm.end(), dr.begin() + i, dr.begin() + std::min(dr.size(), i + CH));
    }
  }
  cb.push_back((uint32_t)perm.size());
  p.spec_wave_begin.push_back((uint32_t)wl.size());
  p.nch = (uint32_t)cs.size();
  p.ndir = (uint32_t)p.dir_ids.size();
  p.nspec = (uint32_t)p.spec_ids.size();
  return 0;
}

// Dword offsets of the plan's arrays in the two packed device buffers, and each buffer's length:
// `chunks` = chunk_begin, chunk_slot; `spec_idx` = dir_ids, spec_ids, spec_wave_begin, wave_list.
struct AccumLayout {
  size_t chunk_begin, chunk_slot, chunks_len;
  size_t dir_ids, spec_ids, spec_wave_begin, wave_list, spec_idx_len;
};
inline AccumLayout accum_layout(const AccumPlan& p) {
  AccumLayout l{};
  l.chunk_begin = 0;
  l.chunk_slot = l.chunk_begin + p.nch + 1;
  l.chunks_len = l.chunk_slot + p.nch;
  l.dir_ids = 0;
  l.spec_ids = l.dir_ids + p.ndir;
  l.spec_wave_begin = l.spec_ids + p.nspec;
  l.wave_list = l.spec_wave_begin + p.nspec + 1;
  l.spec_idx_len = l.wave_list + p.wave_list.size();
  return l;
}

}  // namespace p3g
