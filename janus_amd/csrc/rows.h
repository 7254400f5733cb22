// The strided views of per-report device arrays that kernels take by value and the engine's state
// keeps between calls.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef DEVI
#define DEVI __device__ __forceinline__
#endif

namespace p3g {

// A per-report byte array: element r at base + r*stride.
struct Rows {
  uint8_t* base;
  size_t stride;
  DEVI uint8_t* at(size_t r) const { return base + r * stride; }
};
struct CRows {
  const uint8_t* base;
  size_t stride;
  DEVI const uint8_t* at(size_t r) const { return base + r * stride; }
};

// FLP weight matrix (k_flp_weights* -> k_flp_wires): element e of report r at base + r rs + e es
// (row-major: rs = row bytes, es = ES).
struct WMat {
  uint8_t* base;
  size_t rs, es;
  DEVI uint8_t* el(size_t r, uint32_t e) const { return base + r * rs + (size_t)e * es; }
};

}  // namespace p3g
