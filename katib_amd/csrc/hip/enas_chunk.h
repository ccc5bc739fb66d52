// Device helpers on 16-byte chunks of eight bf16, shared by the ENAS child's layer-input kernels
// (enas_concat.hip) and its gradient fan-in (enas_fanin.hip). HIP translation units only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace katib_hip {
namespace enaschunk {

// a bf16 widened to fp32 bits is <= 0: zero, or negative and no NaN (integer tests, so the answer
// does not depend on the denormal mode)
__device__ __forceinline__ bool le0(uint32_t f) {
  return (int32_t)f <= 0 && (f & 0x7fffffffu) <= 0x7f800000u;
}

// the loaded chunk is live here: keeps the compiler from sinking a load below another chunk's store
__device__ __forceinline__ void pin(uint4& v) { asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w)); }

// eight bf16 out of the sixteen of (lo, hi), from element S on: a dword rotate for the even part of
// S, v_alignbyte_b32 by two bytes for the odd half-word; S is a constant, so it is all register naming
template <int S>
__device__ __forceinline__ uint4 funnel(const uint4& lo, const uint4& hi) {
  const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  constexpr int d = S >> 1;
  uint32_t r[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    r[j] = (S & 1) ? __builtin_amdgcn_alignbyte(w[(d + j + 1) & 7], w[d + j], 2u) : w[d + j];
  return make_uint4(r[0], r[1], r[2], r[3]);
}

}  // namespace enaschunk
}  // namespace katib_hip
