// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): the
// counter-based generator behind every dropout mask of the GPT-2 trial (transformer.hip: the
// LayerNorm and embedding sites, contract above drop_words; the attention probabilities, contract
// above attn_tile_words). ops/transformer.py holds the same function in integer torch arithmetic,
// the oracle of the tests.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace katib_hip {
namespace tfm {

typedef unsigned int philox_u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ philox_u32x4 philox4x32_10(philox_u32x4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    c = philox_u32x4{(uint32_t)(p1 >> 32) ^ c[1] ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c[3] ^ k1, (uint32_t)p0};
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}

}  // namespace tfm
}  // namespace katib_hip
