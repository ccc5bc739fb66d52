// Augmenting batch gather (augment.h): one workgroup per sample, so the sample's index, its Philox
// draw and with them dx, dy and flip are workgroup-uniform - the generator runs once per wave on
// scalar values and the pixel loop sees three scalars.
//
// NCHW fp32 destination: a thread produces 4 consecutive x of every channel - one 16-byte store
// per channel (W % 4 == 0; scalar stores otherwise), and a u8 pixel is one dword load that serves
// all its channels. A flipped row reads the same 4-pixel span in reverse. C8 bf16 destination: a
// thread produces one pixel's 8-channel group, one 16-byte store. The u8 normalisation table
// (C x 256 floats) sits in LDS, filled once per workgroup; an out-of-range pixel reads byte 0 of
// it, which is the fill (the reference pads the raw image with 0 before it normalises).
#include "augment.h"
#include "philox.h"

namespace katib_hip {
namespace aug {
namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint16_t u16;

constexpr int kThreads = 256;

__device__ __forceinline__ u16 f2bf(float f) { return __builtin_bit_cast(u16, (__bf16)f); }

template <int SRC, int DST>
__global__ __launch_bounds__(kThreads) void augment_k(Args a) {
  __shared__ float slut[kLutChannels * 256];  // referenced by the u8 forms only
  const int b = blockIdx.x, tid = threadIdx.x;
  const int C = a.C, H = a.H, W = a.W;
  const int64_t i = a.idx[b];
  const bool ok = i >= 0 && i < a.n_src;
  const int64_t is = ok ? i : 0;
  const uint32_t epoch = a.epoch_ptr ? (uint32_t)*a.epoch_ptr : a.epoch_imm;
  const tfm::philox_u32x4 w = tfm::philox4x32_10(
      tfm::philox_u32x4{(uint32_t)i, (uint32_t)((uint64_t)i >> 32), a.stream, epoch}, a.seed_lo, a.seed_hi);
  const uint32_t k = 2u * (uint32_t)a.pad + 1u;
  // offsets with the padding already taken off: source = destination + (dx, dy)
  const int dx = __builtin_amdgcn_readfirstlane((int)(((uint64_t)w[0] * k) >> 32) - a.pad);
  const int dy = __builtin_amdgcn_readfirstlane((int)(((uint64_t)w[1] * k) >> 32) - a.pad);
  const bool flip = __builtin_amdgcn_readfirstlane((int)(a.flip != 0 && (w[2] >> 31) != 0)) != 0;

  if constexpr (SRC == kSrcU8) {
    for (int j = tid; j < C * 256; j += kThreads) slut[j] = a.lut[j];
    __syncthreads();
  }

  if constexpr (DST == kDstNCHW) {
    const int W4 = (W + 3) >> 2;
    const bool vec = (W & 3) == 0;
    float* out = reinterpret_cast<float*>(a.out) + (int64_t)b * C * H * W;
    for (int t = tid; t < H * W4; t += kThreads) {
      const int y = t / W4, x0 = (t - y * W4) * 4;
      const int sy = y + dy;
      const bool rowok = ok && sy >= 0 && sy < H;
      int sx[4];
      bool in[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int x = x0 + q;
        sx[q] = (flip ? W - 1 - x : x) + dx;
        in[q] = rowok && x < W && sx[q] >= 0 && sx[q] < W;
      }
      if constexpr (SRC == kSrcU8) {
        const uint32_t* row = reinterpret_cast<const uint32_t*>(a.src) + (is * H + (rowok ? sy : 0)) * W;
        uint32_t px[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) px[q] = in[q] ? row[sx[q]] : 0u;
#pragma unroll
        for (int c = 0; c < kLutChannels; ++c) {
          if (c < C) {
            f32x4 v;
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = slut[c * 256 + ((px[q] >> (8 * c)) & 255u)];
            float* o = out + ((int64_t)c * H + y) * W + x0;
            if (vec) {
              *reinterpret_cast<f32x4*>(o) = v;
            } else {
#pragma unroll
              for (int q = 0; q < 4; ++q)
                if (x0 + q < W) o[q] = v[q];
            }
          }
        }
      } else {
        for (int c = 0; c < C; ++c) {
          const float* row = reinterpret_cast<const float*>(a.src) + ((is * C + c) * H + (rowok ? sy : 0)) * W;
          f32x4 v;
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q] = in[q] ? row[sx[q]] : 0.f;
          float* o = out + ((int64_t)c * H + y) * W + x0;
          if (vec) {
            *reinterpret_cast<f32x4*>(o) = v;
          } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
              if (x0 + q < W) o[q] = v[q];
          }
        }
      }
    }
  } else {
    const int C8 = a.C8, G = C8 >> 3;
    u16* out = reinterpret_cast<u16*>(a.out) + (int64_t)b * H * W * C8;
    for (int t = tid; t < H * W * G; t += kThreads) {
      const int p = t / G, g = t - p * G;
      const int y = p / W, x = p - y * W;
      const int sy = y + dy, sx = (flip ? W - 1 - x : x) + dx;
      const bool in = ok && sy >= 0 && sy < H && sx >= 0 && sx < W;
      const int64_t sp = in ? (is * H + sy) * W + sx : 0;  // source pixel
      u16 v[8];
      if constexpr (SRC == kSrcU8) {
        const uint32_t px = in ? reinterpret_cast<const uint32_t*>(a.src)[sp] : 0u;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int c = g * 8 + q;
          v[q] = c < C ? f2bf(slut[(c & 3) * 256 + ((px >> (8 * (c & 3))) & 255u)]) : (u16)0;
        }
      } else {
        const u16* s = reinterpret_cast<const u16*>(a.src) + sp * C;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int c = g * 8 + q;
          v[q] = (in && c < C) ? s[c] : (u16)0;
        }
      }
      *reinterpret_cast<u32x4*>(out + (int64_t)t * 8) =
          u32x4{v[0] | ((uint32_t)v[1] << 16), v[2] | ((uint32_t)v[3] << 16), v[4] | ((uint32_t)v[5] << 16),
                v[6] | ((uint32_t)v[7] << 16)};
    }
  }
}

template <int SRC, int DST>
hipError_t run(const Args& a, hipStream_t st) {
  hipLaunchKernelGGL((augment_k<SRC, DST>), dim3((unsigned)a.B), dim3(kThreads), 0, st, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch(int src_kind, int dst_kind, const Args& a, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  if (a.pad < 0 || a.pad > kMaxPad || a.C < 1 || a.H < 1 || a.W < 1) return hipErrorInvalidValue;
  if (src_kind == kSrcU8 && (a.C > kLutChannels || a.lut == nullptr)) return hipErrorInvalidValue;
  if (dst_kind == kDstC8 && (a.C8 % 8 != 0 || a.C8 < a.C)) return hipErrorInvalidValue;
  if (src_kind == kSrcU8 && dst_kind == kDstNCHW) return run<kSrcU8, kDstNCHW>(a, st);
  if (src_kind == kSrcF32 && dst_kind == kDstNCHW) return run<kSrcF32, kDstNCHW>(a, st);
  if (src_kind == kSrcU8 && dst_kind == kDstC8) return run<kSrcU8, kDstC8>(a, st);
  if (src_kind == kSrcBf16 && dst_kind == kDstC8) return run<kSrcBf16, kDstC8>(a, st);
  return hipErrorInvalidValue;
}

}  // namespace aug
}  // namespace katib_hip
