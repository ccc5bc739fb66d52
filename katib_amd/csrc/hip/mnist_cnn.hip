// Fused MNIST CNN training kernels for gfx950 (the reference's pytorch-mnist trial: conv 1->20 5x5,
// pool, conv 20->50 5x5, pool, fc 800->500, fc 500->10). The two linear layers and the cross-entropy run
// on mlp.hip; this file is the convolution part. bf16 operands, fp32 accumulation, fp32 masters.
//
//  conv1_pool_fwd_k   one image per workgroup, K = 25 is too thin for MFMA: fp32 VALU from an LDS image
//                     and LDS weights; a thread owns one pooled pixel x 8 channels (4 window positions x 8
//                     accumulators), adds the bias, applies ReLU, takes the 2x2 maximum on the fp32 values
//                     (first maximum wins) and stores 16 bytes of p1 and 8 winner bytes.
//  conv2_pool_fwd_k   implicit GEMM on v_mfma_f32_16x16x32_bf16, one image per workgroup: M = 64 output
//                     pixels, N = 64 (50), K = 608 (600). A fragments straight from the image's 12x12x24
//                     LDS patch (a filter row's 5 taps x 24 channels are 120 contiguous elements = 15
//                     chunks of 8), B fragments from the [64][608] shadow. Accumulator row 4q + i of M tile
//                     t is window position i of pooled pixel (t, q), so one lane's four registers are one
//                     pooling window: bias, ReLU, maximum and winner need no cross-lane traffic.
//  conv2_dgrad_k      the same MFMA form, M = 144 input pixels, N = 32 (24), K = 25 taps x 64 channels.
//                     dz2 (dp2 at each window's winner, zero elsewhere) exists only as a zero-haloed
//                     16x16x64 LDS tile; the epilogue masks with p1 > 0.
//  conv2_wgrad_part_k / conv2_sgd_k   per (channel, 8-image slice) partial sums over the 16 winners of
//                     each image, then one fixed-order sum over the slices with momentum SGD and both
//                     shadows re-emitted. conv1_wgrad_part_k / conv1_sgd_k: the same for conv1.
// No atomics: every reduction runs in a fixed order, so a step is bit-reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mnist_cnn.h"

namespace katib_hip {
namespace cnn {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float bf2f(u16 b) { return __uint_as_float((uint32_t)b << 16); }
__device__ __forceinline__ u16 f2bf(float f) { return __builtin_bit_cast(u16, (__bf16)f); }

// maximum of a window's four values after ReLU, first maximum in row-major order wins
__device__ __forceinline__ float pool4(float v0, float v1, float v2, float v3, int& win) {
  float best = fmaxf(v0, 0.f);
  win = 0;
  v1 = fmaxf(v1, 0.f);
  v2 = fmaxf(v2, 0.f);
  v3 = fmaxf(v3, 0.f);
  if (v1 > best) { best = v1; win = 1; }
  if (v2 > best) { best = v2; win = 2; }
  if (v3 > best) { best = v3; win = 3; }
  return best;
}

// ------------------------------------------------------------------ conv1 + bias + ReLU + pool
__global__ __launch_bounds__(448) void conv1_pool_fwd_k(const u16* __restrict__ x, const int64_t* __restrict__ idx,
                                                        const u16* __restrict__ w1s, const float* __restrict__ b1,
                                                        u16* __restrict__ p1, uint8_t* __restrict__ a1) {
  __shared__ float img[IMG];
  __shared__ float wl[25 * C1];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int64_t row = idx ? idx[b] : b;
  for (int i = tid; i < IMG; i += 448) img[i] = bf2f(x[row * IMG + i]);
  for (int i = tid; i < 25 * C1; i += 448) wl[i] = bf2f(w1s[i]);
  __syncthreads();
  if (tid >= P1 * 3) return;
  const int pp = tid / 3, cg = tid % 3, py = pp / 12, px = pp % 12;
  float patch[6][6];
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j < 6; ++j) patch[i][j] = img[(2 * py + i) * 28 + 2 * px + j];
  float acc[4][8];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[i][c] = 0.f;
#pragma unroll
  for (int r = 0; r < 5; ++r)
#pragma unroll
    for (int s = 0; s < 5; ++s) {
      const float* wp = wl + (r * 5 + s) * C1 + cg * 8;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const float w = wp[c];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i][c] += patch[(i >> 1) + r][(i & 1) + s] * w;
      }
    }
  uint32_t out[4], wins[2] = {0u, 0u};
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const float bv = b1[cg * 8 + c];
    int win;
    const float v = pool4(acc[0][c] + bv, acc[1][c] + bv, acc[2][c] + bv, acc[3][c] + bv, win);
    const uint32_t h = f2bf(v);
    if (c & 1) out[c >> 1] |= h << 16; else out[c >> 1] = h;
    wins[c >> 2] |= (uint32_t)win << (8 * (c & 3));
  }
  const int64_t o = ((int64_t)b * P1 + pp) * C1 + cg * 8;
  *reinterpret_cast<u32x4*>(p1 + o) = u32x4{out[0], out[1], out[2], out[3]};
  if (a1) *reinterpret_cast<u32x2*>(a1 + o) = u32x2{wins[0], wins[1]};
}

// ------------------------------------------------------------------ conv2 + bias + ReLU + pool
__global__ __launch_bounds__(256) void conv2_pool_fwd_k(const u16* __restrict__ p1, const u16* __restrict__ w2f,
                                                        const float* __restrict__ b2, u16* __restrict__ p2,
                                                        uint8_t* __restrict__ a2) {
  __shared__ __align__(16) u16 patch[P1 * C1];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const u32x4* src = reinterpret_cast<const u32x4*>(p1 + (int64_t)b * P1 * C1);
  for (int i = tid; i < P1 * C1 / 8; i += 256) reinterpret_cast<u32x4*>(patch)[i] = src[i];
  __syncthreads();
  const int fr = lane & 15, fq = lane >> 4;
  // A row fr of M tile t: window position i = fr & 3 of pooled pixel (t, fr >> 2)
  const int ax = 2 * (fr >> 2) + (fr & 1), ay = (fr >> 1) & 1;
  const u16* brow = w2f + (int64_t)(wave * 16 + fr) * K2P + 8 * fq;
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < K2P / 32; ++ks) {
    const bf16x8 bf = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(brow + ks * 32));
    int c = ks * 4 + fq;       // chunk of 8 along k = (r, s, ci); 15 chunks per filter row
    if (c >= 75) c = 0;        // k >= 600: the shadow is zero there, read any finite A
    const int r = c / 15, off = (c % 15) * 8;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int y = 2 * t + ay;
      const bf16x8 af = __builtin_bit_cast(
          bf16x8, *reinterpret_cast<const u32x4*>(patch + ((y + r) * 12 + ax) * C1 + off));
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf, acc[t], 0, 0, 0);
    }
  }
  // lane: channel n, accumulator rows 4 fq + j = the four positions of pooled pixel (t, fq)
  const int n = wave * 16 + fr;
  if (n >= CO) return;
  const float bv = b2[n];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    int win;
    const float v = pool4(acc[t][0] + bv, acc[t][1] + bv, acc[t][2] + bv, acc[t][3] + bv, win);
    const int64_t o = (int64_t)b * F2 + (t * 4 + fq) * CO + n;
    p2[o] = f2bf(v);
    if (a2) a2[o] = (uint8_t)win;
  }
}

// ------------------------------------------------------------------ conv2 data gradient
__global__ __launch_bounds__(256) void conv2_dgrad_k(const u16* __restrict__ dp2, const uint8_t* __restrict__ a2,
                                                     const u16* __restrict__ w2d, const u16* __restrict__ p1,
                                                     u16* __restrict__ dp1) {
  __shared__ __align__(16) u16 dz[16 * 16 * N2];  // output pixel (oy, ox) at (oy + 4, ox + 4), zero halo
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const u32x4 zero = {0u, 0u, 0u, 0u};
  for (int i = tid; i < 16 * 16 * N2 / 8; i += 256) reinterpret_cast<u32x4*>(dz)[i] = zero;
  __syncthreads();
  for (int e = tid; e < F2; e += 256) {
    const int pp = e / CO, co = e % CO;
    const int a = a2[(int64_t)b * F2 + e] & 3;
    const int oy = 2 * (pp >> 2) + (a >> 1), ox = 2 * (pp & 3) + (a & 1);
    dz[((oy + 4) * 16 + ox + 4) * N2 + co] = dp2[(int64_t)b * F2 + e];
  }
  __syncthreads();
  const int fr = lane & 15, fq = lane >> 4;
  // wave w owns M tiles w, w + 4 and (wave 0 only) 8: 9 tiles of 16 input pixels
  const int nmt = wave == 0 ? 3 : 2;
  int abase[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int px = min((wave + 4 * i) * 16 + fr, P1 - 1);
    abase[i] = ((px / 12 + 4) * 16 + px % 12 + 4) * N2 + 8 * fq;
  }
  const bool bok1 = 16 + fr < C1;
  const u16* brow0 = w2d + (int64_t)fr * KD + 8 * fq;
  const u16* brow1 = w2d + (int64_t)(bok1 ? 16 + fr : 0) * KD + 8 * fq;
  f32x4 acc[3][2];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 5
  for (int ks = 0; ks < KD / 32; ++ks) {
    const int tap = ks >> 1, r = tap / 5, s = tap % 5, ko = (ks & 1) * 32;
    const bf16x8 b0 = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(brow0 + tap * N2 + ko));
    const bf16x8 b1 = __builtin_bit_cast(
        bf16x8, bok1 ? *reinterpret_cast<const u32x4*>(brow1 + tap * N2 + ko) : zero);
    const int aoff = ko - (r * 16 + s) * N2;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      if (i < nmt) {
        const bf16x8 af = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(dz + abase[i] + aoff));
        acc[i][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, b0, acc[i][0], 0, 0, 0);
        acc[i][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, b1, acc[i][1], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    if (i >= nmt) continue;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = j * 16 + fr;
      if (n >= C1) continue;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int px = (wave + 4 * i) * 16 + 4 * fq + q;
        const int64_t o = ((int64_t)b * P1 + px) * C1 + n;
        dp1[o] = bf2f(p1[o]) > 0.f ? f2bf(acc[i][j][q]) : (u16)0;
      }
    }
  }
}

// ------------------------------------------------------------------ conv2 weight gradient
// grid (50 channels, slices of WG2_IMGS images); thread t < 600: weight (tap, ci) = (t / 24, t % 24),
// t == 600: the bias. Only each window's winner carries a gradient: 16 terms per image and channel.
__global__ __launch_bounds__(640) void conv2_wgrad_part_k(const u16* __restrict__ dp2,
                                                          const uint8_t* __restrict__ a2,
                                                          const u16* __restrict__ p1, float* __restrict__ part,
                                                          int B) {
  const int co = blockIdx.x, sl = blockIdx.y, t = threadIdx.x;
  if (t > K2) return;
  const int tap = t / C1, ci = t % C1, r = tap / 5, s = tap % 5;
  const bool isw = t < K2;
  const int toff = isw ? (r * 12 + s) * C1 + ci : 0;
  float acc = 0.f;
  const int bend = min((sl + 1) * WG2_IMGS, B);
  for (int b = sl * WG2_IMGS; b < bend; ++b) {
    const u16* gp = dp2 + (int64_t)b * F2 + co;
    const uint8_t* ap = a2 + (int64_t)b * F2 + co;
    const u16* xp = p1 + (int64_t)b * P1 * C1 + toff;
    float g[P2], xv[P2];
#pragma unroll
    for (int pp = 0; pp < P2; ++pp) {
      g[pp] = bf2f(gp[pp * CO]);
      const int a = ap[pp * CO] & 3;
      const int oy = 2 * (pp >> 2) + (a >> 1), ox = 2 * (pp & 3) + (a & 1);
      xv[pp] = isw ? bf2f(xp[(oy * 12 + ox) * C1]) : 1.f;
    }
#pragma unroll
    for (int pp = 0; pp < P2; ++pp) acc += g[pp] * xv[pp];
  }
  part[((int64_t)sl * CO + co) * PART2_LD + t] = acc;
}

// one thread per weight / bias: sums the slices in order, applies momentum SGD (torch: buf = m buf + g;
// w -= lr buf) and re-emits the forward shadow [64][608] and the dgrad shadow [24][25][64]
__global__ __launch_bounds__(256) void conv2_sgd_k(const float* __restrict__ part, int slices,
                                                   float* __restrict__ w2, float* __restrict__ w2m,
                                                   float* __restrict__ b2, float* __restrict__ b2m,
                                                   u16* __restrict__ w2f, u16* __restrict__ w2d,
                                                   const float* __restrict__ lr_p, float mom) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int co = e / PART2_LD, t = e % PART2_LD;
  if (co >= CO || t > K2) return;
  float g = 0.f;
  for (int s = 0; s < slices; ++s) g += part[((int64_t)s * CO + co) * PART2_LD + t];
  const float lr = lr_p[0];
  if (t < K2) {
    const int o = co * K2 + t;
    const float mb = mom * w2m[o] + g;
    const float p = w2[o] - lr * mb;
    w2m[o] = mb;
    w2[o] = p;
    const u16 pb = f2bf(p);
    w2f[co * K2P + t] = pb;
    w2d[(t % C1) * KD + (t / C1) * N2 + co] = pb;
  } else {
    const float mb = mom * b2m[co] + g;
    b2m[co] = mb;
    b2[co] -= lr * mb;
  }
}

// ------------------------------------------------------------------ conv1 weight gradient
// grid: slices of WG1_IMGS images; thread t < 624: channel c = t / 26, tap t % 26 (25: the bias).
__global__ __launch_bounds__(640) void conv1_wgrad_part_k(const u16* __restrict__ dp1,
                                                          const uint8_t* __restrict__ a1,
                                                          const u16* __restrict__ x, const int64_t* __restrict__ idx,
                                                          float* __restrict__ part, int B) {
  __shared__ float img[IMG];
  __shared__ float gl[P1 * C1];
  __shared__ uint8_t al[P1 * C1];
  const int sl = blockIdx.x, t = threadIdx.x;
  const int c = min(t / 26, C1 - 1), tp = t % 26, r = tp / 5, s = tp % 5;
  const bool isw = tp < 25;
  const int toff = isw ? r * 28 + s : 0;
  float acc = 0.f;
  const int bend = min((sl + 1) * WG1_IMGS, B);
  for (int b = sl * WG1_IMGS; b < bend; ++b) {
    const int64_t row = idx ? idx[b] : b;
    for (int i = t; i < IMG; i += 640) img[i] = bf2f(x[row * IMG + i]);
    for (int i = t; i < P1 * C1; i += 640) {
      gl[i] = bf2f(dp1[(int64_t)b * P1 * C1 + i]);
      al[i] = a1[(int64_t)b * P1 * C1 + i];
    }
    __syncthreads();
    for (int pp = 0; pp < P1; ++pp) {
      const float g = gl[pp * C1 + c];
      const int a = al[pp * C1 + c] & 3;
      const int py = pp / 12, px = pp % 12;
      const float xv = isw ? img[(2 * py + (a >> 1)) * 28 + 2 * px + (a & 1) + toff] : 1.f;
      acc += g * xv;
    }
    __syncthreads();
  }
  if (t < C1 * 26) part[(int64_t)sl * PART1_LD + t] = acc;
}

__global__ __launch_bounds__(640) void conv1_sgd_k(const float* __restrict__ part, int slices,
                                                   float* __restrict__ w1, float* __restrict__ w1m,
                                                   float* __restrict__ b1, float* __restrict__ b1m,
                                                   u16* __restrict__ w1s, const float* __restrict__ lr_p,
                                                   float mom) {
  const int t = threadIdx.x;
  if (t >= C1 * 26) return;
  const int c = t / 26, tp = t % 26;
  float g = 0.f;
  for (int s = 0; s < slices; ++s) g += part[(int64_t)s * PART1_LD + t];
  const float lr = lr_p[0];
  if (tp < 25) {
    const int o = c * 25 + tp;
    const float mb = mom * w1m[o] + g;
    const float p = w1[o] - lr * mb;
    w1m[o] = mb;
    w1[o] = p;
    w1s[tp * C1 + c] = f2bf(p);
  } else {
    const float mb = mom * b1m[c] + g;
    b1m[c] = mb;
    b1[c] -= lr * mb;
  }
}

}  // namespace

hipError_t conv1_pool_fwd(const u16* x, const int64_t* idx, const u16* w1s, const float* b1, u16* p1, uint8_t* a1,
                          int B, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(conv1_pool_fwd_k, dim3(B), dim3(448), 0, st, x, idx, w1s, b1, p1, a1);
  return hipGetLastError();
}

hipError_t conv2_pool_fwd(const u16* p1, const u16* w2f, const float* b2, u16* p2, uint8_t* a2, int B,
                          hipStream_t st) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(conv2_pool_fwd_k, dim3(B), dim3(256), 0, st, p1, w2f, b2, p2, a2);
  return hipGetLastError();
}

hipError_t conv2_dgrad(const u16* dp2, const uint8_t* a2, const u16* w2d, const u16* p1, u16* dp1, int B,
                       hipStream_t st) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(conv2_dgrad_k, dim3(B), dim3(256), 0, st, dp2, a2, w2d, p1, dp1);
  return hipGetLastError();
}

hipError_t conv2_wgrad_sgd(const u16* dp2, const uint8_t* a2, const u16* p1, float* part, float* w2, float* w2m,
                           float* b2, float* b2m, u16* w2f, u16* w2d, const float* lr, float momentum, int B,
                           hipStream_t st) {
  if (B <= 0) return hipSuccess;
  const int slices = wg2_slices(B);
  hipLaunchKernelGGL(conv2_wgrad_part_k, dim3(CO, slices), dim3(640), 0, st, dp2, a2, p1, part, B);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(conv2_sgd_k, dim3((CO * PART2_LD + 255) / 256), dim3(256), 0, st, part, slices, w2, w2m, b2,
                     b2m, w2f, w2d, lr, momentum);
  return hipGetLastError();
}

hipError_t conv1_wgrad_sgd(const u16* dp1, const uint8_t* a1, const u16* x, const int64_t* idx, float* part,
                           float* w1, float* w1m, float* b1, float* b1m, u16* w1s, const float* lr, float momentum,
                           int B, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  const int slices = wg1_slices(B);
  hipLaunchKernelGGL(conv1_wgrad_part_k, dim3(slices), dim3(640), 0, st, dp1, a1, x, idx, part, B);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(conv1_sgd_k, dim3(1), dim3(640), 0, st, part, slices, w1, w1m, b1, b1m, w1s, lr, momentum);
  return hipGetLastError();
}

}  // namespace cnn
}  // namespace katib_hip
