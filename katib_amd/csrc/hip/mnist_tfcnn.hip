// Fused kernels of the Keras MNIST CNN trial for gfx950 (the reference's tf-mnist-with-summaries trial:
// Conv2D(32, 3, relu) -> Flatten -> Dense(128, relu) -> Dense(10)). The two linear layers and the
// cross-entropy run on mlp.hip; this file is the convolution. bf16 operands, fp32 accumulation, fp32 masters.
//
//  conv_fwd_k          a quarter image (169 output pixels) per workgroup. K = 9 is far too thin for MFMA:
//                      fp32 VALU from an LDS copy of the image; a thread keeps the 72 weights and 8 biases
//                      of its 8 channels in registers and owns one pixel x 8 channels at a time. Bias and
//                      ReLU on the fp32 accumulator, then one 16-byte store. z is pixel-major, channel-minor:
//                      Keras' Flatten order, so z viewed as [B][21632] is fc1's input as it stands.
//  conv_wgrad_part_k   the same quarter image per workgroup: dz chunk and image in LDS, thread (channel,
//                      pixel group of 8) accumulates its 9 taps + the bias over ~21 pixels, the 8 pixel groups
//                      are summed in order -> one partial of 320 values per workgroup.
//  conv_opt_k<E>       one workgroup: sums the 4 B partials of every weight / bias in a fixed order (three
//                      contiguous thirds side by side) and applies the optimizer (E = float: momentum SGD;
//                      E = Adam2: mlp_optim.h AdamUpd), re-emitting the shadow.
// No atomics: every reduction runs in a fixed order, so a step is bit-reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "mlp_optim.h"
#include "mnist_tfcnn.h"

namespace katib_hip {
namespace tfcnn {
namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float bf2f(u16 b) { return __uint_as_float((uint32_t)b << 16); }
__device__ __forceinline__ u16 f2bf(float f) { return __builtin_bit_cast(u16, (__bf16)f); }

// 8 bf16 of a 16-byte chunk -> 8 floats
__device__ __forceinline__ void unpack8(const u32x4 v, float* out) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    out[2 * i] = __uint_as_float(v[i] << 16);
    out[2 * i + 1] = __uint_as_float(v[i] & 0xffff0000u);
  }
}

// the image of a workgroup into LDS as fp32: 98 chunks of 8 pixels, threads 0..97
__device__ __forceinline__ void stage_image(const u16* __restrict__ xrow, float* img, int tid) {
  if (tid < IMG / 8) unpack8(*reinterpret_cast<const u32x4*>(xrow + tid * 8), img + tid * 8);
}

// ------------------------------------------------------------------ conv + bias + ReLU
__global__ __launch_bounds__(256) void conv_fwd_k(const u16* __restrict__ x, const int64_t* __restrict__ idx,
                                                  const u16* __restrict__ ws, const float* __restrict__ bias,
                                                  u16* __restrict__ z) {
  __shared__ __align__(16) float img[IMG];
  __shared__ __align__(16) float wl[9 * C];
  const int b = blockIdx.x / SPLIT, ch = blockIdx.x % SPLIT, tid = threadIdx.x, cg = tid & 3;
  const int64_t row = idx ? idx[b] : b;
  float bv[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) bv[c] = bias[cg * 8 + c];
  stage_image(x + row * IMG, img, tid);
  if (tid >= 128 && tid < 128 + 9 * C / 8)  // the shadow: 36 chunks of 8, on the waves that load no pixels
    unpack8(*reinterpret_cast<const u32x4*>(ws + (tid - 128) * 8), wl + (tid - 128) * 8);
  __syncthreads();
  float w[9][8];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int c = 0; c < 8; ++c) w[t][c] = wl[t * C + cg * 8 + c];
  // item = (pixel of the chunk, group of 8 channels): 4 consecutive lanes write one pixel's 64 bytes
  for (int it = tid; it < CHUNK * 4; it += 256) {
    const int p = ch * CHUNK + (it >> 2), py = p / OW, px = p % OW;
    float patch[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) patch[t] = img[(py + t / 3) * 28 + px + t % 3];
    float acc[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int c = 0; c < 8; ++c) acc[c] += patch[t] * w[t][c];
    uint32_t out[4];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const uint32_t h = f2bf(fmaxf(acc[c] + bv[c], 0.f));
      if (c & 1) out[c >> 1] |= h << 16; else out[c >> 1] = h;
    }
    *reinterpret_cast<u32x4*>(z + ((int64_t)b * PIX + p) * C + cg * 8) = u32x4{out[0], out[1], out[2], out[3]};
  }
}

// ------------------------------------------------------------------ weight gradient: partials
__global__ __launch_bounds__(256) void conv_wgrad_part_k(const u16* __restrict__ dz, const u16* __restrict__ x,
                                                         const int64_t* __restrict__ idx, float* __restrict__ part) {
  constexpr int GCH = CHUNK * C / 8;  // 676 chunks of 16 bytes
  __shared__ __align__(16) float img[IMG];
  __shared__ __align__(16) u16 gl[CHUNK * C];
  __shared__ float red[8][NPART];
  const int b = blockIdx.x / SPLIT, ch = blockIdx.x % SPLIT, tid = threadIdx.x;
  const int64_t row = idx ? idx[b] : b;
  const u32x4* src = reinterpret_cast<const u32x4*>(dz + ((int64_t)b * PIX + ch * CHUNK) * C);
  u32x4 g[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int j = tid + 256 * i;
    g[i] = j < GCH ? src[j] : u32x4{0u, 0u, 0u, 0u};
  }
  stage_image(x + row * IMG, img, tid);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int j = tid + 256 * i;
    if (j < GCH) reinterpret_cast<u32x4*>(gl)[j] = g[i];
  }
  __syncthreads();
  const int c = tid & 31, pg = tid >> 5;
  float acc[10];
#pragma unroll
  for (int t = 0; t < 10; ++t) acc[t] = 0.f;
  for (int q = pg; q < CHUNK; q += 8) {
    const int p = ch * CHUNK + q, base = (p / OW) * 28 + p % OW;
    const float gv = bf2f(gl[q * C + c]);
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t] += gv * img[base + (t / 3) * 28 + t % 3];
    acc[9] += gv;
  }
#pragma unroll
  for (int t = 0; t < 10; ++t) red[pg][c * 10 + t] = acc[t];
  __syncthreads();
  for (int e = tid; e < NPART; e += 256) {
    float s = red[0][e];
#pragma unroll
    for (int k = 1; k < 8; ++k) s += red[k][e];
    part[(int64_t)blockIdx.x * NPART + e] = s;
  }
}

// Adam as the kernel's last argument: the element update and the second state arrays
struct Adam2 {
  mlp::AdamUpd upd;
  float* s1;
  float* bs1;
};

// ------------------------------------------------------------------ weight gradient: sum + optimizer
// One workgroup of OPT_GROUPS x 320 threads. Thread (group, e) sums its group's contiguous third of the
// slices in slice order, 16 loads in flight at a time (a single serial chain over the 4 B slices is bound
// by load latency); group 0 then adds the groups' sums in group order and applies the optimizer to element
// e: channel e / 10, tap e % 10 (9: the bias). w / s0 [32][9], b / bs0 [32], ws [9][32]. The order is fixed
// by B alone, so two runs give identical bits.
constexpr int OPT_GROUPS = 3;

template <class E>
__global__ __launch_bounds__(NPART* OPT_GROUPS) void conv_opt_k(const float* __restrict__ part, int slices,
                                                                float* __restrict__ w, float* __restrict__ s0,
                                                                float* __restrict__ b, float* __restrict__ bs0,
                                                                u16* __restrict__ ws, const float* __restrict__ lr_p,
                                                                E e) {
  __shared__ float red[OPT_GROUPS][NPART];
  const int grp = threadIdx.x / NPART, t = threadIdx.x % NPART, c = t / 10, tp = t % 10;
  const bool isw = tp < 9;
  float* wp = isw ? w + c * 9 + tp : b + c;
  float* s0p = isw ? s0 + c * 9 + tp : bs0 + c;
  float* s1p = nullptr;
  float lr = 0.f, wv = 0.f, s0v = 0.f, s1v = 0.f;
  if (grp == 0) {  // the element's master and state: loads that wait for nothing, out before the sums
    lr = lr_p[0];
    wv = *wp;
    s0v = *s0p;
    if constexpr (!std::is_same<E, float>::value) {
      s1p = isw ? e.s1 + c * 9 + tp : e.bs1 + c;
      s1v = *s1p;
    }
  }
  const int per = (slices + OPT_GROUPS - 1) / OPT_GROUPS;
  const int sb = grp * per, se = min(sb + per, slices);
  float g = 0.f;
  for (int s = sb; s < se; s += 16) {
    float v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = s + i < se ? part[(int64_t)(s + i) * NPART + t] : 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) g += v[i];
  }
  red[grp][t] = g;
  __syncthreads();
  if (grp != 0) return;
  g = red[0][t];
#pragma unroll
  for (int k = 1; k < OPT_GROUPS; ++k) g += red[k][t];
  float p;
  if constexpr (std::is_same<E, float>::value) {
    // SGD with momentum (torch semantics, dampening 0): buf = mom * buf + g; p -= lr * buf
    s0v = e * s0v + g;
    p = wv - lr * s0v;
  } else {
    mlp::AdamUpd upd = e.upd;
    upd.init(lr);
    p = upd(g, s0v, s1v, wv);
    *s1p = s1v;
  }
  *s0p = s0v;
  *wp = p;
  if (isw) ws[tp * C + c] = f2bf(p);
}

hipError_t wgrad_part(const u16* dz, const u16* x, const int64_t* idx, float* part, int B, hipStream_t st) {
  hipLaunchKernelGGL(conv_wgrad_part_k, dim3(B * SPLIT), dim3(256), 0, st, dz, x, idx, part);
  return hipGetLastError();
}

}  // namespace

hipError_t conv_fwd(const u16* x, const int64_t* idx, const u16* ws, const float* b, u16* z, int B, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(conv_fwd_k, dim3(B * SPLIT), dim3(256), 0, st, x, idx, ws, b, z);
  return hipGetLastError();
}

hipError_t conv_wgrad_sgd(const u16* dz, const u16* x, const int64_t* idx, float* part, float* w, float* wm, float* b,
                          float* bm, u16* ws, const float* lr, float momentum, int B, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  const hipError_t e = wgrad_part(dz, x, idx, part, B, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(conv_opt_k<float>, dim3(1), dim3(NPART * OPT_GROUPS), 0, st, part, B * SPLIT, w, wm, b, bm, ws, lr, momentum);
  return hipGetLastError();
}

hipError_t conv_wgrad_adam(const u16* dz, const u16* x, const int64_t* idx, float* part, float* w, float* m, float* v,
                           float* b, float* bm, float* bv, u16* ws, const float* lr, const int* step_t, float beta1,
                           float beta2, float eps, int B, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  const hipError_t e = wgrad_part(dz, x, idx, part, B, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(conv_opt_k<Adam2>, dim3(1), dim3(NPART * OPT_GROUPS), 0, st, part, B * SPLIT, w, m, b, bm, ws, lr,
                     Adam2{mlp::AdamUpd{beta1, beta2, eps, step_t, 0.f, 0.f}, v, bv});
  return hipGetLastError();
}

}  // namespace tfcnn
}  // namespace katib_hip
