// Dropout for the GPT-2 trial, fused into the residual-add LayerNorm kernels (gfx950).
//
// Every residual-branch output of the flat model (attention proj, MLP fc2) is read once, by the
// residual-add + LayerNorm forward, and its gradient is written once, as the dr output of the
// LayerNorm backward. Dropout on those tensors therefore costs no launch and no memory traffic:
// ln_fwd_drop_k / ln_bwd_drop_k are ln_fwd_k / ln_bwd_k (transformer.hip, left untouched so the
// p = 0 step runs the code it always ran) with the keep mask applied to r on the way in and to dr
// on the way out. Nothing is stored: both directions recompute the mask from a counter-based
// generator, Philox4x32-10, keyed by
//
//     counter = (q & 0xffffffff, q >> 32, site, step),   key = (seed & 0xffffffff, seed >> 32)
//
// for the element index e = row * D + col of a row-major [M, D] tensor with q = e >> 2 (64-bit);
// the element takes output word e & 3 and is kept iff word >= thr = round(p * 2^32); kept values
// are multiplied by scale = 1 / (1 - p). A lane of the LayerNorm kernels owns columns
// 256 i + 4 lane .. + 3, so one Philox call serves exactly one f32x4. `step` is read from device
// memory (the model's optimizer step counter, fp32 like the AdamW kernel reads it), never passed by
// value: a replayed HIP graph draws a fresh mask every step, and the forward and the backward of
// one step see the same value because the counter advances after the backward.
//
// ops/transformer.py holds the same generator in integer torch arithmetic (the oracle of the tests).
// The tests cannot reach the high counter word at their shapes (q >= 2^32 needs 2^34 elements);
// q is formed in 64 bits here and there in the same way: (int64 row * D + col) >> 2.
//
//  * dropout_f32_k   in place over an fp32 [M, D] tensor (the embedding sum and its gradient).
//  * dropout_mask_k  the keep mask itself as bytes (tests only), from the same device function.
#include "transformer.h"
#include "philox.h"

namespace katib_hip {
namespace tfm {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef uint16_t u16;

__device__ __forceinline__ float lo2f(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float hi2f(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }
__device__ __forceinline__ u16 f2bf(float f) { return __builtin_bit_cast(u16, (__bf16)f); }
__device__ __forceinline__ uint32_t pack2(float a, float b) { return (uint32_t)f2bf(a) | ((uint32_t)f2bf(b) << 16); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// (philox4x32_10: philox.h, shared with the attention kernels of transformer.hip)
// The four random words of elements e .. e + 3 (e % 4 == 0) of a dropout site at this step.
__device__ __forceinline__ u32x4 drop_words(int64_t e, const DropSpec& dp, uint32_t step) {
  const uint64_t q = (uint64_t)e >> 2;
  return philox4x32_10(u32x4{(uint32_t)q, (uint32_t)(q >> 32), dp.site, step}, (uint32_t)dp.seed,
                       (uint32_t)(dp.seed >> 32));
}
__device__ __forceinline__ uint32_t drop_step(const DropSpec& dp) { return (uint32_t)*dp.step; }

// ============================================================== LayerNorm forward, r dropped
template <int V>  // D = 256 * V; one wave per row, lane owns columns 256 i + 4 lane .. + 3
__global__ __launch_bounds__(256) void ln_fwd_drop_k(const float* __restrict__ x32, const u16* __restrict__ r,
                                                     float* __restrict__ xo, const u16* __restrict__ gamma,
                                                     const u16* __restrict__ beta, u16* __restrict__ y,
                                                     float* __restrict__ mean, float* __restrict__ rstd, int M,
                                                     float eps, const DropSpec dp) {
  constexpr int D = 256 * V;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const uint32_t step = drop_step(dp);
  const int64_t base = (int64_t)row * D;
  f32x4 v[V];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < V; ++i) {
    const int c = 256 * i + 4 * lane;
    f32x4 t = *reinterpret_cast<const f32x4*>(x32 + base + c);
    const u32x2 rr = *reinterpret_cast<const u32x2*>(r + base + c);
    const u32x4 w = drop_words(base + c, dp, step);
    const f32x4 rv = f32x4{lo2f(rr[0]), hi2f(rr[0]), lo2f(rr[1]), hi2f(rr[1])};
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (w[k] >= dp.thr) t[k] += dp.scale * rv[k];
    *reinterpret_cast<f32x4*>(xo + base + c) = t;
    v[i] = t;
    s += (t[0] + t[1]) + (t[2] + t[3]);
  }
  const float mu = wave_sum(s) * (1.f / D);
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < V; ++i)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float d = v[i][k] - mu;
      q += d * d;
    }
  const float rs = rsqrtf(wave_sum(q) * (1.f / D) + eps);
#pragma unroll
  for (int i = 0; i < V; ++i) {
    const int c = 256 * i + 4 * lane;
    const u32x2 gg = *reinterpret_cast<const u32x2*>(gamma + c);
    const u32x2 bb = *reinterpret_cast<const u32x2*>(beta + c);
    u32x2 o;
    o[0] = pack2((v[i][0] - mu) * rs * lo2f(gg[0]) + lo2f(bb[0]), (v[i][1] - mu) * rs * hi2f(gg[0]) + hi2f(bb[0]));
    o[1] = pack2((v[i][2] - mu) * rs * lo2f(gg[1]) + lo2f(bb[1]), (v[i][3] - mu) * rs * hi2f(gg[1]) + hi2f(bb[1]));
    *reinterpret_cast<u32x2*>(y + base + c) = o;
  }
  if (lane == 0) {
    mean[row] = mu;
    rstd[row] = rs;
  }
}

// ============================================================== LayerNorm backward, dr dropped
// ln_bwd_k with the mask of the branch whose output gradient dr is: dx (the residual-stream
// gradient) is unchanged, dr = keep ? bf16(scale * dx) : 0, and part_r sums those bf16 values.
// Each f32x4's random words are generated right before its store, so they are never live across
// the two rows the wave holds in registers.
template <int V>
__global__ __launch_bounds__(256) void ln_bwd_drop_k(const u16* __restrict__ dy, const float* __restrict__ xin,
                                                     const float* __restrict__ mean, const float* __restrict__ rstd,
                                                     const u16* __restrict__ gamma, const float* dres, float* dx,
                                                     u16* __restrict__ dr, float* __restrict__ part_g,
                                                     float* __restrict__ part_b, float* __restrict__ part_r, int M,
                                                     const DropSpec dp) {
  constexpr int D = 256 * V;
  __shared__ float red[2][4][D];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint32_t step = drop_step(dp);
  f32x4 ag[V], ab[V], ar[V], gv[V];
#pragma unroll
  for (int i = 0; i < V; ++i) {
    ag[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    ab[i] = ag[i];
    ar[i] = ag[i];
    const u32x2 gg = *reinterpret_cast<const u32x2*>(gamma + 256 * i + 4 * lane);
    gv[i] = f32x4{lo2f(gg[0]), hi2f(gg[0]), lo2f(gg[1]), hi2f(gg[1])};
  }
  // two rows per wave per iteration, as ln_bwd_k: both rows' loads issue before either row's reductions
  constexpr int RR = 2;
  const int stride = gridDim.x * 4;
  for (int row0 = blockIdx.x * 4 + w; row0 < M; row0 += RR * stride) {
    f32x4 xh[RR][V], g[RR][V], rd[RR][V];
    float s1[RR], s2[RR], mu[RR], rs[RR];
    bool ok[RR];
#pragma unroll
    for (int r = 0; r < RR; ++r) {
      const int row = row0 + r * stride;
      ok[r] = row < M;
      const int rw = ok[r] ? row : row0;
      const int64_t base = (int64_t)rw * D;
      mu[r] = mean[rw];
      rs[r] = rstd[rw];
#pragma unroll
      for (int i = 0; i < V; ++i) {
        const int c = 256 * i + 4 * lane;
        xh[r][i] = *reinterpret_cast<const f32x4*>(xin + base + c);
        const u32x2 d2 = *reinterpret_cast<const u32x2*>(dy + base + c);
        g[r][i] = f32x4{lo2f(d2[0]), hi2f(d2[0]), lo2f(d2[1]), hi2f(d2[1])};
        rd[r][i] = dres ? *reinterpret_cast<const f32x4*>(dres + base + c) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
#pragma unroll
    for (int r = 0; r < RR; ++r) {
      s1[r] = 0.f;
      s2[r] = 0.f;
#pragma unroll
      for (int i = 0; i < V; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          xh[r][i][k] = (xh[r][i][k] - mu[r]) * rs[r];
          const float dxh = g[r][i][k] * gv[i][k];
          s1[r] += dxh;
          s2[r] += dxh * xh[r][i][k];
          if (ok[r]) {
            ag[i][k] += g[r][i][k] * xh[r][i][k];
            ab[i][k] += g[r][i][k];
          }
        }
    }
#pragma unroll
    for (int r = 0; r < RR; ++r) {
      s1[r] = wave_sum(s1[r]) * (1.f / D);
      s2[r] = wave_sum(s2[r]) * (1.f / D);
    }
#pragma unroll
    for (int r = 0; r < RR; ++r) {
      if (!ok[r]) continue;  // wave-uniform
      const int64_t base = (int64_t)(row0 + r * stride) * D;
#pragma unroll
      for (int i = 0; i < V; ++i) {
        const int c = 256 * i + 4 * lane;
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = rs[r] * (g[r][i][k] * gv[i][k] - s1[r] - xh[r][i][k] * s2[r]);
        o += rd[r][i];
        *reinterpret_cast<f32x4*>(dx + base + c) = o;
        const u32x4 wd = drop_words(base + c, dp, step);
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = wd[k] >= dp.thr ? dp.scale * o[k] : 0.f;
        const u32x2 ob = u32x2{pack2(o[0], o[1]), pack2(o[2], o[3])};
        *reinterpret_cast<u32x2*>(dr + base + c) = ob;
        if (part_r) ar[i] += f32x4{lo2f(ob[0]), hi2f(ob[0]), lo2f(ob[1]), hi2f(ob[1])};  // what colsum(dr) sums
      }
    }
  }
#pragma unroll
  for (int i = 0; i < V; ++i) {
    *reinterpret_cast<f32x4*>(&red[0][w][256 * i + 4 * lane]) = ag[i];
    *reinterpret_cast<f32x4*>(&red[1][w][256 * i + 4 * lane]) = ab[i];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < D; c += 256) {
    part_g[(int64_t)blockIdx.x * D + c] = (red[0][0][c] + red[0][1][c]) + (red[0][2][c] + red[0][3][c]);
    part_b[(int64_t)blockIdx.x * D + c] = (red[1][0][c] + red[1][1][c]) + (red[1][2][c] + red[1][3][c]);
  }
  if (part_r == nullptr) return;  // uniform
  __syncthreads();  // red[0] is reused, as in ln_bwd_k
#pragma unroll
  for (int i = 0; i < V; ++i) *reinterpret_cast<f32x4*>(&red[0][w][256 * i + 4 * lane]) = ar[i];
  __syncthreads();
  for (int c = threadIdx.x; c < D; c += 256)
    part_r[(int64_t)blockIdx.x * D + c] = (red[0][0][c] + red[0][1][c]) + (red[0][2][c] + red[0][3][c]);
}

// ============================================================== element-wise
// one f32x4 (= one Philox call) per thread; n4 = number of f32x4
__global__ __launch_bounds__(256) void dropout_f32_k(float* __restrict__ x, int64_t n4, const DropSpec dp) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= n4) return;
  const u32x4 w = drop_words(4 * q, dp, drop_step(dp));
  f32x4 t = *reinterpret_cast<const f32x4*>(x + 4 * q);
#pragma unroll
  for (int k = 0; k < 4; ++k) t[k] = w[k] >= dp.thr ? dp.scale * t[k] : 0.f;
  *reinterpret_cast<f32x4*>(x + 4 * q) = t;
}

// four mask bytes (1 = keep) per thread, written as one 32-bit word
__global__ __launch_bounds__(256) void dropout_mask_k(uint32_t* __restrict__ out, int64_t n4, const DropSpec dp) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= n4) return;
  const u32x4 w = drop_words(4 * q, dp, drop_step(dp));
  uint32_t m = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) m |= (w[k] >= dp.thr ? 1u : 0u) << (8 * k);
  out[q] = m;
}

}  // namespace

hipError_t ln_fwd_drop(const float* x32, const bf16* r, float* xo, const bf16* gamma, const bf16* beta, bf16* y,
                       float* mean, float* rstd, int M, int D, float eps, const DropSpec& dp, hipStream_t st) {
  if (r == nullptr || xo == nullptr || dp.step == nullptr) return hipErrorInvalidValue;
  const dim3 grid((M + 3) / 4), blk(256);
  const u16* rr = reinterpret_cast<const u16*>(r);
  const u16* gg = reinterpret_cast<const u16*>(gamma);
  const u16* bb = reinterpret_cast<const u16*>(beta);
  u16* yy = reinterpret_cast<u16*>(y);
  switch (D / 256) {
#define LN_CASE(V) \
  case V: hipLaunchKernelGGL(ln_fwd_drop_k<V>, grid, blk, 0, st, x32, rr, xo, gg, bb, yy, mean, rstd, M, eps, dp); break;
    LN_CASE(1) LN_CASE(2) LN_CASE(3) LN_CASE(4) LN_CASE(5) LN_CASE(6) LN_CASE(8)
#undef LN_CASE
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t ln_bwd_drop(const bf16* dy, const float* xin, const float* mean, const float* rstd, const bf16* gamma,
                       const float* dres, float* dx, bf16* dr, float* part_g, float* part_b, int M, int D,
                       const DropSpec& dp, hipStream_t st, float* part_r) {
  if (dr == nullptr || dp.step == nullptr) return hipErrorInvalidValue;
  const dim3 grid(ln_bwd_blocks(M)), blk(256);
  const u16* d = reinterpret_cast<const u16*>(dy);
  const u16* gg = reinterpret_cast<const u16*>(gamma);
  u16* rr = reinterpret_cast<u16*>(dr);
  switch (D / 256) {
#define LN_CASE(V) \
  case V:          \
    hipLaunchKernelGGL(ln_bwd_drop_k<V>, grid, blk, 0, st, d, xin, mean, rstd, gg, dres, dx, rr, part_g, part_b, \
                       part_r, M, dp);                                                                          \
    break;
    LN_CASE(1) LN_CASE(2) LN_CASE(3) LN_CASE(4) LN_CASE(5) LN_CASE(6) LN_CASE(8)
#undef LN_CASE
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t dropout_f32(float* x, int64_t n, const DropSpec& dp, hipStream_t st) {
  const int64_t n4 = n / 4, blocks = (n4 + 255) / 256;
  if (n <= 0 || n % 4 != 0 || blocks >= (1ll << 31) || dp.step == nullptr) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dropout_f32_k, dim3((unsigned)blocks), dim3(256), 0, st, x, n4, dp);
  return hipGetLastError();
}

hipError_t dropout_mask(uint8_t* out, int64_t n, const DropSpec& dp, hipStream_t st) {
  const int64_t n4 = n / 4, blocks = (n4 + 255) / 256;
  if (n <= 0 || n % 4 != 0 || blocks >= (1ll << 31) || dp.step == nullptr) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dropout_mask_k, dim3((unsigned)blocks), dim3(256), 0, st, reinterpret_cast<uint32_t*>(out), n4, dp);
  return hipGetLastError();
}

}  // namespace tfm
}  // namespace katib_hip
