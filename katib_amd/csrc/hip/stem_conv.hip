// DARTS stem convolution (model.py:90-93 in the reference's darts-cnn-cifar10 trial:
// Conv2d(3, C_stem, 3, padding=1, bias=False)) as two direct kernels for gfx950.
//
// With 3 input channels the conv is a K=27 reduction - far too thin for MFMA tiles and
// a poor fit for the library's fp32 Winograd kernels (0.43 ms / 5 ms launches in eager
// traces, plus find-mode tuning on first use). Neither direction is near the memory system's
// limit on 128x3x32x32 -> 4 channels (3.6 MB forward, 5.8 MB weight gradient: 1-2 us of traffic
// at the 3 TB/s the edge kernels reach): the cost is instruction issue and the cross-lane
// reductions. Measured per call at that shape (profiles/darts_ends_bench_ab.txt): forward +
// statistics 6.7 us, weight gradient 9.1 us + 4.9 us chunk sum.
//   forward: one thread per output pixel keeps its 27-value input patch in registers
//            and sweeps every output channel against a weight slab broadcast from LDS;
//            stores are coalesced along W for each output plane. The BN statistics of four
//            channels at a time leave the wave through one reduce-scatter.
//   wgrad:   grid (pixel chunk, group of kCG output channels); each thread loads the patch of a
//            pixel once and accumulates the kCG * 27 partial products in registers, a butterfly
//            reduce-scatter + LDS folds the 4 waves, and a second launch (one wave per weight)
//            sums the chunk partials in a fixed order (deterministic, no float atomics).
// The input image never needs a gradient, so there is no data-gradient kernel.
#include "darts_ops_dev.h"  // kRep, wave_reduce_scatter
#include "stem_conv.h"

namespace katib_hip {
namespace stem {
namespace {

constexpr int kThreads = 256;

template <int CIN>
__device__ __forceinline__ void load_patch(const float* __restrict__ x, int n, int h, int w, int H, int W,
                                           float (&v)[CIN * 9]) {
#pragma unroll
  for (int ci = 0; ci < CIN; ++ci) {
    const float* plane = x + ((size_t)n * CIN + ci) * H * W;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int hh = h + kh - 1;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int ww = w + kw - 1;
        const bool in = hh >= 0 && hh < H && ww >= 0 && ww < W;
        v[ci * 9 + kh * 3 + kw] = in ? plane[hh * W + ww] : 0.f;
      }
    }
  }
}

template <int CIN>
__global__ __launch_bounds__(kThreads) void stem_fwd_kernel(const float* __restrict__ x, const float* __restrict__ wt,
                                                             float* __restrict__ y, int N, int Cout, int H, int W) {
  __shared__ float ws[kMaxCout * CIN * 9];
  for (int i = threadIdx.x; i < Cout * CIN * 9; i += kThreads) ws[i] = wt[i];
  __syncthreads();
  const int HW = H * W;
  const int p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= N * HW) return;
  const int n = p / HW, r = p - n * HW, h = r / W, w = r - (r / W) * W;
  float v[CIN * 9];
  load_patch<CIN>(x, n, h, w, H, W, v);
  float* out = y + (size_t)n * Cout * HW + r;
  for (int co = 0; co < Cout; ++co) {
    const float* wc = ws + co * CIN * 9;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < CIN * 9; ++k) acc = fmaf(wc[k], v[k], acc);
    out[(size_t)co * HW] = acc;
  }
}

// forward + BN statistics: every thread of the grid takes part in the wave sums
// (out-of-range pixels contribute zeros), waves fold into LDS, the workgroup into replica
// blockIdx.x % kRep of stats[kRep][2*Cout] = (sum, sum of squares).
template <int CIN>
__global__ __launch_bounds__(kThreads) void stem_fwd_stats_kernel(const float* __restrict__ x,
                                                                   const float* __restrict__ wt,
                                                                   float* __restrict__ y, double* __restrict__ stats,
                                                                   int N, int Cout, int H, int W) {
  __shared__ float ws[kMaxCout * CIN * 9];
  __shared__ float st[2 * kMaxCout];
  for (int i = threadIdx.x; i < Cout * CIN * 9; i += kThreads) ws[i] = wt[i];
  for (int i = threadIdx.x; i < 2 * Cout; i += kThreads) st[i] = 0.f;
  __syncthreads();
  const int HW = H * W;
  const int p = blockIdx.x * kThreads + threadIdx.x;
  const bool valid = p < N * HW;
  const int q = valid ? p : 0;
  const int n = q / HW, r = q - n * HW, h = r / W, w = r - (r / W) * W;
  float v[CIN * 9];
  load_patch<CIN>(x, n, h, w, H, W, v);
  float* out = y + (size_t)n * Cout * HW + r;
  const int lane = threadIdx.x & 63;
  // four channels at a time: their 8 statistics leave the wave through one reduce-scatter
  // (10 shuffles) instead of 8 separate wave sums (48)
  for (int co0 = 0; co0 < Cout; co0 += 4) {
    float s[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int co = co0 + j;
      float acc = 0.f;
      if (co < Cout) {
        const float* wc = ws + co * CIN * 9;
#pragma unroll
        for (int k = 0; k < CIN * 9; ++k) acc = fmaf(wc[k], v[k], acc);
        if (valid) out[(size_t)co * HW] = acc;
      }
      const float a = valid ? acc : 0.f;
      s[j] = a;
      s[4 + j] = a * a;
    }
    const float t = wave_reduce_scatter<8>(s);
    const int i = wave_scatter_index<8>(lane), co = co0 + (i & 3);
    if ((lane & 7) == 0 && co < Cout) atomicAdd(&st[(i >> 2) * Cout + co], t);
  }
  __syncthreads();
  double* rep = stats + (size_t)(blockIdx.x % kRep) * 2 * Cout;
  for (int i = threadIdx.x; i < 2 * Cout; i += kThreads) atomicAdd(rep + i, (double)st[i]);
}

constexpr int kCG = 4;  // output channels per weight-gradient workgroup: kCG * 27 accumulators in registers

// wave sums of M accumulators stored to dst[0 .. M): power-of-two chunks through the reduce-scatter
// (108 = 64 + 32 + 8 + 4), as wave_sums_to_lds but with one writer per entry
template <int M>
__device__ __forceinline__ void wave_sums_store(float* acc, float* dst, int lane) {
  if constexpr (M > 0) {
    constexpr int P = M >= 64 ? 64 : (M >= 32 ? 32 : (M >= 16 ? 16 : (M >= 8 ? 8 : (M >= 4 ? 4 : (M >= 2 ? 2 : 1)))));
    const float s = wave_reduce_scatter<P>(acc);
    if ((lane & (64 / P - 1)) == 0) dst[wave_scatter_index<P>(lane)] = s;
    wave_sums_store<M - P>(acc + P, dst + P, lane);
  }
}

// grid (pixel chunk, channel group): the patch of a pixel is loaded once for the kCG channels of
// the group; channels past Cout in the last group read channel Cout - 1 and contribute zeros
template <int CIN, bool BN>
__global__ __launch_bounds__(kThreads) void stem_wgrad_kernel(const float* __restrict__ x,
                                                               const float* __restrict__ dy, BnBwd bn,
                                                               float* __restrict__ partial, int N, int Cout, int H,
                                                               int W, int per_chunk) {
  constexpr int K = CIN * 9, M = kCG * K;
  __shared__ float red[kThreads / 64][M];
  const int co0 = blockIdx.y * kCG, HW = H * W, P = N * HW;
  const int p0 = blockIdx.x * per_chunk, p1 = min(P, p0 + per_chunk);
  // BN backward coefficients: dz = k1 * (dy - m1 - zhat * m2), zhat = (z - mean) * istd
  int cc[kCG];
  bool live[kCG];
  float mean[kCG], istd[kCG], k1[kCG], m1[kCG], m2[kCG];
#pragma unroll
  for (int j = 0; j < kCG; ++j) {
    live[j] = co0 + j < Cout;
    const int co = cc[j] = min(co0 + j, Cout - 1);
    mean[j] = istd[j] = m1[j] = m2[j] = 0.f;
    k1[j] = 1.f;
    if (BN) {
      const double m = bn.stats[co] * (double)bn.inv_count;
      double var = bn.stats[Cout + co] * (double)bn.inv_count - m * m;
      if (var < 0) var = 0;
      mean[j] = (float)m;
      istd[j] = rsqrtf((float)var + bn.eps);
      k1[j] = bn.gamma[co] * istd[j];
      m1[j] = (float)(bn.red[co] * (double)bn.inv_count);
      m2[j] = (float)(bn.red[Cout + co] * (double)bn.inv_count);
    }
  }
  if (BN && blockIdx.x == 0 && threadIdx.x < kCG && co0 + threadIdx.x < Cout) {  // single writer per channel
    const int co = co0 + threadIdx.x;
    if (bn.dgamma) bn.dgamma[co] += (float)(bn.red[Cout + co] * (double)bn.red_scale);
    if (bn.dbeta) bn.dbeta[co] += (float)(bn.red[co] * (double)bn.red_scale);
  }
  float acc[M];
#pragma unroll
  for (int k = 0; k < M; ++k) acc[k] = 0.f;
  for (int p = p0 + threadIdx.x; p < p1; p += kThreads) {
    const int n = p / HW, r = p - n * HW, h = r / W, w = r - (r / W) * W;
    float d[kCG];
#pragma unroll
    for (int j = 0; j < kCG; ++j) {
      const size_t idx = ((size_t)n * Cout + cc[j]) * HW + r;
      float t = dy[idx];
      if (BN) t = k1[j] * (t - m1[j] - (bn.z[idx] - mean[j]) * istd[j] * m2[j]);
      d[j] = live[j] ? t : 0.f;
    }
    float v[K];
    load_patch<CIN>(x, n, h, w, H, W, v);
#pragma unroll
    for (int j = 0; j < kCG; ++j) {
#pragma unroll
      for (int k = 0; k < K; ++k) acc[j * K + k] = fmaf(d[j], v[k], acc[j * K + k]);
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  wave_sums_store<M>(acc, red[wave], lane);
  __syncthreads();
  if (threadIdx.x < M && co0 * K + threadIdx.x < Cout * K) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kThreads / 64; ++i) s += red[i][threadIdx.x];
    partial[((size_t)blockIdx.x * Cout + co0) * K + threadIdx.x] = s;
  }
}

// one wave per weight element: lanes stride over the chunk partials, then a shuffle tree
// (fixed order for a given chunk count -> deterministic)
__global__ __launch_bounds__(64) void chunk_sum_kernel(const float* __restrict__ partial, float* __restrict__ out,
                                                        int n, int chunks, int accumulate) {
  const int i = blockIdx.x;
  float s = 0.f;
  for (int c = threadIdx.x; c < chunks; c += 64) s += partial[(size_t)c * n + i];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
  if (threadIdx.x == 0) out[i] = accumulate ? out[i] + s : s;  // accumulate: into a gradient row
}

}  // namespace

void launch_fwd(const float* x, const float* w, float* y, int N, int Cin, int Cout, int H, int W, hipStream_t s) {
  const int blocks = (N * H * W + kThreads - 1) / kThreads;
  if (Cin == 3)
    hipLaunchKernelGGL(stem_fwd_kernel<3>, dim3(blocks), dim3(kThreads), 0, s, x, w, y, N, Cout, H, W);
  else
    hipLaunchKernelGGL(stem_fwd_kernel<1>, dim3(blocks), dim3(kThreads), 0, s, x, w, y, N, Cout, H, W);
}

namespace {

template <bool BN>
void wgrad_impl(const float* x, const float* dy, const BnBwd& bn, float* partial, float* dw, int N, int Cin, int Cout,
                int H, int W, int chunks, hipStream_t s, bool accumulate = false) {
  const int P = N * H * W;
  const int per_chunk = (P + chunks - 1) / chunks;
  const int groups = (Cout + kCG - 1) / kCG;
  if (Cin == 3)
    hipLaunchKernelGGL((stem_wgrad_kernel<3, BN>), dim3(chunks, groups), dim3(kThreads), 0, s, x, dy, bn, partial, N,
                       Cout, H, W, per_chunk);
  else
    hipLaunchKernelGGL((stem_wgrad_kernel<1, BN>), dim3(chunks, groups), dim3(kThreads), 0, s, x, dy, bn, partial, N,
                       Cout, H, W, per_chunk);
  const int n = Cout * Cin * 9;
  hipLaunchKernelGGL(chunk_sum_kernel, dim3(n), dim3(64), 0, s, partial, dw, n, chunks, accumulate ? 1 : 0);
}

}  // namespace

void launch_wgrad(const float* x, const float* dy, float* partial, float* dw, int N, int Cin, int Cout, int H, int W,
                  int chunks, hipStream_t s) {
  wgrad_impl<false>(x, dy, BnBwd{}, partial, dw, N, Cin, Cout, H, W, chunks, s);
}

void launch_wgrad_bn(const float* x, const float* dy, const BnBwd& bn, float* partial, float* dw, int N, int Cin,
                     int Cout, int H, int W, int chunks, hipStream_t s, bool accumulate) {
  wgrad_impl<true>(x, dy, bn, partial, dw, N, Cin, Cout, H, W, chunks, s, accumulate);
}

void launch_fwd_stats(const float* x, const float* w, float* y, double* stats, int N, int Cin, int Cout, int H, int W,
                      hipStream_t s) {
  const int blocks = (N * H * W + kThreads - 1) / kThreads;
  if (Cin == 3)
    hipLaunchKernelGGL(stem_fwd_stats_kernel<3>, dim3(blocks), dim3(kThreads), 0, s, x, w, y, stats, N, Cout, H, W);
  else
    hipLaunchKernelGGL(stem_fwd_stats_kernel<1>, dim3(blocks), dim3(kThreads), 0, s, x, w, y, stats, N, Cout, H, W);
}

}  // namespace stem
}  // namespace katib_hip
