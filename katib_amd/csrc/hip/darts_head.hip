// Fused DARTS head: gap + classifier + cross-entropy, forward and backward - see darts_head.h.
//
// Both kernels run one workgroup per sample (the logits need every channel of a sample) and move
// 24 KB per workgroup at B5, so their cost is the number of dependent memory round trips, not
// bytes: every load that depends on nothing (label, bias, classifier weights, dl, pooled, the
// first pooling operands) is issued before the first wait, the classifier weights wait in LDS
// while the pooling loads are in flight, and every global store comes after the last load.
#include <cmath>
#include <cstdint>

#include "darts_head.h"
#include "darts_ops_dev.h"  // kRep (weight-gradient replica rows), wave_reduce_scatter

namespace katib_hip {
namespace head {
namespace {

// 8 waves per sample: at B5 head_fwd 8.1 us against 8.7 us with 4 waves, head_bwd 5.1 against 5.5
// (profiles/darts_ends_bench_ab.txt)
constexpr int kThreads = 512;
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;
constexpr int kU = 8;  // channels / classes per wave with loads in flight together
// classifier weights [K][C] are staged in LDS up to this many floats (B5 240, darts-gpu.yaml 2560);
// larger heads read them from global memory after the pooling
constexpr int kWStage = 4096;
constexpr int kWRegs = kWStage / kThreads;
constexpr int kPRegs = kMaxC / kThreads;

__device__ inline float wave_sum(float v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

__device__ inline float wave_max(float v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
  return v;
}

// sum of item q of a plane: a quad (16-byte load, VEC) or one pixel
template <bool VEC>
__device__ __forceinline__ float item_sum(const float* __restrict__ plane, int q) {
  if constexpr (VEC) {
    const float4 f = reinterpret_cast<const float4*>(plane)[q];
    return (f.x + f.y) + (f.z + f.w);
  } else {
    return plane[q];
  }
}

// The K x C classifier weights into registers (thread t takes elements t, t + kThreads, ...), issued
// before anything waits; stage_store puts them into LDS once other loads are in flight behind them.
__device__ __forceinline__ void stage_load(const float* __restrict__ w, int count, float (&wr)[kWRegs]) {
#pragma unroll
  for (int j = 0; j < kWRegs; ++j) {
    const int i = threadIdx.x + j * kThreads;
    wr[j] = i < count ? w[i] : 0.0f;
  }
}
__device__ __forceinline__ void stage_store(float* sw, int count, const float (&wr)[kWRegs]) {
#pragma unroll
  for (int j = 0; j < kWRegs; ++j) {
    const int i = threadIdx.x + j * kThreads;
    if (i < count) sw[i] = wr[j];
  }
}

// One workgroup per sample. A plane is Q items (quads when VEC, else pixels); G = 1 << lg lanes
// share a channel (the smallest power of two covering Q, at most a wave), so one wave load covers
// 64 / G channels and small planes still fill the wave. Fixed summation order, no atomics.
template <bool VEC>
__global__ void __launch_bounds__(kThreads) head_fwd_kernel(FwdArgs a, int lg) {
  __shared__ float sp[kMaxC];
  __shared__ float sl[kMaxK];
  __shared__ float sw[kWStage];
  const int n = blockIdx.x, lane = threadIdx.x % kWave, wid = threadIdx.x / kWave;
  const int KC = a.K * a.C;
  const bool staged = KC <= kWStage;
  // everything that depends on nothing: label, bias, classifier weights
  const int64_t t = a.y[n];
  const float bk = lane < a.K ? a.b[lane] : 0.0f;
  float wr[kWRegs];
  stage_load(a.w, staged ? KC : 0, wr);

  const float inv_hw = 1.0f / a.HW;
  const int G = 1 << lg, cpw = kWave >> lg, sub = lane >> lg, q0 = lane & (G - 1);
  const int Q = VEC ? a.HW >> 2 : a.HW;
  // kU channel groups per wave in flight: all loads issue before the first reduction
  for (int c0 = wid * cpw; c0 < a.C; c0 += kWaves * cpw * kU) {
    float s[kU];
    const float* xc[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {  // rows past C read channel C - 1 (in bounds) and are dropped below
      const int c = min(c0 + u * kWaves * cpw + sub, a.C - 1);
      xc[u] = a.x + plane_off(n, c, a.N, a.C, a.nodes, a.HW);
    }
    if (Q <= G) {  // one item per lane: straight-line loads, lanes past Q read item Q - 1 and add zero
      const int q = min(q0, Q - 1);
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const float v = item_sum<VEC>(xc[u], q);
        s[u] = q0 < Q ? v : 0.0f;
      }
    } else {  // G = 64: items outermost, so every step has kU loads in flight
#pragma unroll
      for (int u = 0; u < kU; ++u) s[u] = 0.0f;
      for (int q = q0; q < Q; q += kWave) {
#pragma unroll
        for (int u = 0; u < kU; ++u) s[u] += item_sum<VEC>(xc[u], q);
      }
    }
    if (lg == 6) {  // a wave per channel: the kU sums leave through one reduce-scatter (10 shuffles, not 48)
      const float v = wave_reduce_scatter<kU>(s);
      const int c = c0 + wave_scatter_index<kU>(lane) * kWaves;
      if ((lane & (kWave / kU - 1)) == 0 && c < a.C) sp[c] = v * inv_hw;
    } else {  // butterfly inside the G lanes of a channel, the kU chains side by side
#pragma unroll
      for (int o = kWave / 4; o > 0; o >>= 1) {
        if (o < G) {
#pragma unroll
          for (int u = 0; u < kU; ++u) s[u] += __shfl_xor(s[u], o, kWave);
        }
      }
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int c = c0 + u * kWaves * cpw + sub;
        if (q0 == 0 && c < a.C) sp[c] = s[u] * inv_hw;
      }
    }
  }
  stage_store(sw, staged ? KC : 0, wr);
  __syncthreads();
  for (int k0 = wid; k0 < a.K; k0 += kWaves * kU) {
    float s[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int k = k0 + u * kWaves;
      float v = 0.0f;
      if (k < a.K) {
        if (staged && a.C <= kWave) {
          v = lane < a.C ? sp[lane] * sw[k * a.C + lane] : 0.0f;
        } else if (staged) {
          for (int c = lane; c < a.C; c += kWave) v += sp[c] * sw[k * a.C + c];
        } else if (a.C <= kWave) {
          v = lane < a.C ? sp[lane] * a.w[(size_t)k * a.C + lane] : 0.0f;
        } else {
          for (int c = lane; c < a.C; c += kWave) v += sp[c] * a.w[(size_t)k * a.C + c];
        }
      }
      s[u] = v;
    }
    const float v = wave_reduce_scatter<kU>(s);
    const int k = k0 + wave_scatter_index<kU>(lane) * kWaves;
    if ((lane & (kWave / kU - 1)) == 0 && k < a.K) sl[k] = v;
  }
  __syncthreads();
  // log-sum-exp, loss and dl in one wave, lane k = class k (kMaxK = a wave)
  if (wid == 0) {
    const bool in = lane < a.K;
    const float l = in ? sl[lane] + bk : -INFINITY;
    const float m = wave_max(l);
    const float lse = m + logf(wave_sum(in ? expf(l - m) : 0.0f));
    const bool ok = t >= 0 && t < a.K;  // out-of-range label -> NaN loss, no out-of-bounds read
    const float lt = __shfl(l, ok ? (int)t : 0, kWave);
    if (in) {
      a.logits[(size_t)n * a.K + lane] = l;
      a.dl[(size_t)n * a.K + lane] = (expf(l - lse) - (lane == t ? 1.0f : 0.0f)) * (1.0f / a.N);
    }
    if (lane == 0) a.loss_n[n] = ok ? lse - lt : NAN;
  }
  // the pooled features leave after the last load: a global store before one could alias it for
  // the compiler, which keeps the load behind the store (a round trip)
  for (int c = threadIdx.x; c < a.C; c += kThreads) a.pooled[(size_t)n * a.C + c] = sp[c];
}

__global__ void __launch_bounds__(kThreads) head_loss_kernel(const float* __restrict__ loss_n, int N,
                                                             float* __restrict__ loss) {
  __shared__ float sh[kWaves];
  float s = 0.0f;
  for (int i = threadIdx.x; i < N; i += kThreads) s += loss_n[i];
  s = wave_sum(s);
  if (threadIdx.x % kWave == 0) sh[threadIdx.x / kWave] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.0f;
    for (int i = 0; i < kWaves; ++i) t += sh[i];
    *loss = t / N;
  }
}

// dx planes are written as Q items (16-byte stores when VEC) by G = 1 << lg lanes per channel, as
// head_fwd_kernel reads them: no division per element.
template <bool VEC>
__global__ void __launch_bounds__(kThreads) head_bwd_kernel(BwdArgs a, int lg) {
  __shared__ float sd[kMaxK];
  __shared__ float sp[kMaxC];
  __shared__ float sdx[kMaxC];
  __shared__ float sw[kWStage];
  const int n = blockIdx.x, lane = threadIdx.x % kWave, wid = threadIdx.x / kWave;
  const int KC = a.K * a.C;
  const bool staged = a.dx != nullptr && KC <= kWStage;
  // every load up front: upstream gradient, dl, pooled features, classifier weights
  const float g = *a.gout;
  const float dlk = threadIdx.x < a.K ? a.dl[(size_t)n * a.K + threadIdx.x] : 0.0f;
  float pr[kPRegs];
#pragma unroll
  for (int j = 0; j < kPRegs; ++j) {
    const int c = threadIdx.x + j * kThreads;
    pr[j] = (a.gw != nullptr && c < a.C) ? a.pooled[(size_t)n * a.C + c] : 0.0f;
  }
  float wr[kWRegs];
  stage_load(a.w, staged ? KC : 0, wr);
  if (threadIdx.x < a.K) sd[threadIdx.x] = g * dlk;
#pragma unroll
  for (int j = 0; j < kPRegs; ++j) {
    const int c = threadIdx.x + j * kThreads;
    if (c < a.C) sp[c] = pr[j];
  }
  stage_store(sw, staged ? KC : 0, wr);
  __syncthreads();
  if (a.dx != nullptr) {
    // d[c] = (dl W)[c] / HW for every channel first, then the broadcast stores: a store between
    // two channels' weight loads (which may alias dx for the compiler) serialised one round trip
    // per channel
    const float inv_hw = 1.0f / a.HW;
    for (int c = threadIdx.x; c < a.C; c += kThreads) {
      float d = 0.0f;
      if (staged) {
        for (int k = 0; k < a.K; ++k) d += sd[k] * sw[k * a.C + c];
      } else {
        for (int k = 0; k < a.K; ++k) d += sd[k] * a.w[(size_t)k * a.C + c];
      }
      sdx[c] = d * inv_hw;
    }
    __syncthreads();
    const int G = 1 << lg, cpw = kWave >> lg, sub = lane >> lg, q0 = lane & (G - 1);
    const int Q = VEC ? a.HW >> 2 : a.HW;
    for (int c = wid * cpw + sub; c < a.C; c += kWaves * cpw) {
      const float v = sdx[c];
      float* dc = a.dx + plane_off(n, c, a.N, a.C, a.nodes, a.HW);
      for (int q = q0; q < Q; q += G) {
        if constexpr (VEC) reinterpret_cast<float4*>(dc)[q] = make_float4(v, v, v, v);
        else dc[q] = v;
      }
    }
  }
  const int rep = n % kRep;
  if (a.gw != nullptr) {
    float* gw = a.gw + (size_t)rep * a.gw_stride;
    for (int i = threadIdx.x; i < KC; i += kThreads) atomicAdd(gw + i, sd[i / a.C] * sp[i % a.C]);
  }
  if (a.gb != nullptr && threadIdx.x < a.K) atomicAdd(a.gb + (size_t)rep * a.gb_stride + threadIdx.x, sd[threadIdx.x]);
}

// 16-byte plane accesses need whole quads per plane and a 16-byte-aligned base (every plane then
// starts on a multiple of HW floats from it); anything else takes the one-pixel path
bool vec_ok(const void* base, int HW) { return HW % 4 == 0 && (reinterpret_cast<uintptr_t>(base) & 15) == 0; }

// log2 of the lanes that share a channel: the smallest power of two covering the plane's items
int lanes_log2(int items) {
  int lg = 0;
  while (lg < 6 && (1 << lg) < items) ++lg;
  return lg;
}

}  // namespace

void launch_fwd(const FwdArgs& a, hipStream_t st) {
  if (vec_ok(a.x, a.HW))
    hipLaunchKernelGGL(head_fwd_kernel<true>, dim3(a.N), dim3(kThreads), 0, st, a, lanes_log2(a.HW / 4));
  else
    hipLaunchKernelGGL(head_fwd_kernel<false>, dim3(a.N), dim3(kThreads), 0, st, a, lanes_log2(a.HW));
}

void launch_loss(const float* loss_n, int N, float* loss, hipStream_t st) {
  hipLaunchKernelGGL(head_loss_kernel, dim3(1), dim3(kThreads), 0, st, loss_n, N, loss);
}

void launch_bwd(const BwdArgs& a, hipStream_t st) {
  if (a.dx == nullptr || vec_ok(a.dx, a.HW))
    hipLaunchKernelGGL(head_bwd_kernel<true>, dim3(a.N), dim3(kThreads), 0, st, a, lanes_log2(a.HW / 4));
  else
    hipLaunchKernelGGL(head_bwd_kernel<false>, dim3(a.N), dim3(kThreads), 0, st, a, lanes_log2(a.HW));
}

}  // namespace head
}  // namespace katib_hip
