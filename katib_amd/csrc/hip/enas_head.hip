// Head of an ENAS child in two launches forward and one backward: global average pooling,
// Dropout, the dense classifier, softmax cross-entropy and the accuracy bookkeeping (reference
// examples/v1beta1/trial-images/enas-cnn-cifar10/ModelConstructor.py: GlobalAveragePooling2D,
// Dropout(0.4), Dense softmax; RunTrial.py: categorical cross-entropy and accuracy).
//
//   x [B][HW][C] bf16 (dense NHWC), W [K][C] and bias [K] fp32 masters, y [B] int64, K <= 64, C <= kMaxC
//   pooled = (sum over pixels, fp32) * (1 / HW)
//   feat   = keep ? pooled * scale : 0; keep from Philox4x32-10 with counter (q lo, q hi, site, step),
//            q = (b Cp + c) >> 2, Cp = 4 ceil(C / 4), word c & 3 >= round(p 2^32) (ops/transformer.py:
//            dropout_mask(B, Cp, ...)[b, c]); without dropout feat = pooled
//   logits = bias + feat W^T; loss_b = lse - logits[y]; hit_b = (lowest argmax == y)
//   dl     = (softmax - onehot) / B; loss = (sum_b loss_b) / B
//   dW = g dl^T feat, db = g colsum(dl), dx[b, pixel, c] = bf16(g keep (scale / HW) sum_k dl[b][k] W[k][c])
//
// enas_head_fwd_k: a workgroup per sample. The label, the bias and the first strip of the W rows are
// loaded before anything is waited for. Pooling, 16-byte path (C % 8 == 0): a thread owns a chunk
// (8 channels) and a pixel lane, nq = C / 8 chunks x floor(256 / nq) lanes, four chunk loads in
// flight before the first add, then eight adds per chunk in pixel order; the pixel lanes' partial
// sums meet in LDS and are added in lane order, so the sum's order depends on (HW, C) alone. With more
// than 256 chunks a thread loops over chunks. Element path: a thread per channel, 2-byte loads that
// are coalesced across the channels. Thread j draws the Philox words of channels 4j .. 4j + 3. Dense:
// wave w owns classes w, w + 4, ..., its lanes stride over c, a butterfly adds the lanes (the same
// order in every lane). Softmax: wave 0, lane = class. All global stores come last.
// enas_head_sum_k: one workgroup adds loss_b and hit_b in a fixed order, adds into the trial's
// statistics and advances the step counter - after every forward workgroup has read it.
// enas_head_bwd_k: one launch, two roles by blockIdx. Data role (b, s): the sample's dx row is formed
// once in LDS as bf16 (K floats of dl, K x C of W from L2) and streamed over pixel segment s with
// 16-byte stores (2-byte on the element path). Weight role: a workgroup owns 64 channels, thread
// (c, class group) adds its classes over b = 0 .. B - 1 in order with dl tiled through LDS; the first
// of them also writes db. No atomics: every output element has one writer and one summation order.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "enas_head.h"
#include "philox.h"

namespace katib_hip {
namespace enashead {

namespace {

using tfm::philox4x32_10;
using tfm::philox_u32x4;

constexpr int kPre = 3;        // classes per wave whose first W strip is loaded up front (K <= 12, C <= 64: all of W)
constexpr int kDlTile = 2048;  // floats of dl per LDS tile of the weight role (>= 32 samples at K = 64)
constexpr int kCUs = 256;
// Bytes of dx a data-role workgroup streams at the least: the segments per sample S grow until
// B S is two workgroups per CU, and stop where a segment would fall under this. Interleaved A/B of
// S = 1, 2, 4, 8, 16 at batch 128 (benchmarks/bench_enas_head.py --segs, profiles/enas_head.log;
// forward + backward, window spread +- 0.5 %): 32x32x64 49.2 / 48.7 / 48.5 / 48.8 / 50.2 us,
// 32x32x67 95.8 / 95.3 / 93.2 / 95.9 / 96.4 us - 32 KB segments are the fastest and 8 KB ones cost
// 3 %; 16x16x64 and 8x8x128 move by 1.5 % between S = 1 and 2, inside what the rule leaves. A 1 MB
// sample (32x32x528) is the exception the rule does not model: 105.5 us at S = 1, 115.2 at the
// rule's S = 4 - the stream is already bandwidth-bound and every further workgroup repeats the
// K x C prologue.
constexpr int kSegBytes = 32768;

__device__ __forceinline__ float bf2f(uint32_t h) { return __uint_as_float(h << 16); }

// round to nearest even; a NaN stays a NaN
__device__ __forceinline__ uint16_t f2bf(float f) {
  const uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

__device__ __forceinline__ void add8(float* s, const uint4& v) {
  s[0] += bf2f(v.x & 0xffffu);
  s[1] += bf2f(v.x >> 16);
  s[2] += bf2f(v.y & 0xffffu);
  s[3] += bf2f(v.y >> 16);
  s[4] += bf2f(v.z & 0xffffu);
  s[5] += bf2f(v.z >> 16);
  s[6] += bf2f(v.w & 0xffffu);
  s[7] += bf2f(v.w >> 16);
}

template <class T>
__device__ __forceinline__ T wave_xor(T v, int off) { return __shfl_xor(v, off, 64); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += wave_xor(v, off);
  return v;
}

template <bool DROP>
__global__ void __launch_bounds__(256) enas_head_fwd_k(const Fwd a, const int vec) {
  __shared__ __align__(16) float red[kMaxC];  // partial sums [pixel lane][C]
  __shared__ float feat_s[kMaxC];
  __shared__ uint8_t keep_s[kMaxC];
  __shared__ float logit_s[kMaxK], bias_s[kMaxK];
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int C = a.C, K = a.K, HW = a.HW;

  // loads that depend on nothing
  const int64_t yraw = a.y[b];
  const float bias_r = t < K ? a.bias[t] : 0.f;
  float wpre[kPre];
#pragma unroll
  for (int i = 0; i < kPre; ++i) {
    const int k = wave + 4 * i;
    wpre[i] = (k < K && lane < C) ? a.w[k * C + lane] : 0.f;
  }
  uint32_t step = 0;
  if (DROP) step = (uint32_t)*a.step;

  int L = 1;  // pixel lanes
  if (vec) {
    const int nq = C >> 3, nqw = nq < 256 ? nq : 256;
    L = 256 / nqw;
    const uint4* __restrict__ xs = static_cast<const uint4*>(a.x) + b * HW * nq;
    if (t < nqw * L) {
      const int pl = t / nqw, q0 = t - pl * nqw;
      for (int q = q0; q < nq; q += nqw) {
        float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        int p = pl;
        for (; p + 3 * L < HW; p += 4 * L) {
          const uint4 v0 = xs[p * nq + q], v1 = xs[(p + L) * nq + q], v2 = xs[(p + 2 * L) * nq + q],
                      v3 = xs[(p + 3 * L) * nq + q];
          add8(s, v0);
          add8(s, v1);
          add8(s, v2);
          add8(s, v3);
        }
        for (; p < HW; p += L) add8(s, xs[p * nq + q]);
        float4* r = reinterpret_cast<float4*>(red + pl * C + q * 8);
        r[0] = make_float4(s[0], s[1], s[2], s[3]);
        r[1] = make_float4(s[4], s[5], s[6], s[7]);
      }
    }
  } else {
    const uint16_t* __restrict__ xs = static_cast<const uint16_t*>(a.x) + b * HW * C;
    for (int c = t; c < C; c += 256) {
      float s = 0.f;
      int p = 0;
      for (; p + 3 < HW; p += 4) {
        const uint16_t v0 = xs[p * C + c], v1 = xs[(p + 1) * C + c], v2 = xs[(p + 2) * C + c],
                       v3 = xs[(p + 3) * C + c];
        s += bf2f(v0);
        s += bf2f(v1);
        s += bf2f(v2);
        s += bf2f(v3);
      }
      for (; p < HW; p += 1) s += bf2f(xs[p * C + c]);
      red[c] = s;
    }
  }
  if (t < K) bias_s[t] = bias_r;
  __syncthreads();

  // pixel lanes in lane order, the mean, the draw
  const float inv_hw = __fdiv_rn(1.f, (float)HW);
  const int Cp4 = (C + 3) >> 2;
  for (int j = t; j < Cp4; j += 256) {
    philox_u32x4 w = {0u, 0u, 0u, 0u};
    if (DROP) {
      const uint64_t q = (uint64_t)b * (uint64_t)Cp4 + (uint64_t)j;
      w = philox4x32_10(philox_u32x4{(uint32_t)q, (uint32_t)(q >> 32), a.site, step}, (uint32_t)a.seed,
                        (uint32_t)(a.seed >> 32));
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = 4 * j + k;
      if (c < C) {
        float s = red[c];
        for (int l = 1; l < L; ++l) s += red[l * C + c];
        const float pooled = s * inv_hw;
        const bool keep = !DROP || w[k] >= a.thr;
        feat_s[c] = DROP ? (keep ? pooled * a.scale : 0.f) : pooled;
        keep_s[c] = keep ? 1 : 0;
      }
    }
  }
  __syncthreads();

  // dense: wave = class group, lanes stride over the channels
  auto dense_row = [&](int k, float first) {
    float acc = lane < C ? feat_s[lane] * first : 0.f;
    for (int c = lane + 64; c < C; c += 64) acc = fmaf(feat_s[c], a.w[k * C + c], acc);
    acc = wave_sum(acc);
    if (lane == 0) logit_s[k] = acc + bias_s[k];
  };
#pragma unroll
  for (int i = 0; i < kPre; ++i) {
    const int k = wave + 4 * i;
    if (k < K) dense_row(k, wpre[i]);
  }
  for (int k = wave + 4 * kPre; k < K; k += 4) dense_row(k, lane < C ? a.w[k * C + lane] : 0.f);
  __syncthreads();

  // softmax cross-entropy: wave 0, lane = class
  float lg = 0.f, dl = 0.f, loss = 0.f, hit = 0.f;
  if (wave == 0) {
    const bool live = lane < K;
    lg = live ? logit_s[lane] : -INFINITY;
    float m = lg;
    int idx = live ? lane : INT_MAX;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float om = wave_xor(m, off);
      const int oi = wave_xor(idx, off);
      if (om > m || (om == m && oi < idx)) {
        m = om;
        idx = oi;
      }
    }
    const float e = live ? expf(lg - m) : 0.f;
    const float s = wave_sum(e);
    const int yc = (int)(yraw < 0 ? 0 : (yraw > K - 1 ? K - 1 : yraw));  // addressing only
    loss = m + logf(s) - logit_s[yc];
    hit = (int64_t)idx == yraw ? 1.f : 0.f;
    dl = (e / s - (lane == yc ? 1.f : 0.f)) / (float)a.B;
  }

  // stores, after the last load
  for (int c = t; c < C; c += 256) {
    a.feat[b * C + c] = feat_s[c];
    a.keep[b * C + c] = keep_s[c];
  }
  if (wave == 0) {
    if (lane < K) {
      a.logits[b * K + lane] = lg;
      a.dl[b * K + lane] = dl;
    }
    if (lane == 0) {
      a.loss_b[b] = loss;
      a.hit_b[b] = hit;
    }
  }
}

__global__ void __launch_bounds__(256) enas_head_sum_k(const Sum a) {
  __shared__ float sl[256], sh[256];
  const int t = threadIdx.x;
  float l = 0.f, h = 0.f;
  for (int b = t; b < a.B; b += 256) {
    l += a.loss_b[b];
    h += a.hit_b[b];
  }
  sl[t] = l;
  sh[t] = h;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
      sl[t] += sl[t + s];
      sh[t] += sh[t + s];
    }
    __syncthreads();
  }
  if (t == 0) {
    const float loss = a.mean ? sl[0] / (float)a.B : sl[0], hits = sh[0];
    float s0 = 0.f, s1 = 0.f;
    int32_t step = 0;
    if (a.stats) {
      s0 = a.stats[0];
      s1 = a.stats[1];
    }
    if (a.step) step = *a.step;
    a.out[0] = loss;
    a.out[1] = hits;
    if (a.stats) {
      a.stats[0] = s0 + loss;
      a.stats[1] = s1 + hits;
    }
    if (a.step) *a.step = (int32_t)((uint32_t)step + 1u);
  }
}

__global__ void __launch_bounds__(256) enas_head_bwd_k(const Bwd a, const int vec, const int nData) {
  // data role: the sample's dx row as bf16 [kMaxC], then K floats of dl; weight role: a dl tile
  __shared__ __align__(16) uint32_t sm[kMaxC / 2 + kMaxK];
  static_assert(kDlTile <= kMaxC / 2 + kMaxK && kDlTile >= kMaxK, "dl tile must fit the shared buffer");
  const int t = threadIdx.x;
  const int B = a.B, C = a.C, K = a.K, HW = a.HW;
  const float g = *a.g;
  if ((int)blockIdx.x < nData) {
    uint16_t* dxs = reinterpret_cast<uint16_t*>(sm);
    float* dl_s = reinterpret_cast<float*>(sm + kMaxC / 2);
    const int b = blockIdx.x / a.S, s = blockIdx.x - b * a.S;
    if (t < K) dl_s[t] = a.dl[b * K + t];
    __syncthreads();
    for (int c = t; c < C; c += 256) {
      const float m = a.keep[b * C + c] ? a.mscale : 0.f;
      float acc = 0.f;
#pragma unroll 4
      for (int k = 0; k < K; ++k) acc = fmaf(dl_s[k], a.w[k * C + c], acc);
      dxs[c] = f2bf(g * m * acc);
    }
    __syncthreads();
    const int p0 = (int)((int64_t)HW * s / a.S), p1 = (int)((int64_t)HW * (s + 1) / a.S);
    if (vec) {
      const int nq = C >> 3, n = (p1 - p0) * nq, adv = 256 % nq;
      uint4* __restrict__ out = static_cast<uint4*>(a.dx) + (b * HW + p0) * nq;
      const uint4* row = reinterpret_cast<const uint4*>(dxs);
      int q = t % nq;
      for (int e = t; e < n; e += 256) {
        out[e] = row[q];
        q += adv;
        if (q >= nq) q -= nq;
      }
    } else {
      const int n = (p1 - p0) * C, adv = 256 % C;
      uint16_t* __restrict__ out = static_cast<uint16_t*>(a.dx) + (b * HW + p0) * C;
      int c = t % C;
      for (int e = t; e < n; e += 256) {
        out[e] = dxs[c];
        c += adv;
        if (c >= C) c -= C;
      }
    }
  } else {
    float* tile = reinterpret_cast<float*>(sm);
    const int wg = blockIdx.x - nData;
    const int kg = t >> 6, c = wg * 64 + (t & 63);
    const bool do_w = a.dw != nullptr && c < C, do_b = a.db != nullptr && wg == 0 && t < K;
    const int nk = kg < K ? (K - kg + 3) >> 2 : 0;  // classes kg, kg + 4, ...
    const int TB = kDlTile / K;                     // samples per tile
    float acc[kMaxK / 4];
#pragma unroll
    for (int i = 0; i < kMaxK / 4; ++i) acc[i] = 0.f;
    float dbs = 0.f;
    auto add = [&](int bb, float f) {
#pragma unroll
      for (int i = 0; i < kMaxK / 4; ++i)
        if (i < nk) acc[i] = fmaf(tile[bb * K + kg + 4 * i], f, acc[i]);
    };
    for (int b0 = 0; b0 < B; b0 += TB) {
      const int nb = B - b0 < TB ? B - b0 : TB;
      __syncthreads();  // the tile before this one has been read
      for (int i = t; i < nb * K; i += 256) tile[i] = a.dl[b0 * K + i];
      __syncthreads();
      if (do_b)
        for (int bb = 0; bb < nb; ++bb) dbs += tile[bb * K + t];
      if (do_w) {
        const float* __restrict__ fp = a.feat + b0 * C + c;
        int bb = 0;
        for (; bb + 7 < nb; bb += 8) {
          float f[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) f[u] = fp[(bb + u) * C];
#pragma unroll
          for (int u = 0; u < 8; ++u) add(bb + u, f[u]);
        }
        for (; bb < nb; ++bb) add(bb, fp[bb * C]);
      }
    }
    if (do_w) {
#pragma unroll
      for (int i = 0; i < kMaxK / 4; ++i)
        if (i < nk) a.dw[(kg + 4 * i) * C + c] = g * acc[i];
    }
    if (do_b) a.db[t] = g * dbs;
  }
}

}  // namespace

bool vector_ok(const void* x, int C) { return C % 8 == 0 && reinterpret_cast<uintptr_t>(x) % 16 == 0; }

int segments(int B, int HW, int C) {
  const int64_t bytes = (int64_t)HW * C * 2;
  int64_t S = (2 * kCUs + B - 1) / B;
  if (S > bytes / kSegBytes) S = bytes / kSegBytes;
  if (S > HW) S = HW;
  return S < 1 ? 1 : (int)S;
}

static bool sizes_ok(int B, int HW, int C, int K) {
  return B >= 1 && HW >= 1 && C >= 1 && C <= kMaxC && K >= 1 && K <= kMaxK &&
         (int64_t)B * HW * C < (1ll << 31);
}

hipError_t launch_fwd(const Fwd& a, bool drop, hipStream_t st) {
  if (!sizes_ok(a.B, a.HW, a.C, a.K) || (drop && a.step == nullptr)) return hipErrorInvalidValue;
  const int vec = vector_ok(a.x, a.C) ? 1 : 0;
  if (drop)
    hipLaunchKernelGGL(enas_head_fwd_k<true>, dim3(a.B), dim3(256), 0, st, a, vec);
  else
    hipLaunchKernelGGL(enas_head_fwd_k<false>, dim3(a.B), dim3(256), 0, st, a, vec);
  return hipGetLastError();
}

hipError_t launch_sum(const Sum& a, hipStream_t st) {
  if (a.B < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(enas_head_sum_k, dim3(1), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_bwd(const Bwd& a, hipStream_t st) {
  if (!sizes_ok(a.B, a.HW, a.C, a.K) || a.S < 1 || a.S > a.HW) return hipErrorInvalidValue;
  const int nData = a.dx ? a.B * a.S : 0;
  const int nW = a.dw ? (a.C + 63) / 64 : (a.db ? 1 : 0);
  if (nData + nW == 0) return hipSuccess;
  const int vec = a.dx && vector_ok(a.dx, a.C) ? 1 : 0;
  hipLaunchKernelGGL(enas_head_bwd_k, dim3(nData + nW), dim3(256), 0, st, a, vec, nData);
  return hipGetLastError();
}

}  // namespace enashead
}  // namespace katib_hip
