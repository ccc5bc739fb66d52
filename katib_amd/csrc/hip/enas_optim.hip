// One-launch Adam of an ENAS child (ops/enas_optim.py), see enas_optim.h for the contract.
//
// Work mapping. The launch is a list of segments, one per parameter tensor; a segment owns the workgroups
// [tile0, tile0 + tiles) and a workgroup (256 threads, 4 waves) finds its segment by binary search.
//  flat       1024 elements per workgroup, 4 per thread, 256 apart: the 16 loads of p, g, m, v are issued
//             before the first arithmetic.
//  conv       one (r, s) of a 64 x 64 (output, input) channel tile. A wave reads rows of 64 input channels of
//             p, g, m, v (4 output channels in flight per thread), updates, and writes the row of the bf16
//             [K][RS][C8] image; the rounded values also go into an LDS tile of pitch 65, from which the
//             transposed image [C8][RS][K] leaves in rows of 64 output channels.
//  depthwise  64 consecutive elements of [K][RS] per workgroup, one per lane. Wave w sums the partial rows
//             w, w + 4, ... with 8 loads in flight into 8 accumulators (row r goes to accumulator (r / 4) % 8),
//             folds them pairwise, and the 4 waves meet in LDS: ((w0 + w1) + (w2 + w3)). The order depends on
//             `rows` alone. Wave 0 then updates and scatters the tap-major image.
// Step counter. Thread 0 of every workgroup reads t, fences, and draws a ticket with one integer atomicAdd;
// the workgroup with the last ticket stores t + 1 and resets the ticket. Nobody waits for anybody.
#include "enas_optim.h"
#include "mlp_optim.h"

namespace katib_hip {
namespace enasoptim {

namespace {

typedef unsigned short u16;
constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kFlatTile = 1024;
constexpr int kFlatPer = kFlatTile / kThreads;
constexpr int kT = 64;       // conv tile: 64 output x 64 input channels of one (r, s)
constexpr int kPitch = kT + 1;
constexpr int kInFlight = 4;  // output channels of a conv tile a thread holds at once
constexpr int kDwTile = 64;   // depthwise elements per workgroup
constexpr int kDwAcc = 8;

// fp32 -> bf16 bits, round to nearest even; NaN -> 0x7FC0 (what Tensor.to(torch.bfloat16) gives)
__device__ __forceinline__ u16 f2bf(float f) {
  unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;
  u += 0x7fffu + ((u >> 16) & 1u);
  return (u16)(u >> 16);
}

__global__ __launch_bounds__(kThreads) void enas_adam_k(const Seg* __restrict__ segs, int nseg, int32_t* counters,
                                                        float lr, float b1, float b2, float eps, int update) {
  __shared__ u16 tile[kT * kPitch];
  __shared__ float red[kThreads / kWave][kWave];
  __shared__ float coef[2];
  const int t = blockIdx.x, tid = threadIdx.x;
  mlp::AdamUpd upd{b1, b2, eps, nullptr, 0.f, 0.f};
  if (update) {
    if (tid == 0) {
      const int done = __hip_atomic_load(counters, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __threadfence();  // the read of t is over before the ticket is drawn
      const int ticket = atomicAdd(counters + 1, 1);
      if (ticket == (int)gridDim.x - 1) {  // every other workgroup has read t
        __hip_atomic_store(counters + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(counters, done + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      coef[0] = lr / (1.f - mlp::AdamUpd::ipow(b1, done + 1));
      coef[1] = sqrtf(1.f - mlp::AdamUpd::ipow(b2, done + 1));
    }
    __syncthreads();
    upd.step = coef[0];
    upd.sbc2 = coef[1];
  }
  int lo = 0, hi = nseg - 1;  // last segment with tile0 <= t
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (segs[mid].tile0 <= t)
      lo = mid;
    else
      hi = mid - 1;
  }
  const Seg s = segs[lo];
  const int lt = t - s.tile0;

  if (s.kind == kFlat) {
    if (!update) return;
    float p[kFlatPer], g[kFlatPer], m[kFlatPer], v[kFlatPer];
    const int base = lt * kFlatTile + tid;
#pragma unroll
    for (int j = 0; j < kFlatPer; ++j) {
      const int i = base + kThreads * j;
      if (i < s.n) {
        p[j] = s.p[i];
        g[j] = s.g[i];
        m[j] = s.m[i];
        v[j] = s.v[i];
      }
    }
#pragma unroll
    for (int j = 0; j < kFlatPer; ++j) {
      const int i = base + kThreads * j;
      if (i < s.n) {
        const float w = upd(g[j], m[j], v[j], p[j]);
        s.p[i] = w;
        s.m[i] = m[j];
        s.v[i] = v[j];
        s.g[i] = 0.f;
      }
    }
    return;
  }

  if (s.kind == kConv) {
    u16* wk = reinterpret_cast<u16*>(s.img);
    u16* wt = reinterpret_cast<u16*>(s.wt);
    const int tiles_k = (s.K + kT - 1) / kT;
    const int rs = lt % s.RS, r2 = lt / s.RS, kt = r2 % tiles_k, ct = r2 / tiles_k;
    const int cl = tid & (kT - 1), c = ct * kT + cl;
    const bool real = c < s.C, col = c < s.C8;
    for (int jb = 0; jb < kT * kT / kThreads; jb += kInFlight) {
      float p[kInFlight], g[kInFlight], m[kInFlight], v[kInFlight];
#pragma unroll
      for (int jj = 0; jj < kInFlight; ++jj) {
        const int k = kt * kT + (tid >> 6) + (kThreads / kT) * (jb + jj);
        p[jj] = 0.f;
        if (k < s.K && real) {
          const int row = k * s.RS + rs;
          p[jj] = s.p[row * s.C + c];
          if (update) {
            g[jj] = s.g[row * s.C8 + c];
            m[jj] = s.m[row * s.C + c];
            v[jj] = s.v[row * s.C + c];
          }
        }
      }
#pragma unroll
      for (int jj = 0; jj < kInFlight; ++jj) {
        const int kl = (tid >> 6) + (kThreads / kT) * (jb + jj), k = kt * kT + kl;
        if (k < s.K && col) {
          const int row = k * s.RS + rs;
          if (update) {
            if (real) {
              p[jj] = upd(g[jj], m[jj], v[jj], p[jj]);
              s.p[row * s.C + c] = p[jj];
              s.m[row * s.C + c] = m[jj];
              s.v[row * s.C + c] = v[jj];
            }
            s.g[row * s.C8 + c] = 0.f;
          }
          wk[row * s.C8 + c] = f2bf(p[jj]);
        }
        tile[cl * kPitch + kl] = f2bf(p[jj]);
      }
    }
    if (wt == nullptr) return;  // uniform per workgroup
    __syncthreads();
    const int kl = tid & (kT - 1), k = kt * kT + kl;
#pragma unroll 4
    for (int j = 0; j < kT * kT / kThreads; ++j) {
      const int cl2 = (tid >> 6) + (kThreads / kT) * j, c2 = ct * kT + cl2;
      if (c2 < s.C8 && k < s.K) wt[(c2 * s.RS + rs) * s.K + k] = tile[cl2 * kPitch + kl];
    }
    return;
  }

  // depthwise
  float* img = reinterpret_cast<float*>(s.img);
  const int lane = tid & (kWave - 1), w = tid >> 6;
  const int e = lt * kDwTile + lane;
  const bool ok = e < s.n;
  const int co = ok ? e / s.RS : 0, tap = e - co * s.RS;
  if (!update) {
    if (w == 0 && ok) img[tap * s.K + co] = s.p[e];
    return;
  }
  float p = 0.f, m = 0.f, v = 0.f;
  if (w == 0 && ok) {
    p = s.p[e];
    m = s.m[e];
    v = s.v[e];
  }
  float acc[kDwAcc];
#pragma unroll
  for (int u = 0; u < kDwAcc; ++u) acc[u] = 0.f;
  const int nw = kThreads / kWave;
  for (int r0 = w; r0 < s.rows; r0 += nw * kDwAcc) {
    float x[kDwAcc];
#pragma unroll
    for (int u = 0; u < kDwAcc; ++u) {
      const int r = r0 + nw * u;
      x[u] = (ok && r < s.rows) ? s.g[r * s.n + e] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < kDwAcc; ++u) acc[u] += x[u];
  }
  red[w][lane] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
  __syncthreads();
  if (w == 0 && ok) {
    const float g = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
    p = upd(g, m, v, p);
    s.p[e] = p;
    s.m[e] = m;
    s.v[e] = v;
    img[tap * s.K + co] = p;
  }
}

}  // namespace

int tiles(const Seg& s) {
  if (s.kind == kConv) return s.RS * ((s.K + kT - 1) / kT) * ((s.C8 + kT - 1) / kT);
  if (s.kind == kDepthwise) return (s.n + kDwTile - 1) / kDwTile;
  return (s.n + kFlatTile - 1) / kFlatTile;
}

hipError_t launch(const Seg* segs_dev, int nseg, int total_tiles, int32_t* counters, float lr, float beta1,
                  float beta2, float eps, int update, hipStream_t st) {
  hipLaunchKernelGGL(enas_adam_k, dim3(total_tiles), dim3(kThreads), 0, st, segs_dev, nseg, counters, lr, beta1, beta2,
                     eps, update);
  return hipGetLastError();
}

}  // namespace enasoptim
}  // namespace katib_hip
