// Input of an ENAS child layer in one kernel per direction: layer l reads layer l-1 and every
// earlier layer its skip bits select, smaller maps zero-padded (d / 2 above and left, the rest
// below and right) to the largest, concatenated along the channels, then ReLU for every op but
// `reduction` (reference examples/v1beta1/trial-images/enas-cnn-cifar10/ModelConstructor.py:24-81,
// op_library.py:22-155). bf16 NHWC sources [B][H_i][H_i][C_i] with square maps:
//
//   forward : out[b][y][x][off_i + c] = act(x_i[b][y - t_i][x - t_i][c]) inside the map, else 0
//   backward: gx_i[b][y][x][c] = gout[b][y + t_i][x + t_i][off_i + c] (* (x_i > 0) with ReLU)
//
// Selection, zero fill and a sign test only, so both directions are exact. act keeps v unless
// v <= 0, and the backward passes g unless x <= 0: v > 0 ? v : 0 for every number, and a NaN goes
// through in both directions as it does through torch's relu.
//
// The source table travels by value in the kernel arguments. Vector path (every C_i % 8 == 0):
// a workgroup owns one row - (b, y) of the output forward, (b, y) of one source backward - so the
// row, the batch index and (backward) the source are uniform; a thread owns up to kChunks 16-byte
// chunks (8 channels) of that row, blockIdx.y selecting the segment of a long row. Forward, a
// chunk's pixel comes from a multiply-high by ceil(2^32 / (Ct / 8)) and its source from an unrolled
// scan of the channel prefix; no division by a runtime size per chunk. All loads of a thread are
// issued before its first store. No LDS, no atomics; every output element is written exactly once.
// Element path (the 3-channel image as a skip source, a gout pixel stride that is no multiple of
// 8): one thread per element with scalar accesses and plain divisions; correct, not fast.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "enas_concat.h"

namespace katib_hip {
namespace enasconcat {

namespace {

constexpr int kChunks = 4;  // 16-byte chunks per thread, all in flight together

// a bf16 widened to fp32 bits is <= 0: zero, or negative and no NaN (integer tests, so the answer
// does not depend on the denormal mode)
__device__ __forceinline__ bool le0(uint32_t f) {
  return (int32_t)f <= 0 && (f & 0x7fffffffu) <= 0x7f800000u;
}

// bf16 pair in a dword: the halves of g cleared where the half of x is <= 0
__device__ __forceinline__ uint32_t keep2(uint32_t x, uint32_t g) {
  return (le0(x << 16) ? 0u : g & 0x0000ffffu) | (le0(x & 0xffff0000u) ? 0u : g & 0xffff0000u);
}

__device__ __forceinline__ uint4 keep8(const uint4& x, const uint4& g) {
  return make_uint4(keep2(x.x, g.x), keep2(x.y, g.y), keep2(x.z, g.z), keep2(x.w, g.w));
}

__device__ __forceinline__ uint16_t keep1(uint16_t x, uint16_t g) {
  return le0((uint32_t)x << 16) ? (uint16_t)0 : g;
}

// the loaded chunk is live here: keeps the compiler from sinking a load below another chunk's store
__device__ __forceinline__ void pin(uint4& v) { asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w)); }

// index of the source whose channel range holds c (unused entries start at INT_MAX)
__device__ __forceinline__ int find_src(const Table& tb, int c) {
  int i = 0;
#pragma unroll
  for (int j = 1; j < kMaxSrc; ++j) i += c >= tb.s[j].off ? 1 : 0;
  return i;
}

// Both vector kernels are free of branches up to the stores: a chunk past the row's end is clamped
// to the last one and a pixel outside its source's map to the nearest inside (loaded, then dropped).
// Forward, the kChunks record fetches are issued one prefix scan apart with no wait between them,
// then the kChunks data loads back to back, then the stores.
template <bool RELU>
__global__ void __launch_bounds__(256) concat_fwd_vec_k(const Table tb, const uint32_t magic,
                                                        uint4* __restrict__ out) {
  const int row = blockIdx.x;  // b * m + y
  const int b = row / tb.m, y = row - b * tb.m;
  const int Ct8 = tb.Ct >> 3;
  const int nq = tb.m * Ct8;  // chunks of the row
  const int q0 = blockIdx.y * (blockDim.x * kChunks) + threadIdx.x;
  int x[kChunks], c8[kChunks], i[kChunks];
#pragma unroll
  for (int u = 0; u < kChunks; ++u) {
    const int q = min(q0 + u * (int)blockDim.x, nq - 1);
    x[u] = Ct8 == 1 ? q : (int)__umulhi((uint32_t)q, magic);
    c8[u] = q - x[u] * Ct8;
    i[u] = find_src(tb, c8[u] << 3);
  }
  const uint4* src[kChunks];
  bool inside[kChunks];
#pragma unroll
  for (int u = 0; u < kChunks; ++u) {
    const Src& s = tb.s[i[u]];  // a per-lane read of the kernel arguments
    const int H = s.H, sy = y - s.t, sx = x[u] - s.t;
    const int cy = min(max(sy, 0), H - 1), cx = min(max(sx, 0), H - 1);
    inside[u] = sy == cy && sx == cx;
    src[u] = static_cast<const uint4*>(s.x) + (((b * H + cy) * H + cx) * (s.C >> 3) + c8[u] - (s.off >> 3));
  }
  uint4 v[kChunks];
#pragma unroll
  for (int u = 0; u < kChunks; ++u) v[u] = *src[u];
#pragma unroll
  for (int u = 0; u < kChunks; ++u) pin(v[u]);
#pragma unroll
  for (int u = 0; u < kChunks; ++u) {
    const int q = q0 + u * (int)blockDim.x;
    if (!inside[u]) v[u] = make_uint4(0u, 0u, 0u, 0u);
    if (q < nq) out[row * nq + q] = RELU ? keep8(v[u], v[u]) : v[u];
  }
}

template <bool RELU>
__global__ void __launch_bounds__(256) concat_bwd_vec_k(const Table tb, const uint4* __restrict__ gout,
                                                        const int gs8) {
  const int r = blockIdx.x;  // a (b, y) row of one source: which one is uniform
  int i = 0;
#pragma unroll
  for (int j = 1; j < kMaxSrc; ++j) i += r >= tb.s[j].row0 ? 1 : 0;
  const Src s = tb.s[i];
  const int C8 = s.C >> 3;
  const int nq = s.H * C8;
  const int q0 = blockIdx.y * (blockDim.x * kChunks) + threadIdx.x;
  if (q0 - (int)threadIdx.x >= nq) return;  // a segment past this source's row
  const int rr = r - s.row0;                // b * H + y
  const int b = rr / s.H, y = rr - b * s.H;
  const uint4* __restrict__ xs = static_cast<const uint4*>(s.x) + rr * nq;
  uint4* __restrict__ gx = static_cast<uint4*>(s.gx) + rr * nq;
  const uint4* __restrict__ grow = gout + (((b * tb.m + y + s.t) * tb.m + s.t) * gs8 + (s.off >> 3));
  uint4 g[kChunks], xv[kChunks];
#pragma unroll
  for (int u = 0; u < kChunks; ++u) {
    const int q = min(q0 + u * (int)blockDim.x, nq - 1);
    const int x = C8 == 1 ? q : (int)__umulhi((uint32_t)q, s.magic);
    g[u] = grow[x * gs8 + q - x * C8];
    if (RELU) xv[u] = xs[q];
  }
#pragma unroll
  for (int u = 0; u < kChunks; ++u) {
    pin(g[u]);
    if (RELU) pin(xv[u]);
  }
#pragma unroll
  for (int u = 0; u < kChunks; ++u) {
    const int q = q0 + u * (int)blockDim.x;
    if (q < nq) gx[q] = RELU ? keep8(xv[u], g[u]) : g[u];
  }
}

template <bool RELU>
__global__ void __launch_bounds__(256) concat_fwd_elem_k(const Table tb, const int total,
                                                         uint16_t* __restrict__ out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int p = e / tb.Ct, c = e - p * tb.Ct;
  const int r = p / tb.m, x = p - r * tb.m;
  const int b = r / tb.m, y = r - b * tb.m;
  const int i = find_src(tb, c);
  const int H = tb.s[i].H, sy = y - tb.s[i].t, sx = x - tb.s[i].t;
  uint16_t v = 0;
  if ((unsigned)sy < (unsigned)H && (unsigned)sx < (unsigned)H)
    v = static_cast<const uint16_t*>(tb.s[i].x)[((b * H + sy) * H + sx) * tb.s[i].C + c - tb.s[i].off];
  out[e] = RELU ? keep1(v, v) : v;
}

// blockIdx.y is the source
template <bool RELU>
__global__ void __launch_bounds__(256) concat_bwd_elem_k(const Table tb, const uint16_t* __restrict__ gout,
                                                         const int gs) {
  const Src s = tb.s[blockIdx.y];
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (s.gx == nullptr || e >= tb.B * s.H * s.H * s.C) return;
  const int p = e / s.C, c = e - p * s.C;
  const int r = p / s.H, x = p - r * s.H;
  const int b = r / s.H, y = r - b * s.H;
  const uint16_t g = gout[((b * tb.m + y + s.t) * tb.m + x + s.t) * gs + s.off + c];
  static_cast<uint16_t*>(s.gx)[e] = RELU ? keep1(static_cast<const uint16_t*>(s.x)[e], g) : g;
}

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

uint32_t magic_of(int d) { return d <= 1 ? 0u : (uint32_t)(((1ull << 32) + d - 1) / d); }

int threads_for(int nq) { return nq <= 64 ? 64 : (nq <= 128 ? 128 : 256); }

}  // namespace

bool finish(Table& tb, int64_t gs) {
  if (tb.n < 1 || tb.n > kMaxSrc || tb.B < 1) return false;
  int64_t m = 0, Ct = 0;
  for (int i = 0; i < tb.n; ++i) {
    if (tb.s[i].H < 1 || tb.s[i].C < 1) return false;
    m = tb.s[i].H > m ? tb.s[i].H : m;
    Ct += tb.s[i].C;
  }
  if (gs < Ct) gs = Ct;
  if ((int64_t)tb.B * m * m * gs >= (1ll << 31)) return false;  // 32-bit indices in the kernels
  if (m * (Ct / 8 + 1) * (Ct / 8 + 1) >= (1ll << 32)) return false;  // chunk * magic stays exact
  tb.m = (int)m;
  tb.Ct = (int)Ct;
  int off = 0, rows = 0;
  for (int i = 0; i < kMaxSrc; ++i) {
    Src& s = tb.s[i];
    if (i >= tb.n) {
      s = Src{nullptr, nullptr, 0, 0, INT_MAX, 0, INT_MAX, 0u};
      continue;
    }
    s.off = off;
    s.t = (tb.m - s.H) / 2;
    s.row0 = rows;
    s.magic = s.C % 8 == 0 ? magic_of(s.C / 8) : 0u;
    off += s.C;
    if (s.gx != nullptr) rows += tb.B * s.H;
  }
  return true;
}

bool vector_ok(const Table& tb, const void* dense, int64_t gs, bool backward) {
  if (!aligned16(dense) || (backward && gs % 8 != 0)) return false;
  for (int i = 0; i < tb.n; ++i)
    if (tb.s[i].C % 8 != 0 || !aligned16(tb.s[i].x) || !aligned16(tb.s[i].gx)) return false;
  return true;
}

hipError_t launch_fwd(const Table& tb, bool relu, void* out, hipStream_t st) {
  if (vector_ok(tb, out, tb.Ct, false)) {
    const int nq = tb.m * (tb.Ct / 8), th = threads_for(nq);
    const dim3 grid(tb.B * tb.m, (nq + th * kChunks - 1) / (th * kChunks));
    if (grid.y > 65535u) return hipErrorInvalidValue;
    if (relu)
      hipLaunchKernelGGL(concat_fwd_vec_k<true>, grid, dim3(th), 0, st, tb, magic_of(tb.Ct / 8),
                         static_cast<uint4*>(out));
    else
      hipLaunchKernelGGL(concat_fwd_vec_k<false>, grid, dim3(th), 0, st, tb, magic_of(tb.Ct / 8),
                         static_cast<uint4*>(out));
  } else {
    const int total = tb.B * tb.m * tb.m * tb.Ct;
    const dim3 grid((total + 255) / 256);
    if (relu)
      hipLaunchKernelGGL(concat_fwd_elem_k<true>, grid, dim3(256), 0, st, tb, total, static_cast<uint16_t*>(out));
    else
      hipLaunchKernelGGL(concat_fwd_elem_k<false>, grid, dim3(256), 0, st, tb, total, static_cast<uint16_t*>(out));
  }
  return hipGetLastError();
}

hipError_t launch_bwd(const Table& tb, bool relu, const void* gout, int gs, hipStream_t st) {
  int rows = 0, nq = 0, numel = 0;  // over the sources that get a gradient
  for (int i = 0; i < tb.n; ++i) {
    const Src& s = tb.s[i];
    if (s.gx == nullptr) continue;
    rows += tb.B * s.H;
    nq = s.H * (s.C / 8) > nq ? s.H * (s.C / 8) : nq;
    numel = tb.B * s.H * s.H * s.C > numel ? tb.B * s.H * s.H * s.C : numel;
  }
  if (rows == 0) return hipSuccess;
  if (vector_ok(tb, gout, gs, true)) {
    const int th = threads_for(nq);
    const dim3 grid(rows, (nq + th * kChunks - 1) / (th * kChunks));
    if (grid.y > 65535u) return hipErrorInvalidValue;
    if (relu)
      hipLaunchKernelGGL(concat_bwd_vec_k<true>, grid, dim3(th), 0, st, tb, static_cast<const uint4*>(gout), gs / 8);
    else
      hipLaunchKernelGGL(concat_bwd_vec_k<false>, grid, dim3(th), 0, st, tb, static_cast<const uint4*>(gout), gs / 8);
  } else {
    const dim3 grid((numel + 255) / 256, tb.n);
    if (relu)
      hipLaunchKernelGGL(concat_bwd_elem_k<true>, grid, dim3(256), 0, st, tb, static_cast<const uint16_t*>(gout), gs);
    else
      hipLaunchKernelGGL(concat_bwd_elem_k<false>, grid, dim3(256), 0, st, tb, static_cast<const uint16_t*>(gout), gs);
  }
  return hipGetLastError();
}

}  // namespace enasconcat
}  // namespace katib_hip
