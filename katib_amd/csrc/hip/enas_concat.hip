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
// pad8: an output pixel holds Cs = 8 ceil(Ct / 8) channels, the last Cs - Ct zeros written by the
// kernel (no memset), and gout comes over Cs channels of which only the first Ct are ever used.
// Shifted vector path (pad8, one source of C < 8 channels - the 3-channel image as a skip source -
// among sources with C % 8 == 0, Ct = 67, 131, ...): the same work mapping over the table of the
// aligned sources alone; every output chunk behind the narrow source is a funnel shift by C bf16
// over two aligned 16-byte loads, done in registers (dword renaming + v_alignbyte_b32), the chunk
// at the narrow source takes its C values by 2-byte loads, and the half past the last source is
// the zero pad. Backward the inverse shift over two gout chunks of one pixel; C is a template
// parameter, the narrow source's chunk index a kernel argument.
// Element path (anything else: several narrow sources, no pad8 with an odd channel sum, a gout
// pixel stride that is no multiple of 8): one thread per element with scalar accesses and plain
// divisions; correct, not fast. With pad8 it writes the zero pad too.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "enas_chunk.h"
#include "enas_concat.h"

namespace katib_hip {
namespace enasconcat {

namespace {

constexpr int kChunks = 4;  // 16-byte chunks per thread, all in flight together

using enaschunk::funnel;  // enas_chunk.h: shared with the gradient fan-in
using enaschunk::le0;
using enaschunk::pin;

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

// ---- shifted vector path: one source of C < 8 channels among sources with C % 8 == 0 -------------
// `ta` is the table of the aligned sources alone (D', A8 chunks a pixel), `nr` the narrow source at
// chunk o8 of D'. An output pixel has A8 + 1 chunks: chunk k < o8 is D' chunk k; chunk o8 is the C
// narrow values, then the first 8 - C of D' chunk o8; chunk k > o8 is the last C of D' chunk k - 1,
// then the first 8 - C of D' chunk k, and D' chunk A8 is zeros (the pad channels). Backward, a source
// at or behind o8 reads its chunk j from the last 8 - C of gout chunk off / 8 + j and the first C of
// the next one.

// (funnel<S>, the shift itself, is in enas_chunk.h)

// Like concat_fwd_vec_k: no branch before the stores; the record fetches first (two a chunk, one
// per half), then all 16-byte loads back to back, then the narrow source's C values of the chunk's
// pixel (every lane loads them from a clamped address, the lanes of chunk o8 keep them: a branch
// here would put a wait for everything in flight into each chunk), pin, shift, ReLU, stores. Each
// half has its own inside-the-map test and is zeroed before the shift: the halves may come from
// sources with different H and t.
template <int C, bool RELU>
__global__ void __launch_bounds__(256) concat_fwd_shift_k(const Table ta, const Narrow nr, const uint32_t magic,
                                                          uint4* __restrict__ out) {
  const int row = blockIdx.x;  // b * m + y
  const int b = row / ta.m, y = row - b * ta.m;
  const int A8 = ta.Ct >> 3, Cs8 = A8 + 1;
  const int nq = ta.m * Cs8;  // chunks of the row
  const int q0 = blockIdx.y * (blockDim.x * kChunks) + threadIdx.x;
  int x[kChunks], k8[kChunks], ka[kChunks], kb[kChunks], ia[kChunks], ib[kChunks];
#pragma unroll
  for (int u = 0; u < kChunks; ++u) {
    const int q = min(q0 + u * (int)blockDim.x, nq - 1);
    x[u] = (int)__umulhi((uint32_t)q, magic);  // Cs8 >= 2
    k8[u] = q - x[u] * Cs8;
    kb[u] = min(k8[u], A8 - 1);      // the chunk of D' at k, clamped into D'
    ka[u] = max(kb[u] - (k8[u] < A8 ? 1 : 0), 0);  // the one before chunk k
    ib[u] = find_src(ta, kb[u] << 3);
    ia[u] = find_src(ta, ka[u] << 3);
  }
  const uint4 *pa[kChunks], *pb[kChunks];
  const uint16_t* pn[kChunks];
  bool ina[kChunks], inb[kChunks], inn[kChunks];
#pragma unroll
  for (int u = 0; u < kChunks; ++u) {
    {
      const Src& s = ta.s[ib[u]];
      const int H = s.H, sy = y - s.t, sx = x[u] - s.t;
      const int cy = min(max(sy, 0), H - 1), cx = min(max(sx, 0), H - 1);
      inb[u] = sy == cy && sx == cx && k8[u] < A8;
      pb[u] = static_cast<const uint4*>(s.x) + (((b * H + cy) * H + cx) * (s.C >> 3) + kb[u] - (s.off >> 3));
    }
    {
      const Src& s = ta.s[ia[u]];
      const int H = s.H, sy = y - s.t, sx = x[u] - s.t;
      const int cy = min(max(sy, 0), H - 1), cx = min(max(sx, 0), H - 1);
      ina[u] = sy == cy && sx == cx && k8[u] > nr.o8;
      pa[u] = static_cast<const uint4*>(s.x) + (((b * H + cy) * H + cx) * (s.C >> 3) + ka[u] - (s.off >> 3));
    }
    {
      const int H = nr.H, sy = y - nr.t, sx = x[u] - nr.t;
      const int cy = min(max(sy, 0), H - 1), cx = min(max(sx, 0), H - 1);
      inn[u] = sy == cy && sx == cx && k8[u] == nr.o8;
      pn[u] = static_cast<const uint16_t*>(nr.x) + ((b * H + cy) * H + cx) * C;
    }
  }
  uint4 va[kChunks], vb[kChunks];
  uint32_t vn[kChunks][C];
#pragma unroll
  for (int u = 0; u < kChunks; ++u) {
    vb[u] = *pb[u];
    va[u] = *pa[u];
  }
#pragma unroll
  for (int u = 0; u < kChunks; ++u)
#pragma unroll
    for (int e = 0; e < C; ++e) vn[u][e] = pn[u][e];
#pragma unroll
  for (int u = 0; u < kChunks; ++u) {
    pin(vb[u]);
    pin(va[u]);
#pragma unroll
    for (int e = 0; e < C; ++e) asm volatile("" : "+v"(vn[u][e]));
  }
#pragma unroll
  for (int u = 0; u < kChunks; ++u) {
    const int q = q0 + u * (int)blockDim.x;
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    if (!inb[u]) vb[u] = z;
    if (!ina[u]) va[u] = z;
    // the narrow values as the last C elements of the low half (zeros on every other lane)
    uint32_t lo[4] = {va[u].x, va[u].y, va[u].z, va[u].w};
#pragma unroll
    for (int e = 0; e < C; ++e) lo[(8 - C + e) >> 1] |= (inn[u] ? vn[u][e] : 0u) << (((8 - C + e) & 1) * 16);
    const uint4 sh = funnel<8 - C>(make_uint4(lo[0], lo[1], lo[2], lo[3]), vb[u]);
    const uint4 v = k8[u] < nr.o8 ? vb[u] : sh;
    if (q < nq) out[row * nq + q] = RELU ? keep8(v, v) : v;
  }
}

// One source's row: SH = 0 reads gout like concat_bwd_vec_k, SH = C is the inverse funnel shift
// over a gout chunk and the next one of the same pixel (both inside Cs <= gs).
template <int SH, bool RELU>
__device__ __forceinline__ void bwd_shift_row(const Src& s, const int rr, const int m, const uint4* __restrict__ gout,
                                              const int gs8, const int g0) {
  const int C8 = s.C >> 3;
  const int nq = s.H * C8;
  const int q0 = blockIdx.y * (blockDim.x * kChunks) + threadIdx.x;
  const int b = rr / s.H, y = rr - b * s.H;
  const uint4* __restrict__ xs = static_cast<const uint4*>(s.x) + rr * nq;
  uint4* __restrict__ gx = static_cast<uint4*>(s.gx) + rr * nq;
  const uint4* __restrict__ grow = gout + (((b * m + y + s.t) * m + s.t) * gs8 + g0);
  uint4 g[kChunks], h[kChunks], xv[kChunks];
#pragma unroll
  for (int u = 0; u < kChunks; ++u) {
    const int q = min(q0 + u * (int)blockDim.x, nq - 1);
    const int x = C8 == 1 ? q : (int)__umulhi((uint32_t)q, s.magic);
    g[u] = grow[x * gs8 + q - x * C8];
    if (SH) h[u] = grow[x * gs8 + q - x * C8 + 1];
    if (RELU) xv[u] = xs[q];
  }
#pragma unroll
  for (int u = 0; u < kChunks; ++u) {
    pin(g[u]);
    if (SH) pin(h[u]);
    if (RELU) pin(xv[u]);
  }
#pragma unroll
  for (int u = 0; u < kChunks; ++u) {
    const int q = q0 + u * (int)blockDim.x;
    const uint4 v = SH ? funnel<SH>(g[u], h[u]) : g[u];
    if (q < nq) gx[q] = RELU ? keep8(xv[u], v) : v;
  }
}

// a workgroup owns a (b, y) row of one source of `ta` (the narrow source gets no workgroups), so
// whether the row is shifted is uniform
template <int C, bool RELU>
__global__ void __launch_bounds__(256) concat_bwd_shift_k(const Table ta, const int o8, const uint4* __restrict__ gout,
                                                          const int gs8) {
  const int r = blockIdx.x;
  int i = 0;
#pragma unroll
  for (int j = 1; j < kMaxSrc; ++j) i += r >= ta.s[j].row0 ? 1 : 0;
  const Src s = ta.s[i];
  if ((int)(blockIdx.y * (blockDim.x * kChunks)) >= s.H * (s.C >> 3)) return;  // a segment past this source's row
  if ((s.off >> 3) >= o8)
    bwd_shift_row<C, RELU>(s, r - s.row0, ta.m, gout, gs8, s.off >> 3);
  else
    bwd_shift_row<0, RELU>(s, r - s.row0, ta.m, gout, gs8, s.off >> 3);
}

// the output pixel has tb.Cs >= tb.Ct channels: the pad channels get zeros
template <bool RELU>
__global__ void __launch_bounds__(256) concat_fwd_elem_k(const Table tb, const int total,
                                                         uint16_t* __restrict__ out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int p = e / tb.Cs, c = e - p * tb.Cs;
  const int r = p / tb.m, x = p - r * tb.m;
  const int b = r / tb.m, y = r - b * tb.m;
  const int i = find_src(tb, c);
  const int H = tb.s[i].H, sy = y - tb.s[i].t, sx = x - tb.s[i].t;
  uint16_t v = 0;
  if (c < tb.Ct && (unsigned)sy < (unsigned)H && (unsigned)sx < (unsigned)H)
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

// The aligned sources of tb alone, with their own prefix and first rows (D' of the shifted path).
Table without_narrow(const Table& tb) {
  Table ta = tb;
  int n = 0, off = 0, rows = 0;
  for (int i = 0; i < kMaxSrc; ++i) {
    if (i >= tb.n || i == tb.nar) continue;
    Src& s = ta.s[n++];
    s = tb.s[i];
    s.off = off;
    s.row0 = rows;
    off += s.C;
    if (s.gx != nullptr) rows += tb.B * s.H;
  }
  for (int i = n; i < kMaxSrc; ++i) ta.s[i] = Src{nullptr, nullptr, 0, 0, INT_MAX, 0, INT_MAX, 0u};
  ta.n = n;
  ta.Ct = off;
  ta.Cs = off + 8;
  ta.nar = -1;
  return ta;
}

Narrow narrow_of(const Table& tb) {
  int o = 0;
  for (int i = 0; i < tb.nar; ++i) o += tb.s[i].C;
  return Narrow{tb.s[tb.nar].x, tb.s[tb.nar].H, tb.s[tb.nar].t, o / 8};
}

// K<c, relu> for the narrow width c = 1 .. 7
#define KATIB_CONCAT_SHIFT(K, c, relu, grid, th, st, ...)                                                   \
  switch ((c) * 2 + ((relu) ? 1 : 0)) {                                                                     \
    case 2: hipLaunchKernelGGL((K<1, false>), grid, dim3(th), 0, st, __VA_ARGS__); break;                   \
    case 3: hipLaunchKernelGGL((K<1, true>), grid, dim3(th), 0, st, __VA_ARGS__); break;                    \
    case 4: hipLaunchKernelGGL((K<2, false>), grid, dim3(th), 0, st, __VA_ARGS__); break;                   \
    case 5: hipLaunchKernelGGL((K<2, true>), grid, dim3(th), 0, st, __VA_ARGS__); break;                    \
    case 6: hipLaunchKernelGGL((K<3, false>), grid, dim3(th), 0, st, __VA_ARGS__); break;                   \
    case 7: hipLaunchKernelGGL((K<3, true>), grid, dim3(th), 0, st, __VA_ARGS__); break;                    \
    case 8: hipLaunchKernelGGL((K<4, false>), grid, dim3(th), 0, st, __VA_ARGS__); break;                   \
    case 9: hipLaunchKernelGGL((K<4, true>), grid, dim3(th), 0, st, __VA_ARGS__); break;                    \
    case 10: hipLaunchKernelGGL((K<5, false>), grid, dim3(th), 0, st, __VA_ARGS__); break;                  \
    case 11: hipLaunchKernelGGL((K<5, true>), grid, dim3(th), 0, st, __VA_ARGS__); break;                   \
    case 12: hipLaunchKernelGGL((K<6, false>), grid, dim3(th), 0, st, __VA_ARGS__); break;                  \
    case 13: hipLaunchKernelGGL((K<6, true>), grid, dim3(th), 0, st, __VA_ARGS__); break;                   \
    case 14: hipLaunchKernelGGL((K<7, false>), grid, dim3(th), 0, st, __VA_ARGS__); break;                  \
    case 15: hipLaunchKernelGGL((K<7, true>), grid, dim3(th), 0, st, __VA_ARGS__); break;                   \
    default: return hipErrorInvalidValue;                                                                   \
  }

}  // namespace

bool finish(Table& tb, int64_t gs, bool pad8) {
  if (tb.n < 1 || tb.n > kMaxSrc || tb.B < 1) return false;
  int64_t m = 0, Ct = 0;
  int narrow = 0, ragged = 0, nar = -1;  // sources with C < 8; wider ones with C % 8 != 0
  for (int i = 0; i < tb.n; ++i) {
    if (tb.s[i].H < 1 || tb.s[i].C < 1) return false;
    m = tb.s[i].H > m ? tb.s[i].H : m;
    Ct += tb.s[i].C;
    if (tb.s[i].C < 8) {
      ++narrow;
      nar = i;
    } else if (tb.s[i].C % 8 != 0) {
      ++ragged;
    }
  }
  const int64_t Cs = pad8 ? (Ct + 7) / 8 * 8 : Ct;
  if (gs < Cs) gs = Cs;
  if ((int64_t)tb.B * m * m * gs >= (1ll << 31)) return false;  // 32-bit indices in the kernels
  if (m * (Ct / 8 + 1) * (Ct / 8 + 1) >= (1ll << 32)) return false;  // chunk * magic stays exact
  tb.m = (int)m;
  tb.Ct = (int)Ct;
  tb.Cs = (int)Cs;
  tb.nar = pad8 && narrow == 1 && ragged == 0 && tb.n >= 2 ? nar : -1;
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

bool shift_ok(const Table& tb, const void* dense, int64_t gs, bool backward) {
  if (tb.nar < 0 || !aligned16(dense) || (backward && (gs % 8 != 0 || gs < tb.Cs))) return false;
  for (int i = 0; i < tb.n; ++i) {
    const Src& s = tb.s[i];
    if (i == tb.nar ? s.gx != nullptr || reinterpret_cast<uintptr_t>(s.x) % 2 != 0
                    : !aligned16(s.x) || !aligned16(s.gx))
      return false;
  }
  return true;
}

hipError_t launch_fwd(const Table& tb, bool relu, void* out, hipStream_t st) {
  if (shift_ok(tb, out, tb.Cs, false)) {
    const Table ta = without_narrow(tb);
    const int nq = tb.m * (tb.Cs / 8), th = threads_for(nq);
    const dim3 grid(tb.B * tb.m, (nq + th * kChunks - 1) / (th * kChunks));
    if (grid.y > 65535u) return hipErrorInvalidValue;
    KATIB_CONCAT_SHIFT(concat_fwd_shift_k, tb.s[tb.nar].C, relu, grid, th, st, ta, narrow_of(tb),
                       magic_of(tb.Cs / 8), static_cast<uint4*>(out));
    return hipGetLastError();
  }
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
    const int total = tb.B * tb.m * tb.m * tb.Cs;
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
  if (gs < tb.Cs) return hipErrorInvalidValue;
  if (shift_ok(tb, gout, gs, true)) {
    const Table ta = without_narrow(tb);
    const int th = threads_for(nq);
    const dim3 grid(rows, (nq + th * kChunks - 1) / (th * kChunks));
    if (grid.y > 65535u) return hipErrorInvalidValue;
    KATIB_CONCAT_SHIFT(concat_bwd_shift_k, tb.s[tb.nar].C, relu, grid, th, st, ta, narrow_of(tb).o8,
                       static_cast<const uint4*>(gout), gs / 8);
    return hipGetLastError();
  }
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
