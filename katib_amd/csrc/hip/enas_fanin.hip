// Gradient fan-in of an ENAS child layer: layer i is read by layer i + 1 and by every later layer
// whose skip bit selects it, each through its own pad + concat (+ ReLU), so its gradient is a sum with
// one term per reader (enas_fanin.h has the formula). One launch forms that sum where it reads: n
// gradient reads, one read of x for the ReLU mask, one write, one rounding from an fp32 sum - in
// place of a full-size gradient per reader and n - 1 bf16 adds between them.
//
// Work split. The term table travels by value in the kernel arguments. A workgroup owns one (b, y)
// row of the producer (64, 128 or 256 threads by row length, blockIdx.y the segment of a row longer
// than kChunks chunks a thread), so the row, the batch index and with them the first chunk of every
// term's row are uniform: n scalar address computations a workgroup, and per chunk one multiply-high
// (chunk -> pixel) and one multiply-add per term. A thread owns up to kChunks 16-byte chunks (8
// channels) and takes them in_flight(N) at a time: the x load and all n term loads of those chunks
// are issued before the first add, in one basic block - no load depends on another, and s_waitcnt
// vmcnt retires loads in issue order, so the adds of term k wait for terms 0 .. k only while the rest
// are still in flight. Two fp32 x 8 accumulators a chunk, behind the ReLU mask and past it; a chunk
// ends with one select, one rounding and one 16-byte store. A chunk past the row's end is clamped to
// the last one (loaded, then dropped), so there is no branch per lane before the store.
//
// Templates. N is the number of terms, exact, so the load phase has no branch at all (a branch per
// absent slot would split it into blocks with a full wait at each join). SH is the launch's one
// non-zero off % 8: a reader that took the 3-channel image as a skip source under pad8 has everything
// behind the image at 3 mod 8, and such a term is two aligned 16-byte loads of one pixel plus the
// inverse funnel shift of the shifted concat backward (enas_chunk.h). Which terms are shifted is a bit
// mask in the table; in a launch with SH != 0 every term loads a second chunk, the next one if it is
// shifted and the same one again if not, and a uniform select keeps the funnel or the plain chunk. With
// no ReLU term the x load is pointed at term 0's chunk instead (x is not read) and its value unused.
//
// The mask is a select on the bits of x (x <= 0 and no NaN drops the masked sum), so a NaN in g
// passes where x > 0 and does not where x <= 0, exactly as in the concat backward. No LDS, no
// atomics, 32-bit indices (checked by finish()).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "enas_chunk.h"
#include "enas_fanin.h"

namespace katib_hip {
namespace enasfanin {

namespace {

using enaschunk::funnel;
using enaschunk::le0;

constexpr int kChunks = 4;  // 16-byte chunks per thread

// chunks of a thread whose loads are issued together: 1 + N (SH: 1 + 2 N) 16-byte loads each
constexpr int in_flight(int N) { return N <= 2 ? 4 : (N <= 5 ? 2 : 1); }

__device__ __forceinline__ void add8(float (&a)[8], const uint4& v) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    a[2 * j] += __uint_as_float(w[j] << 16);
    a[2 * j + 1] += __uint_as_float(w[j] & 0xffff0000u);
  }
}

__device__ __forceinline__ uint32_t bf16_bits(float f) {
  return (uint32_t)__builtin_bit_cast(uint16_t, (__bf16)f);  // round to nearest even
}

template <int N, int SH>
__global__ void __launch_bounds__(256) fanin_k(const Table tb, uint4* __restrict__ gx) {
  constexpr int U = in_flight(N);
  const int row = blockIdx.x;  // b * H + y
  const int b = row / tb.H, y = row - b * tb.H;
  const int C8 = tb.C8, nq = tb.H * C8;  // chunks of the row
  const int bd = blockDim.x, seg0 = blockIdx.y * (bd * kChunks);
  const bool mask = tb.relu != 0u;
  const uint4* __restrict__ xs = static_cast<const uint4*>(tb.x) + row * nq;
  // first chunk of the row in every term: uniform
  const uint4* base[N];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const Term& t = tb.k[k];
    base[k] = static_cast<const uint4*>(t.g) + (((b * t.m + y + t.t) * t.m + t.t) * t.gs8 + t.off8);
  }
#pragma unroll 1
  for (int u0 = 0; u0 < kChunks; u0 += U) {
    if (seg0 + u0 * bd >= nq) break;  // uniform: nothing of the row left for this workgroup
    int q[U];
    uint4 xv[U], g[U][N], h[U][SH ? N : 1];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      q[u] = min(seg0 + (u0 + u) * bd + (int)threadIdx.x, nq - 1);
      const int px = C8 == 1 ? q[u] : (int)__umulhi((uint32_t)q[u], tb.magic);
      const int c8 = q[u] - px * C8;
      const uint4* p[N];
#pragma unroll
      for (int k = 0; k < N; ++k) p[k] = base[k] + (px * tb.k[k].gs8 + c8);
      xv[u] = *(mask ? xs + q[u] : p[0]);
#pragma unroll
      for (int k = 0; k < N; ++k) {
        g[u][k] = p[k][0];
        if (SH) h[u][k] = p[k][tb.shift >> k & 1u];
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float am[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, au[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < N; ++k) {
        uint4 v = g[u][k];
        if (SH) {
          const uint4 f = funnel<(SH ? SH : 1)>(g[u][k], h[u][k]);
          if (tb.shift >> k & 1u) v = f;  // uniform: four selects
        }
        if (tb.relu >> k & 1u)  // uniform, and past the loads
          add8(am, v);
        else
          add8(au, v);
      }
      const uint32_t xw[4] = {xv[u].x, xv[u].y, xv[u].z, xv[u].w};
      uint32_t o[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {  // without a ReLU term am is zero, whatever xv holds
        const float lo = (le0(xw[j] << 16) ? 0.f : am[2 * j]) + au[2 * j];
        const float hi = (le0(xw[j] & 0xffff0000u) ? 0.f : am[2 * j + 1]) + au[2 * j + 1];
        o[j] = bf16_bits(lo) | bf16_bits(hi) << 16;
      }
      if (seg0 + (u0 + u) * bd + (int)threadIdx.x < nq) gx[row * nq + q[u]] = make_uint4(o[0], o[1], o[2], o[3]);
    }
  }
}

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

template <int N>
hipError_t launch_n(const Table& tb, uint4* gx, dim3 grid, int th, hipStream_t st) {
  switch (tb.sh) {
    case 0: hipLaunchKernelGGL((fanin_k<N, 0>), grid, dim3(th), 0, st, tb, gx); break;
    case 1: hipLaunchKernelGGL((fanin_k<N, 1>), grid, dim3(th), 0, st, tb, gx); break;
    case 2: hipLaunchKernelGGL((fanin_k<N, 2>), grid, dim3(th), 0, st, tb, gx); break;
    case 3: hipLaunchKernelGGL((fanin_k<N, 3>), grid, dim3(th), 0, st, tb, gx); break;
    case 4: hipLaunchKernelGGL((fanin_k<N, 4>), grid, dim3(th), 0, st, tb, gx); break;
    case 5: hipLaunchKernelGGL((fanin_k<N, 5>), grid, dim3(th), 0, st, tb, gx); break;
    case 6: hipLaunchKernelGGL((fanin_k<N, 6>), grid, dim3(th), 0, st, tb, gx); break;
    case 7: hipLaunchKernelGGL((fanin_k<N, 7>), grid, dim3(th), 0, st, tb, gx); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace

const char* finish(Table& tb, const void* gx) {
  if (tb.n < 1 || tb.n > kMaxTerms) return "1 to 16 terms";
  if (tb.B < 1 || tb.H < 1 || tb.C8 < 1) return "empty producer";
  if ((int64_t)tb.B * tb.H * tb.H * tb.C8 * 8 >= (1ll << 31)) return "B * H * H * C >= 2^31";
  if ((int64_t)tb.H * tb.C8 * tb.C8 >= (1ll << 32)) return "row too long for the chunk arithmetic";
  if (gx == nullptr || !aligned16(gx)) return "gx must be 16-byte aligned";
  if (tb.n < 32 && (tb.relu >> tb.n || tb.shift >> tb.n)) return "a flag past the last term";
  if (tb.relu && (tb.x == nullptr || !aligned16(tb.x))) return "a ReLU term needs x, 16-byte aligned";
  if (tb.shift ? tb.sh < 1 || tb.sh > 7 : tb.sh != 0) return "shifted terms share one off % 8 in 1 .. 7";
  for (int k = 0; k < tb.n; ++k) {
    const Term& t = tb.k[k];
    if (t.g == nullptr || !aligned16(t.g)) return "a term's gradient must be 16-byte aligned";
    if (t.m < tb.H || t.t != (t.m - tb.H) / 2) return "a term's map is smaller than the producer's";
    if (t.gs8 < 1 || t.off8 < 0) return "a term's pixel stride or offset is out of range";
    // the last chunk read of a pixel lies inside the pixel's stride
    if ((int64_t)t.off8 + tb.C8 + (tb.shift >> k & 1u) > t.gs8) return "a term's channels reach past its pixel stride";
    if ((int64_t)tb.B * t.m * t.m * t.gs8 * 8 >= (1ll << 31)) return "B * m * m * gs >= 2^31";
  }
  tb.magic = tb.C8 <= 1 ? 0u : (uint32_t)(((1ull << 32) + tb.C8 - 1) / tb.C8);
  return nullptr;
}

hipError_t launch(const Table& tb, void* gx, hipStream_t st) {
  const int nq = tb.H * tb.C8, th = nq <= 64 ? 64 : (nq <= 128 ? 128 : 256);
  const dim3 grid(tb.B * tb.H, (nq + th * kChunks - 1) / (th * kChunks));
  if (grid.y > 65535u) return hipErrorInvalidValue;
  uint4* out = static_cast<uint4*>(gx);
  switch (tb.n) {
#define KATIB_FANIN_N(n) \
  case n: return launch_n<n>(tb, out, grid, th, st);
    KATIB_FANIN_N(1) KATIB_FANIN_N(2) KATIB_FANIN_N(3) KATIB_FANIN_N(4) KATIB_FANIN_N(5) KATIB_FANIN_N(6)
    KATIB_FANIN_N(7) KATIB_FANIN_N(8) KATIB_FANIN_N(9) KATIB_FANIN_N(10) KATIB_FANIN_N(11) KATIB_FANIN_N(12)
    KATIB_FANIN_N(13) KATIB_FANIN_N(14) KATIB_FANIN_N(15) KATIB_FANIN_N(16)
#undef KATIB_FANIN_N
    default: return hipErrorInvalidValue;
  }
}

}  // namespace enasfanin
}  // namespace katib_hip
