// Fused MLP training kernels for gfx950 (BASELINE config 2: TPE over lr / batch size / width
// of an MNIST MLP; and the B1 search space: depth and optimizer). One train step
// of an MLP with L hidden layers is 3L + 3 launches (nine for 784 -> h -> h/2 -> 10), all
// graph-captured, with no separate bias, activation, gather, cast, loss or optimizer kernels:
//
//  lin_fwd    Y = act(X W^T + b): bf16 MFMA (v_mfma_f32_16x16x32_bf16) over K-contiguous
//             operands staged through padded LDS rows; optional row gather of X (the
//             minibatch indices into the device-resident dataset), bias + ReLU epilogue, or
//             a ReLU-derivative mask epilogue (dgrad: dX = (dY W) * [X_act > 0] with the
//             transposed bf16 weight shadow as the K-contiguous operand).
//  lin_fwd_splitk  the same product for K much larger than M (the Keras MNIST CNN's fc1: M <= 64, N = 128,
//             K = 21,632, two output tiles): the same main loop over slabs of SPLITK_KS columns, one workgroup
//             per slab and tile, into fp32 partials; a second launch sums a row's slabs in slab order, then
//             bias, ReLU and the bf16 rounding. No gather, no mask.
//  lin_wgrad dW = dY^T X reduced over the whole minibatch inside one workgroup (the
//             minibatch is the reduction, <= a few hundred rows), both operands read with
//             ds_read_b64_tr_b16, and the optimizer applied in the epilogue to the fp32
//             master and its state, with the bf16 weight and transposed-weight shadows
//             refreshed; the workgroups of the first K tile also reduce and update the bias.
//             One templated kernel (wgrad_k), three epilogues over its main loop: SGD with
//             momentum (wgrad_k<float>), Adam and FTRL-proximal (wgrad_k<Opt2<AdamUpd>>,
//             wgrad_k<Opt2<FtrlUpd>>). The latter two issue all of a thread's 48 state loads
//             before the first arithmetic.
//  xent_small cross-entropy + its gradient for a handful of classes, one lane per row. It
//             runs once per step between the previous step's last weight-gradient launch
//             and this step's first, so it is also where the device step counter (Adam's
//             t) advances: thread 0 of block 0 adds 1 when a counter is given.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>

#include <type_traits>

#include "mlp.h"
#include "mlp_optim.h"

namespace katib_hip {
namespace mlp {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef uint16_t u16;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

constexpr int BM = 64, BN = 64, BK = 64, PAD = 8, LD = BK + PAD;

__device__ __forceinline__ float bf2f(u16 b) { return __uint_as_float((uint32_t)b << 16); }
__device__ __forceinline__ u16 f2bf(float f) { return __builtin_bit_cast(u16, (__bf16)f); }

// ------------------------------------------------------------------ Y = epi(A B^T)
// The MFMA main loop of one 64 x 64 output tile at (m0, n0) over k in [kb, ke): A [M][K] (rows optionally
// gathered through idx), B [N][K], both K-contiguous; K % 8 == 0, kb % 8 == 0, ke % 8 == 0. smem holds
// 2 * (BM + BN) * LD elements. acc[a][b][j]: row m0 + wr * 32 + a * 16 + 4 * (lane >> 4) + j, column
// n0 + wc * 32 + b * 16 + (lane & 15); rows >= M and columns >= N accumulate zeros.
__device__ __forceinline__ void gemm_nt_tile(const u16* __restrict__ A, const int64_t* __restrict__ idx,
                                             const u16* __restrict__ B, int M, int N, int K, int m0, int n0, int kb,
                                             int ke, u16* smem, f32x4 (&acc)[2][2]) {
  u16* As = smem;
  u16* Bs = smem + 2 * BM * LD;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wr = wid >> 1, wc = wid & 1;
  const int kc = tid & 7, trow = tid >> 3;  // 32 rows x 8 chunks of 16 B per pass
  const u16* arow[2];
  const u16* brow[2];
  bool aok[2], bok[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int m = m0 + trow + 32 * i, n = n0 + trow + 32 * i;
    aok[i] = m < M;
    bok[i] = n < N;
    const int64_t am = aok[i] ? (idx ? idx[m] : m) : 0;
    arow[i] = A + am * K;
    brow[i] = B + (int64_t)(bok[i] ? n : 0) * K;
  }
  u32x4 ra[2], rb[2];
  const u32x4 zero = {0u, 0u, 0u, 0u};
  auto gload = [&](int kt) {
    const int kk = kb + kt * BK + kc * 8;
    const bool kin = kk < ke;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      ra[i] = (kin && aok[i]) ? *reinterpret_cast<const u32x4*>(arow[i] + kk) : zero;
      rb[i] = (kin && bok[i]) ? *reinterpret_cast<const u32x4*>(brow[i] + kk) : zero;
    }
  };
  auto sstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      *reinterpret_cast<u32x4*>(As + (buf * BM + trow + 32 * i) * LD + kc * 8) = ra[i];
      *reinterpret_cast<u32x4*>(Bs + (buf * BN + trow + 32 * i) * LD + kc * 8) = rb[i];
    }
  };
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nk = (ke - kb + BK - 1) / BK;
  gload(0);
  sstore(0);
  __syncthreads();
  const int fr = lane & 15, fk = 8 * (lane >> 4);
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) gload(kt + 1);
#pragma unroll
    for (int ks = 0; ks < BK / 32; ++ks) {
      bf16x8 af[2], bfr[2];
#pragma unroll
      for (int a = 0; a < 2; ++a)
        af[a] = __builtin_bit_cast(
            bf16x8, *reinterpret_cast<const u32x4*>(As + (buf * BM + wr * 32 + a * 16 + fr) * LD + ks * 32 + fk));
#pragma unroll
      for (int b = 0; b < 2; ++b)
        bfr[b] = __builtin_bit_cast(
            bf16x8, *reinterpret_cast<const u32x4*>(Bs + (buf * BN + wc * 32 + b * 16 + fr) * LD + ks * 32 + fk));
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[a], bfr[b], acc[a][b], 0, 0, 0);
    }
    if (kt + 1 < nk) sstore(buf ^ 1);
    __syncthreads();
  }
}

// epi: + bias, ReLU (relu != 0), or * [mask > 0] (mask [M][N] bf16). Output bf16 [M][N].
__global__ __launch_bounds__(256) void gemm_nt_k(const u16* __restrict__ A, const int64_t* __restrict__ idx,
                                                 const u16* __restrict__ B, const float* __restrict__ bias,
                                                 const u16* __restrict__ mask, u16* __restrict__ Y, int M, int N,
                                                 int K, int relu) {
  __shared__ __align__(16) u16 smem[2 * (BM + BN) * LD];
  const int tilesN = (N + BN - 1) / BN;
  const int m0 = (blockIdx.x / tilesN) * BM, n0 = (blockIdx.x % tilesN) * BN;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, wr = wid >> 1, wc = wid & 1, fr = lane & 15;
  f32x4 acc[2][2];
  gemm_nt_tile(A, idx, B, M, N, K, m0, n0, 0, K, smem, acc);
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int col = n0 + wc * 32 + b * 16 + fr;
      if (col >= N) continue;
      const float bv = bias ? bias[col] : 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = m0 + wr * 32 + a * 16 + 4 * (lane >> 4) + j;
        if (row >= M) continue;
        float v = acc[a][b][j] + bv;
        if (relu) v = fmaxf(v, 0.f);
        if (mask && !(bf2f(mask[(int64_t)row * N + col]) > 0.f)) v = 0.f;
        Y[(int64_t)row * N + col] = f2bf(v);
      }
    }
}

// ------------------------------------------------------------------ split-K: Y = act(A B^T + bias), K >> M
// Slab s of KS columns of one 64 x 64 tile per workgroup (the main loop above over [s KS, (s + 1) KS)), fp32
// partials P [slabs][M][N]; then splitk_reduce_k sums a row's slabs in slab order, adds the bias, applies ReLU
// and rounds. KS is a constant, so a row's result does not depend on M: not on the batch it sits in.
__global__ __launch_bounds__(256) void gemm_nt_slab_k(const u16* __restrict__ A, const u16* __restrict__ B,
                                                      float* __restrict__ P, int M, int N, int K) {
  __shared__ __align__(16) u16 smem[2 * (BM + BN) * LD];
  const int tilesN = (N + BN - 1) / BN, tilesM = (M + BM - 1) / BM;
  const int slab = blockIdx.x / (tilesM * tilesN), tile = blockIdx.x % (tilesM * tilesN);
  const int m0 = (tile / tilesN) * BM, n0 = (tile % tilesN) * BN;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, wr = wid >> 1, wc = wid & 1, fr = lane & 15;
  f32x4 acc[2][2];
  gemm_nt_tile(A, nullptr, B, M, N, K, m0, n0, slab * SPLITK_KS, min((slab + 1) * SPLITK_KS, K), smem, acc);
  float* __restrict__ Ps = P + (int64_t)slab * M * N;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int col = n0 + wc * 32 + b * 16 + fr;
      if (col >= N) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = m0 + wr * 32 + a * 16 + 4 * (lane >> 4) + j;
        if (row < M) Ps[(int64_t)row * N + col] = acc[a][b][j];
      }
    }
}

// one thread per 4 consecutive outputs (N % 4 == 0), 16 bytes per slab, summed in slab order
__global__ __launch_bounds__(256) void splitk_reduce_k(const float* __restrict__ P, int slabs,
                                                       const float* __restrict__ bias, u16* __restrict__ Y, int MN,
                                                       int N, int relu) {
  const int o = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (o >= MN) return;
  f32x4 s = *reinterpret_cast<const f32x4*>(P + o);
#pragma unroll 8
  for (int k = 1; k < slabs; ++k) s += *reinterpret_cast<const f32x4*>(P + (int64_t)k * MN + o);
  if (bias) s += *reinterpret_cast<const f32x4*>(bias + o % N);
  u16 h[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) h[j] = f2bf(relu ? fmaxf(s[j], 0.f) : s[j]);
  *reinterpret_cast<uint2*>(Y + o) = uint2{(uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16)};
}

// Element updates of the two-state optimizers: operator() takes the gradient, the element's two
// state values (updated in place) and its weight, and returns the new weight. Both leave an
// element with g = 0 and zero state exactly as it was (the padded output rows, dead ReLU units).
// AdamUpd (torch.optim.Adam, default flags: s0 = exp_avg, s1 = exp_avg_sq) is in mlp_optim.h, which
// mnist_tfcnn.hip shares.
// The trial's Ftrl class (FTRL-proximal as MXNet's), operation for operation: s0 = z, s1 = n.
struct FtrlUpd {
  float l1, beta, wd;
  float lr;
  __device__ __forceinline__ void init(float lr_) { lr = lr_; }
  __device__ __forceinline__ float operator()(float g, float& z, float& n, float w) const {
    const float sq_old = sqrtf(n);
    n += g * g;  // n only grows from >= 0: both square roots are of non-negative numbers
    const float sq = sqrtf(n);
    z += g - (sq - sq_old) / lr * w;
    const float sgn = z > 0.f ? 1.f : (z < 0.f ? -1.f : 0.f);
    return fabsf(z) > l1 ? (sgn * l1 - z) / ((beta + sq) / lr + wd) : 0.f;  // zero state, g = 0: z = 0, w = 0
  }
};

// A two-state optimizer as the kernel's last argument: the element update and the second state arrays.
template <class U>
struct Opt2 {
  typedef U Upd;
  U upd;
  float* s1;
  float* bs1;
};

// ------------------------------------------------------------------ dW = dY^T X, fused optimizers
// dY [M][N] bf16, X [M][K] bf16 (rows gathered through idx when given), W [N][K] fp32 master.
// One workgroup per 64 x 64 tile of W, reducing over all M rows. One kernel, three epilogues,
// chosen by the type of the last argument: float = SGD with momentum (S0 = the momentum buffer;
// this instantiation has the argument layout and the body the SGD-only kernel had), Opt2<U> = a
// two-state optimizer U (S0 and the Opt2's s1: Adam's m, v or FTRL's z, n).
template <class E>
__global__ __launch_bounds__(256) void wgrad_k(const u16* __restrict__ dY, const u16* __restrict__ X,
                                               const int64_t* __restrict__ idx, int M, int N, int K,
                                               float* __restrict__ W, float* __restrict__ S0,
                                               u16* __restrict__ W16, u16* __restrict__ W16t,
                                               float* __restrict__ bias, float* __restrict__ bs0,
                                               const float* __restrict__ lr_p, E e) {
  constexpr int BP = 64;
  constexpr int LDA = BN + PAD, LDB = BK + PAD;
  __shared__ __align__(16) u16 smem[2 * BP * (LDA + LDB)];
  __shared__ float bsum[4][64];
  u16* As = smem;                 // [buf][m][n]
  u16* Bs = smem + 2 * BP * LDA;  // [buf][m][k]
  const int tilesK = (K + BK - 1) / BK;
  const int n0 = (blockIdx.x / tilesK) * BN, k0 = (blockIdx.x % tilesK) * BK;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wr = wid >> 1, wc = wid & 1;
  const bool do_bias = bias != nullptr && k0 == 0;
  // 64 rows x 8 chunks per operand per stage: 2 chunks per thread each
  int prow[2], pch[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int id = tid + 256 * i;
    prow[i] = id >> 3;
    pch[i] = id & 7;
  }
  u32x4 ra[2], rb[2];
  const u32x4 zero = {0u, 0u, 0u, 0u};
  auto gload = [&](int p0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int m = p0 + prow[i];
      const int n = n0 + pch[i] * 8, k = k0 + pch[i] * 8;
      ra[i] = (m < M && n < N) ? *reinterpret_cast<const u32x4*>(dY + (int64_t)m * N + n) : zero;
      const int64_t xm = m < M ? (idx ? idx[m] : m) : 0;
      rb[i] = (m < M && k < K) ? *reinterpret_cast<const u32x4*>(X + xm * K + k) : zero;
    }
  };
  auto sstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      *reinterpret_cast<u32x4*>(As + (buf * BP + prow[i]) * LDA + pch[i] * 8) = ra[i];
      *reinterpret_cast<u32x4*>(Bs + (buf * BP + prow[i]) * LDB + pch[i] * 8) = rb[i];
    }
  };
  f32x4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bacc = 0.f;
  const int tg = lane >> 4, tq = (lane & 15) >> 2, tp = lane & 3;
  gload(0);
  sstore(0);
  __syncthreads();
  int buf = 0;
  for (int p0 = 0; p0 < M; p0 += BP) {
    const bool more = p0 + BP < M;
    if (more) gload(p0 + BP);
    if (do_bias && tid < 256) {  // column sums of the staged dY tile: 4 row groups x 64 columns
      const int c = tid & 63, rg = tid >> 6;
      for (int r = rg; r < BP; r += 4) bacc += bf2f(As[(buf * BP + r) * LDA + c]);
    }
#pragma unroll
    for (int ks = 0; ks < BP / 32; ++ks) {
      const int pr = buf * BP + ks * 32 + 8 * tg + tq;
      bf16x8 af[2], bfr[2];
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const u16* p1 = As + pr * LDA + wr * 32 + a * 16 + 4 * tp;
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p1));
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p1 + 4 * LDA));
        af[a] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
      }
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const u16* p1 = Bs + pr * LDB + wc * 32 + b * 16 + 4 * tp;
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p1));
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p1 + 4 * LDB));
        bfr[b] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
      }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[a], bfr[b], acc[a][b], 0, 0, 0);
    }
    if (more) sstore(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }
  if constexpr (std::is_same<E, float>::value) {
    const float mom = e;
    const float lr = lr_p[0];
    // SGD with momentum (torch semantics, dampening 0): buf = mom * buf + g; p -= lr * buf
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int k = k0 + wc * 32 + b * 16 + (lane & 15);
        if (k >= K) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int n = n0 + wr * 32 + a * 16 + 4 * (lane >> 4) + j;
          if (n >= N) continue;
          const int64_t o = (int64_t)n * K + k;
          const float mb = mom * S0[o] + acc[a][b][j];
          const float p = W[o] - lr * mb;
          S0[o] = mb;
          W[o] = p;
          const u16 pb = f2bf(p);
          W16[o] = pb;
          W16t[(int64_t)k * N + n] = pb;
        }
      }
    if (do_bias) {
      bsum[tid >> 6][tid & 63] = bacc;
      __syncthreads();
      if (tid < 64 && n0 + tid < N) {
        const float g = (bsum[0][tid] + bsum[1][tid]) + (bsum[2][tid] + bsum[3][tid]);
        const float mb = mom * bs0[n0 + tid] + g;
        bs0[n0 + tid] = mb;
        bias[n0 + tid] -= lr * mb;
      }
    }
  } else {
    using U = typename E::Upd;
    U upd = e.upd;
    upd.init(lr_p[0]);
    float* __restrict__ S1 = e.s1;
    float* __restrict__ bs1 = e.bs1;
    float w[2][2][4], s0[2][2][4], s1[2][2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int k = k0 + wc * 32 + b * 16 + (lane & 15);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int n = n0 + wr * 32 + a * 16 + 4 * (lane >> 4) + j;
          const bool in = k < K && n < N;
          const int64_t o = in ? (int64_t)n * K + k : 0;
          w[a][b][j] = in ? W[o] : 0.f;
          s0[a][b][j] = in ? S0[o] : 0.f;
          s1[a][b][j] = in ? S1[o] : 0.f;
        }
      }
    float bw = 0.f, b0 = 0.f, b1 = 0.f;
    const bool bias_lane = do_bias && tid < 64 && n0 + tid < N;
    if (bias_lane) {
      bw = bias[n0 + tid];
      b0 = bs0[n0 + tid];
      b1 = bs1[n0 + tid];
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int k = k0 + wc * 32 + b * 16 + (lane & 15);
        if (k >= K) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int n = n0 + wr * 32 + a * 16 + 4 * (lane >> 4) + j;
          if (n >= N) continue;
          const int64_t o = (int64_t)n * K + k;
          const float p = upd(acc[a][b][j], s0[a][b][j], s1[a][b][j], w[a][b][j]);
          S0[o] = s0[a][b][j];
          S1[o] = s1[a][b][j];
          W[o] = p;
          const u16 pb = f2bf(p);
          W16[o] = pb;
          W16t[(int64_t)k * N + n] = pb;
        }
      }
    if (do_bias) {
      bsum[tid >> 6][tid & 63] = bacc;
      __syncthreads();
      if (bias_lane) {
        const float g = (bsum[0][tid] + bsum[1][tid]) + (bsum[2][tid] + bsum[3][tid]);
        bias[n0 + tid] = upd(g, b0, b1, bw);
        bs0[n0 + tid] = b0;
        bs1[n0 + tid] = b1;
      }
    }
  }
}

// ------------------------------------------------------------------ softmax cross-entropy, few classes
// logits [M][ld] bf16 (first C columns real); dlogits = (softmax - onehot) / M (pad columns 0);
// stats[0] += sum of losses / M, stats[1] += number of correct argmax predictions. step_t (may be
// null): the device step counter, advanced by one per launch; nothing else reads or writes it here.
__global__ __launch_bounds__(256) void xent_small_k(const u16* __restrict__ logits, const int64_t* __restrict__ y,
                                                    const int64_t* __restrict__ idx, u16* __restrict__ dl, int M,
                                                    int C, int ld, float* __restrict__ stats,
                                                    int* __restrict__ step_t) {
  __shared__ float red[2][4];
  const int r = blockIdx.x * 256 + threadIdx.x;
  float loss = 0.f, correct = 0.f;
  if (r < M) {
    const u16* L = logits + (int64_t)r * ld;
    const int64_t t = y[idx ? idx[r] : r];
    float mx = -INFINITY;
    int arg = 0;
    for (int c = 0; c < C; ++c) {
      const float v = bf2f(L[c]);
      if (v > mx) {
        mx = v;
        arg = c;
      }
    }
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += __expf(bf2f(L[c]) - mx);
    const float lse = mx + __logf(s);
    loss = (t >= 0 && t < C) ? (lse - bf2f(L[t])) / M : 0.f;
    correct = (arg == t) ? 1.f : 0.f;
    for (int c = 0; c < ld; ++c)
      dl[(int64_t)r * ld + c] = f2bf(c < C ? (__expf(bf2f(L[c]) - lse) - (c == t ? 1.f : 0.f)) / M : 0.f);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    loss += __shfl_xor(loss, o, 64);
    correct += __shfl_xor(correct, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = loss;
    red[1][threadIdx.x >> 6] = correct;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicAdd(stats, (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]));
    atomicAdd(stats + 1, (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]));
    if (step_t != nullptr && blockIdx.x == 0) step_t[0] += 1;
  }
}

}  // namespace

hipError_t lin_fwd(const bf16* x, const int64_t* idx, const bf16* w, const float* bias, const bf16* mask, bf16* y,
                   int M, int N, int K, int relu, hipStream_t st) {
  const int grid = ((M + BM - 1) / BM) * ((N + BN - 1) / BN);
  hipLaunchKernelGGL(gemm_nt_k, dim3(grid), dim3(256), 0, st, reinterpret_cast<const u16*>(x), idx,
                     reinterpret_cast<const u16*>(w), bias, reinterpret_cast<const u16*>(mask),
                     reinterpret_cast<u16*>(y), M, N, K, relu);
  return hipGetLastError();
}

hipError_t lin_fwd_splitk(const bf16* x, const bf16* w, const float* bias, float* part, bf16* y, int M, int N, int K,
                          int relu, hipStream_t st) {
  const int slabs = splitk_slabs(K);
  const int grid = ((M + BM - 1) / BM) * ((N + BN - 1) / BN) * slabs;
  hipLaunchKernelGGL(gemm_nt_slab_k, dim3(grid), dim3(256), 0, st, reinterpret_cast<const u16*>(x),
                     reinterpret_cast<const u16*>(w), part, M, N, K);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(splitk_reduce_k, dim3((M * N / 4 + 255) / 256), dim3(256), 0, st, part, slabs, bias,
                     reinterpret_cast<u16*>(y), M * N, N, relu);
  return hipGetLastError();
}

hipError_t lin_wgrad_sgd(const bf16* dy, const bf16* x, const int64_t* idx, int M, int N, int K, float* w, float* wm,
                         bf16* w16, bf16* w16t, float* bias, float* bm, const float* lr, float momentum,
                         hipStream_t st) {
  const int grid = ((N + BN - 1) / BN) * ((K + BK - 1) / BK);
  hipLaunchKernelGGL(wgrad_k<float>, dim3(grid), dim3(256), 0, st, reinterpret_cast<const u16*>(dy),
                     reinterpret_cast<const u16*>(x), idx, M, N, K, w, wm, reinterpret_cast<u16*>(w16),
                     reinterpret_cast<u16*>(w16t), bias, bm, lr, momentum);
  return hipGetLastError();
}

template <class U>
static hipError_t launch_wgrad_opt(const bf16* dy, const bf16* x, const int64_t* idx, int M, int N, int K, float* w,
                                   float* s0, float* s1, bf16* w16, bf16* w16t, float* bias, float* bs0, float* bs1,
                                   const float* lr, U upd, hipStream_t st) {
  const int grid = ((N + BN - 1) / BN) * ((K + BK - 1) / BK);
  hipLaunchKernelGGL(wgrad_k<Opt2<U>>, dim3(grid), dim3(256), 0, st, reinterpret_cast<const u16*>(dy),
                     reinterpret_cast<const u16*>(x), idx, M, N, K, w, s0, reinterpret_cast<u16*>(w16),
                     reinterpret_cast<u16*>(w16t), bias, bs0, lr, Opt2<U>{upd, s1, bs1});
  return hipGetLastError();
}

hipError_t lin_wgrad_adam(const bf16* dy, const bf16* x, const int64_t* idx, int M, int N, int K, float* w, float* m,
                          float* v, bf16* w16, bf16* w16t, float* bias, float* bm, float* bv, const float* lr,
                          const int* step_t, float beta1, float beta2, float eps, hipStream_t st) {
  return launch_wgrad_opt(dy, x, idx, M, N, K, w, m, v, w16, w16t, bias, bm, bv, lr,
                          AdamUpd{beta1, beta2, eps, step_t, 0.f, 0.f}, st);
}

hipError_t lin_wgrad_ftrl(const bf16* dy, const bf16* x, const int64_t* idx, int M, int N, int K, float* w, float* z,
                          float* n, bf16* w16, bf16* w16t, float* bias, float* bz, float* bn, const float* lr,
                          float l1, float beta, float wd, hipStream_t st) {
  return launch_wgrad_opt(dy, x, idx, M, N, K, w, z, n, w16, w16t, bias, bz, bn, lr, FtrlUpd{l1, beta, wd, 0.f}, st);
}

hipError_t xent_small(const bf16* logits, const int64_t* y, const int64_t* idx, bf16* dl, int M, int C, int ld,
                      float* stats, int* step_t, hipStream_t st) {
  hipLaunchKernelGGL(xent_small_k, dim3((M + 255) / 256), dim3(256), 0, st, reinterpret_cast<const u16*>(logits), y,
                     idx, reinterpret_cast<u16*>(dl), M, C, ld, stats, step_t);
  return hipGetLastError();
}

}  // namespace mlp
}  // namespace katib_hip
