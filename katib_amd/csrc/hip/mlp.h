// Fused MLP training kernels (mlp.hip): bf16 activations/weight shadows, fp32 masters.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>

namespace katib_hip {
namespace mlp {

typedef __hip_bfloat16 bf16;

// y[M][N] = epi(x[idx?][K] . w[N][K]^T); epi = + bias (may be null), ReLU if relu, * [mask > 0] if mask.
hipError_t lin_fwd(const bf16* x, const int64_t* idx, const bf16* w, const float* bias, const bf16* mask, bf16* y,
                   int M, int N, int K, int relu, hipStream_t st);
// The same product for K much larger than M, without gather and mask: slabs of SPLITK_KS columns of K, one
// per workgroup and 64 x 64 tile, into fp32 partials part [splitk_slabs(K)][M][N]; a second launch sums them
// in slab order, then bias, ReLU and the bf16 rounding. SPLITK_KS does not depend on M, so a row's result
// does not depend on the batch it sits in. N % 8 == 0, K % 8 == 0.
constexpr int SPLITK_KS = 512;
inline int splitk_slabs(int K) { return (K + SPLITK_KS - 1) / SPLITK_KS; }
hipError_t lin_fwd_splitk(const bf16* x, const bf16* w, const float* bias, float* part, bf16* y, int M, int N, int K,
                          int relu, hipStream_t st);
// dW = dy^T x (x rows through idx when given) and SGD with momentum on w (fp32 [N][K]), its momentum
// buffer, bf16 shadows w16 [N][K] / w16t [K][N]; bias (+ its buffer) updated from the column sums of dy.
hipError_t lin_wgrad_sgd(const bf16* dy, const bf16* x, const int64_t* idx, int M, int N, int K, float* w, float* wm,
                         bf16* w16, bf16* w16t, float* bias, float* bm, const float* lr, float momentum,
                         hipStream_t st);
// The same reduction with torch.optim.Adam (default flags) in the epilogue: m / v [N][K] fp32, bm / bv [N];
// t = step_t[0] is the 1-based number of the running step (device int32, advanced by xent_small).
hipError_t lin_wgrad_adam(const bf16* dy, const bf16* x, const int64_t* idx, int M, int N, int K, float* w, float* m,
                          float* v, bf16* w16, bf16* w16t, float* bias, float* bm, float* bv, const float* lr,
                          const int* step_t, float beta1, float beta2, float eps, hipStream_t st);
// ... and with FTRL-proximal (workloads/mnist_mlp.py Ftrl): z / n [N][K] fp32, bz / bn [N].
hipError_t lin_wgrad_ftrl(const bf16* dy, const bf16* x, const int64_t* idx, int M, int N, int K, float* w, float* z,
                          float* n, bf16* w16, bf16* w16t, float* bias, float* bz, float* bn, const float* lr,
                          float l1, float beta, float wd, hipStream_t st);
// softmax cross-entropy over the first C of ld columns; dl = (softmax - onehot) / M; stats += (mean loss, correct).
// step_t (may be null): device int32 step counter, incremented once per launch.
hipError_t xent_small(const bf16* logits, const int64_t* y, const int64_t* idx, bf16* dl, int M, int C, int ld,
                      float* stats, int* step_t, hipStream_t st);

}  // namespace mlp
}  // namespace katib_hip
