// Element updates of the fused optimizers, shared by the weight-gradient epilogues of mlp.hip and
// mnist_tfcnn.hip (device code only; include from a .hip file).
#pragma once
#include <hip/hip_runtime.h>

namespace katib_hip {
namespace mlp {

// Element update of a two-state optimizer: operator() takes the gradient, the element's two state
// values (updated in place) and its weight, and returns the new weight. It leaves an element with
// g = 0 and zero state exactly as it was (the padded output rows, dead ReLU units).
//
// torch.optim.Adam, default flags: s0 = exp_avg, s1 = exp_avg_sq. step = lr / (1 - beta1^t) and
// sbc2 = sqrt(1 - beta2^t) are the same for every element; init() computes them once per thread.
struct AdamUpd {
  float b1, b2, eps;
  const int* step_t;
  float step, sbc2;
  // beta^t by binary exponentiation: exact at t = 1, where 1 - beta2^t = 1e-3 magnifies an error of
  // beta2^t a thousandfold, and within t * 2^-24 relative anywhere
  static __device__ __forceinline__ float ipow(float b, int t) {
    float r = 1.f;
    for (; t > 0; t >>= 1, b *= b)
      if (t & 1) r *= b;
    return r;
  }
  __device__ __forceinline__ void init(float lr) {
    const int t = max(step_t[0], 1);  // 1-based; a counter nobody advanced must not divide by 0
    step = lr / (1.f - ipow(b1, t));
    sbc2 = sqrtf(1.f - ipow(b2, t));
  }
  __device__ __forceinline__ float operator()(float g, float& m, float& v, float w) const {
    m = b1 * m + (1.f - b1) * g;
    v = b2 * v + (1.f - b2) * (g * g);
    return w - step * (m / (sqrtf(v) / sbc2 + eps));  // zero state, g = 0: 0 / eps = 0
  }
};

}  // namespace mlp
}  // namespace katib_hip
