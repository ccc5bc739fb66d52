// Separable convolution of the ENAS child in one kernel per direction (enas_sepconv.hip): depthwise
// (fp32 VALU) feeding the pointwise 1x1 (bf16 MFMA) through LDS, so the depthwise result never reaches
// HBM. NHWC bf16 activations, fp32 tap-major depthwise weights, bf16 pointwise weights.
#pragma once
#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

namespace katib_hip {
namespace sepconv {

struct Geom {
  int N, H, W, C;  // input, C % 8 == 0
  int DM;          // depth multiplier: depthwise channel o reads input channel o / DM (1 or 2)
  int K;           // square depthwise kernel: 3, 5 or 7
  int S;           // stride 1 or 2
  int pt, pl;      // top / left padding (TF 'same': the odd pixel goes bottom / right)
  int OH, OW;
  int F;           // pointwise filters, F % 16 == 0, F <= 128
};

// How the kernels cut the map: a band is `rows` whole output rows of one image (at most 128 pixels),
// `bands` of them per image; the staged input patch of a band is PH x PW pixels.
struct Plan {
  bool ok;  // false: the map is wider than 128 output columns or one band does not fit the LDS
  int rows, bands, PH, PW;
  int region0_fwd, region0_bwd;  // bytes of the patch region (shared with the output tiles)
  int lds_fwd, lds_bwd;
  int groups;  // backward: workgroups per channel chunk, each with a contiguous set of bands
};

constexpr int kLdsLimit = 160 * 1024;  // gfx950 LDS per workgroup

Plan plan(const Geom& g);

// y[n,oy,ox,f] = bf16(bias[f] + sum_cd bf16(d[n,oy,ox,cd]) * wp[f][cd]),
// d = sum_taps x[n, oy*S - pt + ky, ox*S - pl + kx, cd / DM] * wd[ky*K + kx][cd] in fp32, taps in (ky, kx) order
hipError_t launch_fwd(const Geom& g, const Plan& p, const __hip_bfloat16* x, const float* wd, const __hip_bfloat16* wp,
                      const float* bias, __hip_bfloat16* y, hipStream_t st);
// gd[n,oy,ox,cd] = bf16(sum_f gy[n,oy,ox,f] * wt[cd][f]);  gwp[f][cd] += sum_pixels gy * bf16(d) (fp32
// atomics into the caller-zeroed accumulator); d is recomputed from x with the forward's device function
hipError_t launch_bwd_pw(const Geom& g, const Plan& p, const __hip_bfloat16* x, const float* wd,
                         const __hip_bfloat16* wt, const __hip_bfloat16* gy, __hip_bfloat16* gd, float* gwp,
                         hipStream_t st);

}  // namespace sepconv
}  // namespace katib_hip
