// torch bindings of the fused separable convolution (enas_sepconv.hip). Every tensor is checked against
// the geometry before the launch: the kernels' loads and stores are 16-byte vectors at 32-bit offsets,
// and these checks keep them inside the tensors.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include "enas_sepconv.h"

namespace py = pybind11;
using at::Tensor;
namespace SC = katib_hip::sepconv;

namespace {

SC::Geom make_geom(const std::vector<int64_t>& v) {
  TORCH_CHECK(v.size() == 12, "geometry: N,H,W,C,DM,K,S,pt,pl,OH,OW,F");
  SC::Geom g{};
  int* f[12] = {&g.N, &g.H, &g.W, &g.C, &g.DM, &g.K, &g.S, &g.pt, &g.pl, &g.OH, &g.OW, &g.F};
  for (int i = 0; i < 12; ++i) {
    TORCH_CHECK(v[i] >= 0 && v[i] < (1 << 30), "geometry value out of range");
    *f[i] = (int)v[i];
  }
  TORCH_CHECK(g.N > 0 && g.H > 0 && g.W > 0 && g.C > 0, "empty geometry");
  TORCH_CHECK(g.C % 8 == 0, "separable conv: C must be a multiple of 8");
  TORCH_CHECK(g.DM == 1 || g.DM == 2, "depth multiplier must be 1 or 2");
  TORCH_CHECK(g.K == 3 || g.K == 5 || g.K == 7, "kernel size must be 3, 5 or 7");
  TORCH_CHECK(g.S == 1 || g.S == 2, "stride must be 1 or 2");
  TORCH_CHECK(g.F % 16 == 0 && g.F >= 16 && g.F <= 128, "filters must be a multiple of 16, at most 128");
  // TF 'same': the kernels rely on exactly this output size and padding
  const int OH = (g.H + g.S - 1) / g.S, OW = (g.W + g.S - 1) / g.S;
  TORCH_CHECK(g.OH == OH && g.OW == OW, "output size is not ceil(size / stride)");
  TORCH_CHECK(g.pt == std::max((OH - 1) * g.S + g.K - g.H, 0) / 2 && g.pl == std::max((OW - 1) * g.S + g.K - g.W, 0) / 2,
              "padding is not TF 'same'");
  TORCH_CHECK((int64_t)g.N * g.H * g.W * std::max(g.C * g.DM, g.F) < (1ll << 31), "N*H*W*max(Cd, F) >= 2^31");
  return g;
}

void check(const Tensor& t, at::ScalarType ty, int64_t numel, const char* name, const Tensor& on) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == ty && t.is_contiguous() && t.device() == on.device(), name,
              " must be a contiguous ", ty == at::kBFloat16 ? "bf16" : "fp32", " tensor on the input's GPU");
  TORCH_CHECK(t.numel() == numel, name, " has ", t.numel(), " elements, geometry needs ", numel);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name, " must be 16-byte aligned");
}

hipStream_t stream() { return c10::hip::getCurrentHIPStream().stream(); }
const __hip_bfloat16* bf(const Tensor& t) { return reinterpret_cast<const __hip_bfloat16*>(t.data_ptr()); }

SC::Plan plan_or_throw(const SC::Geom& g) {
  const SC::Plan p = SC::plan(g);
  TORCH_CHECK(p.ok, "separable conv: a band of this map does not fit the kernels (OW <= 128, one output row's "
                    "patch within the LDS)");
  return p;
}

// x [N,H,W,C] bf16, wd [K*K][Cd] fp32, wp [F][Cd] bf16, bias [F] fp32 or None -> y [N,OH,OW,F] bf16
void sep_fwd(const Tensor& x, const Tensor& wd, const Tensor& wp, const c10::optional<Tensor>& bias, const Tensor& y,
             const std::vector<int64_t>& geom) {
  const SC::Geom g = make_geom(geom);
  const SC::Plan p = plan_or_throw(g);
  const int64_t Cd = (int64_t)g.C * g.DM;
  check(x, at::kBFloat16, (int64_t)g.N * g.H * g.W * g.C, "x", x);
  check(wd, at::kFloat, g.K * g.K * Cd, "wd", x);
  check(wp, at::kBFloat16, g.F * Cd, "wp", x);
  check(y, at::kBFloat16, (int64_t)g.N * g.OH * g.OW * g.F, "y", x);
  const float* b = nullptr;
  if (bias.has_value() && bias->defined()) {
    check(*bias, at::kFloat, g.F, "bias", x);
    b = bias->data_ptr<float>();
  }
  TORCH_CHECK(SC::launch_fwd(g, p, bf(x), wd.data_ptr<float>(), bf(wp), b,
                             reinterpret_cast<__hip_bfloat16*>(y.data_ptr()), stream()) == hipSuccess,
              "sep_fwd launch failed");
}

// wt [Cd][F] bf16, gy [N,OH,OW,F] bf16 -> gd [N,OH,OW,Cd] bf16; gwp [F][Cd] fp32 is added into
void sep_bwd_pw(const Tensor& x, const Tensor& wd, const Tensor& wt, const Tensor& gy, const Tensor& gd,
                const Tensor& gwp, const std::vector<int64_t>& geom) {
  const SC::Geom g = make_geom(geom);
  const SC::Plan p = plan_or_throw(g);
  const int64_t Cd = (int64_t)g.C * g.DM, P = (int64_t)g.N * g.OH * g.OW;
  check(x, at::kBFloat16, (int64_t)g.N * g.H * g.W * g.C, "x", x);
  check(wd, at::kFloat, g.K * g.K * Cd, "wd", x);
  check(wt, at::kBFloat16, g.F * Cd, "wt", x);
  check(gy, at::kBFloat16, P * g.F, "gy", x);
  check(gd, at::kBFloat16, P * Cd, "gd", x);
  check(gwp, at::kFloat, g.F * Cd, "gwp", x);
  TORCH_CHECK(SC::launch_bwd_pw(g, p, bf(x), wd.data_ptr<float>(), bf(wt), bf(gy),
                                reinterpret_cast<__hip_bfloat16*>(gd.data_ptr()), gwp.data_ptr<float>(),
                                stream()) == hipSuccess,
              "sep_bwd_pw launch failed");
}

// (rows per band, bands per image, LDS bytes forward, backward, backward workgroups per chunk) or None
py::object sep_plan(const std::vector<int64_t>& geom) {
  const SC::Plan p = SC::plan(make_geom(geom));
  if (!p.ok) return py::none();
  return py::make_tuple(p.rows, p.bands, p.lds_fwd, p.lds_bwd, p.groups);
}

}  // namespace

void register_sepconv(py::module& m) {
  m.def("sep_fwd", &sep_fwd, "separable conv forward: depthwise + pointwise + bias in one launch (NHWC bf16)");
  m.def("sep_bwd_pw", &sep_bwd_pw, "its pointwise backward: recomputed depthwise, gd and the pointwise weight gradient");
  m.def("sep_plan", &sep_plan, "how the kernels cut the map, None where they do not serve it");
}
