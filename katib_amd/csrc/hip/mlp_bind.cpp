// torch bindings of the fused MLP kernels (mlp.hip), with the shape / dtype / alignment /
// index-range checks the kernels and their grids rely on.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include "mlp.h"

namespace py = pybind11;
using at::Tensor;
namespace M_ = katib_hip::mlp;

namespace {

hipStream_t stream() { return c10::hip::getCurrentHIPStream().stream(); }
M_::bf16* bp(const Tensor& t) { return reinterpret_cast<M_::bf16*>(t.data_ptr()); }
void ok(hipError_t e, const char* w) { TORCH_CHECK(e == hipSuccess, w, ": ", hipGetErrorString(e)); }

void chk(const Tensor& t, at::ScalarType dt, int64_t n, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == dt && t.is_contiguous() && t.numel() == n, name,
              " must be a contiguous ", c10::toString(dt), " GPU tensor of ", n, " elements (got ", t.numel(), ")");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name, " must be 16-byte aligned");
}
// the gather index must address rows of x: the kernels trust it
void chk_idx(const c10::optional<Tensor>& idx, int64_t M) {
  if (!idx.has_value()) return;
  TORCH_CHECK(idx->is_cuda() && idx->scalar_type() == at::kLong && idx->is_contiguous() && idx->numel() == M,
              "idx must be a contiguous int64 GPU tensor with one entry per row");
}

void lin_fwd(const Tensor& x, const c10::optional<Tensor>& idx, const Tensor& w, const c10::optional<Tensor>& bias,
             const c10::optional<Tensor>& mask, const Tensor& y, bool relu) {
  TORCH_CHECK(w.dim() == 2 && y.dim() == 2 && x.dim() == 2, "lin_fwd: 2-D operands");
  const int64_t N = w.size(0), K = w.size(1), M = y.size(0);
  TORCH_CHECK(K % 8 == 0 && K == x.size(1) && y.size(1) == N, "lin_fwd: K % 8 == 0 and matching shapes");
  TORCH_CHECK(idx.has_value() || x.size(0) == M, "lin_fwd: x rows must match y rows without a gather");
  chk(x, at::kBFloat16, x.numel(), "x");
  chk(w, at::kBFloat16, N * K, "w");
  chk(y, at::kBFloat16, M * N, "y");
  chk_idx(idx, M);
  if (bias.has_value()) chk(*bias, at::kFloat, N, "bias");
  if (mask.has_value()) chk(*mask, at::kBFloat16, M * N, "mask");
  ok(M_::lin_fwd(bp(x), idx.has_value() ? idx->data_ptr<int64_t>() : nullptr, bp(w),
                 bias.has_value() ? bias->data_ptr<float>() : nullptr, mask.has_value() ? bp(*mask) : nullptr, bp(y),
                 (int)M, (int)N, (int)K, relu ? 1 : 0, stream()),
     "lin_fwd");
}

int64_t splitk_part_size(int64_t M, int64_t N, int64_t K) { return (int64_t)M_::splitk_slabs((int)K) * M * N; }

void lin_fwd_splitk(const Tensor& x, const Tensor& w, const c10::optional<Tensor>& bias, const Tensor& part,
                    const Tensor& y, bool relu) {
  TORCH_CHECK(w.dim() == 2 && y.dim() == 2 && x.dim() == 2, "lin_fwd_splitk: 2-D operands");
  const int64_t N = w.size(0), K = w.size(1), M = y.size(0);
  TORCH_CHECK(M > 0 && K > 0 && K % 8 == 0 && N % 8 == 0 && K == x.size(1) && y.size(1) == N && x.size(0) == M,
              "lin_fwd_splitk: N, K % 8 == 0 and matching shapes");
  TORCH_CHECK(M * N < (1 << 28) && K < (1 << 28), "lin_fwd_splitk: operands too large");
  chk(x, at::kBFloat16, M * K, "x");
  chk(w, at::kBFloat16, N * K, "w");
  chk(y, at::kBFloat16, M * N, "y");
  chk(part, at::kFloat, splitk_part_size(M, N, K), "part");
  if (bias.has_value()) chk(*bias, at::kFloat, N, "bias");
  ok(M_::lin_fwd_splitk(bp(x), bp(w), bias.has_value() ? bias->data_ptr<float>() : nullptr, part.data_ptr<float>(),
                        bp(y), (int)M, (int)N, (int)K, relu ? 1 : 0, stream()),
     "lin_fwd_splitk");
}

void lin_wgrad_sgd(const Tensor& dy, const Tensor& x, const c10::optional<Tensor>& idx, const Tensor& w,
                   const Tensor& wm, const Tensor& w16, const Tensor& w16t, const c10::optional<Tensor>& bias,
                   const c10::optional<Tensor>& bm, const Tensor& lr, double momentum) {
  TORCH_CHECK(dy.dim() == 2 && x.dim() == 2 && w.dim() == 2, "lin_wgrad_sgd: 2-D operands");
  const int64_t M = dy.size(0), N = dy.size(1), K = w.size(1);
  TORCH_CHECK(w.size(0) == N && x.size(1) == K && N % 8 == 0 && K % 8 == 0, "lin_wgrad_sgd: N, K % 8 == 0");
  TORCH_CHECK(idx.has_value() || x.size(0) == M, "lin_wgrad_sgd: x rows must match dy rows without a gather");
  chk(dy, at::kBFloat16, M * N, "dy");
  chk(x, at::kBFloat16, x.numel(), "x");
  chk_idx(idx, M);
  chk(w, at::kFloat, N * K, "w");
  chk(wm, at::kFloat, N * K, "wm");
  chk(w16, at::kBFloat16, N * K, "w16");
  chk(w16t, at::kBFloat16, N * K, "w16t");
  TORCH_CHECK(bias.has_value() == bm.has_value(), "bias and its momentum buffer go together");
  if (bias.has_value()) {
    chk(*bias, at::kFloat, N, "bias");
    chk(*bm, at::kFloat, N, "bias momentum");
  }
  TORCH_CHECK(lr.is_cuda() && lr.scalar_type() == at::kFloat && lr.numel() == 1, "lr must be a GPU fp32 scalar");
  ok(M_::lin_wgrad_sgd(bp(dy), bp(x), idx.has_value() ? idx->data_ptr<int64_t>() : nullptr, (int)M, (int)N, (int)K,
                       w.data_ptr<float>(), wm.data_ptr<float>(), bp(w16), bp(w16t),
                       bias.has_value() ? bias->data_ptr<float>() : nullptr,
                       bm.has_value() ? bm->data_ptr<float>() : nullptr, lr.data_ptr<float>(), (float)momentum,
                       stream()),
     "lin_wgrad_sgd");
}

// the operands every fused weight-gradient kernel shares; returns (M, N, K)
struct WgShape {
  int64_t M, N, K;
};
WgShape chk_wgrad(const char* who, const Tensor& dy, const Tensor& x, const c10::optional<Tensor>& idx, const Tensor& w,
                  const Tensor& w16, const Tensor& w16t, const Tensor& lr) {
  TORCH_CHECK(dy.dim() == 2 && x.dim() == 2 && w.dim() == 2, who, ": 2-D operands");
  const int64_t M = dy.size(0), N = dy.size(1), K = w.size(1);
  TORCH_CHECK(w.size(0) == N && x.size(1) == K && N % 8 == 0 && K % 8 == 0, who, ": N, K % 8 == 0");
  TORCH_CHECK(idx.has_value() || x.size(0) == M, who, ": x rows must match dy rows without a gather");
  chk(dy, at::kBFloat16, M * N, "dy");
  chk(x, at::kBFloat16, x.numel(), "x");
  chk_idx(idx, M);
  chk(w, at::kFloat, N * K, "w");
  chk(w16, at::kBFloat16, N * K, "w16");
  chk(w16t, at::kBFloat16, N * K, "w16t");
  TORCH_CHECK(lr.is_cuda() && lr.scalar_type() == at::kFloat && lr.numel() == 1, "lr must be a GPU fp32 scalar");
  return {M, N, K};
}
// bias and its two state vectors: together or not at all
bool chk_bias2(const c10::optional<Tensor>& bias, const c10::optional<Tensor>& s0, const c10::optional<Tensor>& s1,
               int64_t N, const char* n0, const char* n1) {
  TORCH_CHECK(bias.has_value() == s0.has_value() && bias.has_value() == s1.has_value(),
              "bias and its two state vectors go together");
  if (!bias.has_value()) return false;
  chk(*bias, at::kFloat, N, "bias");
  chk(*s0, at::kFloat, N, n0);
  chk(*s1, at::kFloat, N, n1);
  return true;
}
const int64_t* idx_p(const c10::optional<Tensor>& idx) { return idx.has_value() ? idx->data_ptr<int64_t>() : nullptr; }
void chk_step_t(const Tensor& step_t) {
  TORCH_CHECK(step_t.is_cuda() && step_t.scalar_type() == at::kInt && step_t.numel() == 1,
              "step_t must be a GPU int32 tensor of one element");
}

void lin_wgrad_adam(const Tensor& dy, const Tensor& x, const c10::optional<Tensor>& idx, const Tensor& w,
                    const Tensor& m, const Tensor& v, const Tensor& w16, const Tensor& w16t,
                    const c10::optional<Tensor>& bias, const c10::optional<Tensor>& bm,
                    const c10::optional<Tensor>& bv, const Tensor& lr, const Tensor& step_t, double beta1,
                    double beta2, double eps) {
  const WgShape s = chk_wgrad("lin_wgrad_adam", dy, x, idx, w, w16, w16t, lr);
  chk(m, at::kFloat, s.N * s.K, "m");
  chk(v, at::kFloat, s.N * s.K, "v");
  const bool hb = chk_bias2(bias, bm, bv, s.N, "bm", "bv");
  chk_step_t(step_t);
  ok(M_::lin_wgrad_adam(bp(dy), bp(x), idx_p(idx), (int)s.M, (int)s.N, (int)s.K, w.data_ptr<float>(),
                        m.data_ptr<float>(), v.data_ptr<float>(), bp(w16), bp(w16t),
                        hb ? bias->data_ptr<float>() : nullptr, hb ? bm->data_ptr<float>() : nullptr,
                        hb ? bv->data_ptr<float>() : nullptr, lr.data_ptr<float>(), step_t.data_ptr<int>(),
                        (float)beta1, (float)beta2, (float)eps, stream()),
     "lin_wgrad_adam");
}

void lin_wgrad_ftrl(const Tensor& dy, const Tensor& x, const c10::optional<Tensor>& idx, const Tensor& w,
                    const Tensor& z, const Tensor& n, const Tensor& w16, const Tensor& w16t,
                    const c10::optional<Tensor>& bias, const c10::optional<Tensor>& bz,
                    const c10::optional<Tensor>& bn, const Tensor& lr, double l1, double beta, double wd) {
  const WgShape s = chk_wgrad("lin_wgrad_ftrl", dy, x, idx, w, w16, w16t, lr);
  chk(z, at::kFloat, s.N * s.K, "z");
  chk(n, at::kFloat, s.N * s.K, "n");
  const bool hb = chk_bias2(bias, bz, bn, s.N, "bz", "bn");
  ok(M_::lin_wgrad_ftrl(bp(dy), bp(x), idx_p(idx), (int)s.M, (int)s.N, (int)s.K, w.data_ptr<float>(),
                        z.data_ptr<float>(), n.data_ptr<float>(), bp(w16), bp(w16t),
                        hb ? bias->data_ptr<float>() : nullptr, hb ? bz->data_ptr<float>() : nullptr,
                        hb ? bn->data_ptr<float>() : nullptr, lr.data_ptr<float>(), (float)l1, (float)beta, (float)wd,
                        stream()),
     "lin_wgrad_ftrl");
}

void xent_small(const Tensor& logits, const Tensor& y, const c10::optional<Tensor>& idx, const Tensor& dl,
                int64_t C, const Tensor& stats, const c10::optional<Tensor>& step_t) {
  TORCH_CHECK(logits.dim() == 2, "logits must be [M, ld]");
  const int64_t M = logits.size(0), ld = logits.size(1);
  TORCH_CHECK(C > 0 && C <= ld && ld <= 64, "xent_small: 0 < C <= ld <= 64");
  chk(logits, at::kBFloat16, M * ld, "logits");
  chk(dl, at::kBFloat16, M * ld, "dl");
  TORCH_CHECK(y.is_cuda() && y.scalar_type() == at::kLong && y.is_contiguous(), "labels must be int64 on the GPU");
  chk_idx(idx, M);
  TORCH_CHECK(idx.has_value() || y.numel() == M, "labels must have one entry per row without a gather");
  TORCH_CHECK(stats.is_cuda() && stats.scalar_type() == at::kFloat && stats.numel() == 2, "stats: fp32[2]");
  if (step_t.has_value()) chk_step_t(*step_t);
  ok(M_::xent_small(bp(logits), y.data_ptr<int64_t>(), idx.has_value() ? idx->data_ptr<int64_t>() : nullptr, bp(dl),
                    (int)M, (int)C, (int)ld, stats.data_ptr<float>(),
                    step_t.has_value() ? step_t->data_ptr<int>() : nullptr, stream()),
     "xent_small");
}

}  // namespace

void register_mlp(py::module& m) {
  m.def("lin_fwd", &lin_fwd, "fused linear (+bias, +ReLU or ReLU-derivative mask), optional row gather");
  m.def("lin_fwd_splitk", &lin_fwd_splitk,
        "fused linear (+bias, +ReLU) for K >> M: slabs of LIN_SPLITK_KS columns into fp32 partials, summed in order");
  m.def("lin_splitk_part_size", &splitk_part_size, "fp32 elements of lin_fwd_splitk's partial buffer for (M, N, K)");
  m.attr("LIN_SPLITK_KS") = M_::SPLITK_KS;
  m.def("lin_wgrad_sgd", &lin_wgrad_sgd, "weight/bias gradient with fused SGD-momentum update");
  m.def("lin_wgrad_adam", &lin_wgrad_adam, "weight/bias gradient with fused Adam update (t = step_t[0], 1-based)");
  m.def("lin_wgrad_ftrl", &lin_wgrad_ftrl, "weight/bias gradient with fused FTRL-proximal update");
  m.def("xent_small", &xent_small,
        "softmax cross-entropy + gradient for a few classes; advances the int32 device counter step_t when given",
        py::arg("logits"), py::arg("y"), py::arg("idx"), py::arg("dl"), py::arg("C"), py::arg("stats"),
        py::arg("step_t") = py::none());
}
