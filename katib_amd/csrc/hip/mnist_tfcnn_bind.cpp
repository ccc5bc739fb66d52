// torch bindings of the Keras MNIST CNN convolution kernels (mnist_tfcnn.hip), with the shape / dtype /
// alignment checks the kernels and their grids rely on. The geometry is fixed; B comes from z / dz.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include "mnist_tfcnn.h"

namespace py = pybind11;
using at::Tensor;
namespace T_ = katib_hip::tfcnn;

namespace {

hipStream_t stream() { return c10::hip::getCurrentHIPStream().stream(); }
T_::u16* bp(const Tensor& t) { return reinterpret_cast<T_::u16*>(t.data_ptr()); }
void ok(hipError_t e, const char* w) { TORCH_CHECK(e == hipSuccess, w, ": ", hipGetErrorString(e)); }

void chk(const Tensor& t, at::ScalarType dt, int64_t n, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == dt && t.is_contiguous() && t.numel() == n, name,
              " must be a contiguous ", c10::toString(dt), " GPU tensor of ", n, " elements (got ", t.numel(), ")");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name, " must be 16-byte aligned");
}
// the images: [rows][784] bf16; the gather index must address its rows, the kernels trust it
void chk_x(const Tensor& x, const c10::optional<Tensor>& idx, int64_t B) {
  TORCH_CHECK(x.dim() == 2 && x.size(1) == T_::IMG, "x must be [rows][784]");
  chk(x, at::kBFloat16, x.numel(), "x");
  if (idx.has_value()) {
    TORCH_CHECK(idx->is_cuda() && idx->scalar_type() == at::kLong && idx->is_contiguous() && idx->numel() == B,
                "idx must be a contiguous int64 GPU tensor with one entry per image");
  } else {
    TORCH_CHECK(x.size(0) == B, "x rows must match the batch without a gather");
  }
}
const int64_t* idx_p(const c10::optional<Tensor>& idx) { return idx.has_value() ? idx->data_ptr<int64_t>() : nullptr; }
int64_t batch(const Tensor& t, const char* name) {
  TORCH_CHECK(t.numel() > 0 && t.numel() % T_::F == 0, name, " must hold a whole number of images");
  const int64_t B = t.numel() / T_::F;
  TORCH_CHECK(B < (1 << 20), "batch too large");
  return B;
}
void chk_lr(const Tensor& lr) {
  TORCH_CHECK(lr.is_cuda() && lr.scalar_type() == at::kFloat && lr.numel() == 1, "lr must be a GPU fp32 scalar");
}

void tfcnn_conv_fwd(const Tensor& x, const c10::optional<Tensor>& idx, const Tensor& ws, const Tensor& b,
                    const Tensor& z) {
  const int64_t B = batch(z, "z");
  chk_x(x, idx, B);
  chk(ws, at::kBFloat16, 9 * T_::C, "ws");
  chk(b, at::kFloat, T_::C, "b");
  chk(z, at::kBFloat16, B * T_::F, "z");
  ok(T_::conv_fwd(bp(x), idx_p(idx), bp(ws), b.data_ptr<float>(), bp(z), (int)B, stream()), "tfcnn_conv_fwd");
}

// the operands both weight-gradient bindings share; returns B
int64_t chk_wgrad(const Tensor& dz, const Tensor& x, const c10::optional<Tensor>& idx, const Tensor& part,
                  const Tensor& w, const Tensor& b, const Tensor& ws, const Tensor& lr) {
  const int64_t B = batch(dz, "dz");
  chk(dz, at::kBFloat16, B * T_::F, "dz");
  chk_x(x, idx, B);
  chk(part, at::kFloat, T_::part_size((int)B), "part");
  chk(w, at::kFloat, T_::C * 9, "w");
  chk(b, at::kFloat, T_::C, "b");
  chk(ws, at::kBFloat16, 9 * T_::C, "ws");
  chk_lr(lr);
  return B;
}

void tfcnn_conv_wgrad_sgd(const Tensor& dz, const Tensor& x, const c10::optional<Tensor>& idx, const Tensor& part,
                          const Tensor& w, const Tensor& wm, const Tensor& b, const Tensor& bm, const Tensor& ws,
                          const Tensor& lr, double momentum) {
  const int64_t B = chk_wgrad(dz, x, idx, part, w, b, ws, lr);
  chk(wm, at::kFloat, T_::C * 9, "wm");
  chk(bm, at::kFloat, T_::C, "bm");
  ok(T_::conv_wgrad_sgd(bp(dz), bp(x), idx_p(idx), part.data_ptr<float>(), w.data_ptr<float>(), wm.data_ptr<float>(),
                        b.data_ptr<float>(), bm.data_ptr<float>(), bp(ws), lr.data_ptr<float>(), (float)momentum,
                        (int)B, stream()),
     "tfcnn_conv_wgrad_sgd");
}

void tfcnn_conv_wgrad_adam(const Tensor& dz, const Tensor& x, const c10::optional<Tensor>& idx, const Tensor& part,
                           const Tensor& w, const Tensor& m, const Tensor& v, const Tensor& b, const Tensor& bm,
                           const Tensor& bv, const Tensor& ws, const Tensor& lr, const Tensor& step_t, double beta1,
                           double beta2, double eps) {
  const int64_t B = chk_wgrad(dz, x, idx, part, w, b, ws, lr);
  chk(m, at::kFloat, T_::C * 9, "m");
  chk(v, at::kFloat, T_::C * 9, "v");
  chk(bm, at::kFloat, T_::C, "bm");
  chk(bv, at::kFloat, T_::C, "bv");
  TORCH_CHECK(step_t.is_cuda() && step_t.scalar_type() == at::kInt && step_t.numel() == 1,
              "step_t must be a GPU int32 tensor of one element");
  ok(T_::conv_wgrad_adam(bp(dz), bp(x), idx_p(idx), part.data_ptr<float>(), w.data_ptr<float>(), m.data_ptr<float>(),
                         v.data_ptr<float>(), b.data_ptr<float>(), bm.data_ptr<float>(), bv.data_ptr<float>(), bp(ws),
                         lr.data_ptr<float>(), step_t.data_ptr<int>(), (float)beta1, (float)beta2, (float)eps, (int)B,
                         stream()),
     "tfcnn_conv_wgrad_adam");
}

}  // namespace

void register_mnist_tfcnn(py::module& m) {
  m.def("tfcnn_conv_fwd", &tfcnn_conv_fwd, "3x3 conv 1->32 + bias + ReLU, pixel-major output [B][676][32], row gather");
  m.def("tfcnn_conv_wgrad_sgd", &tfcnn_conv_wgrad_sgd, "conv weight/bias gradient with fused SGD-momentum update");
  m.def("tfcnn_conv_wgrad_adam", &tfcnn_conv_wgrad_adam,
        "conv weight/bias gradient with fused Adam update (t = step_t[0], 1-based)");
  m.def("tfcnn_part_size", [](int64_t B) { return T_::part_size((int)B); },
        "fp32 elements of the conv weight-gradient partial buffer at batch B");
}
