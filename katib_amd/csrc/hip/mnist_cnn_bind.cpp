// torch bindings of the fused MNIST CNN kernels (mnist_cnn.hip), with the shape / dtype / alignment
// checks the kernels and their grids rely on. The geometry is fixed; B comes from the output tensor.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include "mnist_cnn.h"

namespace py = pybind11;
using at::Tensor;
namespace C_ = katib_hip::cnn;

namespace {

hipStream_t stream() { return c10::hip::getCurrentHIPStream().stream(); }
C_::u16* bp(const Tensor& t) { return reinterpret_cast<C_::u16*>(t.data_ptr()); }
void ok(hipError_t e, const char* w) { TORCH_CHECK(e == hipSuccess, w, ": ", hipGetErrorString(e)); }

void chk(const Tensor& t, at::ScalarType dt, int64_t n, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == dt && t.is_contiguous() && t.numel() == n, name,
              " must be a contiguous ", c10::toString(dt), " GPU tensor of ", n, " elements (got ", t.numel(), ")");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name, " must be 16-byte aligned");
}
// the images: [rows][784] bf16; the gather index must address its rows, the kernels trust it
void chk_x(const Tensor& x, const c10::optional<Tensor>& idx, int64_t B) {
  TORCH_CHECK(x.dim() == 2 && x.size(1) == C_::IMG, "x must be [rows][784]");
  chk(x, at::kBFloat16, x.numel(), "x");
  if (idx.has_value()) {
    TORCH_CHECK(idx->is_cuda() && idx->scalar_type() == at::kLong && idx->is_contiguous() && idx->numel() == B,
                "idx must be a contiguous int64 GPU tensor with one entry per image");
  } else {
    TORCH_CHECK(x.size(0) == B, "x rows must match the batch without a gather");
  }
}
const int64_t* idx_p(const c10::optional<Tensor>& idx) { return idx.has_value() ? idx->data_ptr<int64_t>() : nullptr; }
int64_t batch(const Tensor& t, int64_t per, const char* name) {
  TORCH_CHECK(t.numel() > 0 && t.numel() % per == 0, name, " must hold a whole number of images");
  const int64_t B = t.numel() / per;
  TORCH_CHECK(B < (1 << 20), "batch too large");
  return B;
}
void chk_lr(const Tensor& lr) {
  TORCH_CHECK(lr.is_cuda() && lr.scalar_type() == at::kFloat && lr.numel() == 1, "lr must be a GPU fp32 scalar");
}

void cnn_conv1_pool_fwd(const Tensor& x, const c10::optional<Tensor>& idx, const Tensor& w1s, const Tensor& b1,
                        const Tensor& p1, const c10::optional<Tensor>& a1) {
  const int64_t B = batch(p1, C_::P1 * C_::C1, "p1");
  chk_x(x, idx, B);
  chk(w1s, at::kBFloat16, 25 * C_::C1, "w1s");
  chk(b1, at::kFloat, C_::C1, "b1");
  chk(p1, at::kBFloat16, B * C_::P1 * C_::C1, "p1");
  if (a1.has_value()) chk(*a1, at::kByte, B * C_::P1 * C_::C1, "a1");
  ok(C_::conv1_pool_fwd(bp(x), idx_p(idx), bp(w1s), b1.data_ptr<float>(), bp(p1),
                        a1.has_value() ? a1->data_ptr<uint8_t>() : nullptr, (int)B, stream()),
     "cnn_conv1_pool_fwd");
}

void cnn_conv2_pool_fwd(const Tensor& p1, const Tensor& w2f, const Tensor& b2, const Tensor& p2,
                        const c10::optional<Tensor>& a2) {
  const int64_t B = batch(p2, C_::F2, "p2");
  chk(p1, at::kBFloat16, B * C_::P1 * C_::C1, "p1");
  chk(w2f, at::kBFloat16, C_::N2 * C_::K2P, "w2f");
  chk(b2, at::kFloat, C_::CO, "b2");
  chk(p2, at::kBFloat16, B * C_::F2, "p2");
  if (a2.has_value()) chk(*a2, at::kByte, B * C_::F2, "a2");
  ok(C_::conv2_pool_fwd(bp(p1), bp(w2f), b2.data_ptr<float>(), bp(p2),
                        a2.has_value() ? a2->data_ptr<uint8_t>() : nullptr, (int)B, stream()),
     "cnn_conv2_pool_fwd");
}

void cnn_conv2_dgrad(const Tensor& dp2, const Tensor& a2, const Tensor& w2d, const Tensor& p1, const Tensor& dp1) {
  const int64_t B = batch(dp2, C_::F2, "dp2");
  chk(dp2, at::kBFloat16, B * C_::F2, "dp2");
  chk(a2, at::kByte, B * C_::F2, "a2");
  chk(w2d, at::kBFloat16, C_::C1 * C_::KD, "w2d");
  chk(p1, at::kBFloat16, B * C_::P1 * C_::C1, "p1");
  chk(dp1, at::kBFloat16, B * C_::P1 * C_::C1, "dp1");
  ok(C_::conv2_dgrad(bp(dp2), a2.data_ptr<uint8_t>(), bp(w2d), bp(p1), bp(dp1), (int)B, stream()),
     "cnn_conv2_dgrad");
}

void cnn_conv2_wgrad_sgd(const Tensor& dp2, const Tensor& a2, const Tensor& p1, const Tensor& part, const Tensor& w2,
                         const Tensor& w2m, const Tensor& b2, const Tensor& b2m, const Tensor& w2f,
                         const Tensor& w2d, const Tensor& lr, double momentum) {
  const int64_t B = batch(dp2, C_::F2, "dp2");
  chk(dp2, at::kBFloat16, B * C_::F2, "dp2");
  chk(a2, at::kByte, B * C_::F2, "a2");
  chk(p1, at::kBFloat16, B * C_::P1 * C_::C1, "p1");
  chk(part, at::kFloat, (int64_t)C_::wg2_slices((int)B) * C_::CO * C_::PART2_LD, "part");
  chk(w2, at::kFloat, C_::CO * C_::K2, "w2");
  chk(w2m, at::kFloat, C_::CO * C_::K2, "w2m");
  chk(b2, at::kFloat, C_::CO, "b2");
  chk(b2m, at::kFloat, C_::CO, "b2m");
  chk(w2f, at::kBFloat16, C_::N2 * C_::K2P, "w2f");
  chk(w2d, at::kBFloat16, C_::C1 * C_::KD, "w2d");
  chk_lr(lr);
  ok(C_::conv2_wgrad_sgd(bp(dp2), a2.data_ptr<uint8_t>(), bp(p1), part.data_ptr<float>(), w2.data_ptr<float>(),
                         w2m.data_ptr<float>(), b2.data_ptr<float>(), b2m.data_ptr<float>(), bp(w2f), bp(w2d),
                         lr.data_ptr<float>(), (float)momentum, (int)B, stream()),
     "cnn_conv2_wgrad_sgd");
}

void cnn_conv1_wgrad_sgd(const Tensor& dp1, const Tensor& a1, const Tensor& x, const c10::optional<Tensor>& idx,
                         const Tensor& part, const Tensor& w1, const Tensor& w1m, const Tensor& b1,
                         const Tensor& b1m, const Tensor& w1s, const Tensor& lr, double momentum) {
  const int64_t B = batch(dp1, C_::P1 * C_::C1, "dp1");
  chk(dp1, at::kBFloat16, B * C_::P1 * C_::C1, "dp1");
  chk(a1, at::kByte, B * C_::P1 * C_::C1, "a1");
  chk_x(x, idx, B);
  chk(part, at::kFloat, (int64_t)C_::wg1_slices((int)B) * C_::PART1_LD, "part");
  chk(w1, at::kFloat, C_::C1 * 25, "w1");
  chk(w1m, at::kFloat, C_::C1 * 25, "w1m");
  chk(b1, at::kFloat, C_::C1, "b1");
  chk(b1m, at::kFloat, C_::C1, "b1m");
  chk(w1s, at::kBFloat16, 25 * C_::C1, "w1s");
  chk_lr(lr);
  ok(C_::conv1_wgrad_sgd(bp(dp1), a1.data_ptr<uint8_t>(), bp(x), idx_p(idx), part.data_ptr<float>(),
                         w1.data_ptr<float>(), w1m.data_ptr<float>(), b1.data_ptr<float>(), b1m.data_ptr<float>(),
                         bp(w1s), lr.data_ptr<float>(), (float)momentum, (int)B, stream()),
     "cnn_conv1_wgrad_sgd");
}

}  // namespace

void register_mnist_cnn(py::module& m) {
  m.def("cnn_conv1_pool_fwd", &cnn_conv1_pool_fwd, "5x5 conv 1->24 + bias + ReLU + 2x2 max-pool (+ winners), row gather");
  m.def("cnn_conv2_pool_fwd", &cnn_conv2_pool_fwd, "5x5 conv 24->50 + bias + ReLU + 2x2 max-pool (+ winners), MFMA");
  m.def("cnn_conv2_dgrad", &cnn_conv2_dgrad, "conv2 data gradient from the pooled gradient and the winners");
  m.def("cnn_conv2_wgrad_sgd", &cnn_conv2_wgrad_sgd, "conv2 weight/bias gradient with fused SGD-momentum update");
  m.def("cnn_conv1_wgrad_sgd", &cnn_conv1_wgrad_sgd, "conv1 weight/bias gradient with fused SGD-momentum update");
  m.def("cnn_part_sizes", [](int64_t B) {
    return py::make_tuple((int64_t)C_::wg1_slices((int)B) * C_::PART1_LD,
                          (int64_t)C_::wg2_slices((int)B) * C_::CO * C_::PART2_LD);
  }, "fp32 elements of the conv1 / conv2 weight-gradient partial buffers at batch B");
}
