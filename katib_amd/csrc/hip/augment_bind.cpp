// torch binding of the augmenting batch gather (augment.hip). The source and destination kinds
// follow from the dtypes; every tensor is checked against the sizes the kernel indexes.
#include <c10/hip/HIPStream.h>
#include <torch/extension.h>

#include "augment.h"

namespace py = pybind11;
using at::Tensor;
namespace A_ = katib_hip::aug;

namespace {

void chk(const Tensor& t, at::ScalarType dt, const char* name, const Tensor& ref) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == dt && t.is_contiguous(), "augment_gather: ", name,
              " must be a contiguous ", c10::toString(dt), " GPU tensor");
  TORCH_CHECK(t.device() == ref.device(), "augment_gather: ", name, " must be on the device of out");
}

// src: u8 [N, H, W, 4] (+ lut [C, 256] f32) | f32 [N, C, H, W] | bf16 [N, H, W, C]; idx: [B] int64;
// out: f32 [B, C, H, W] (from u8, f32) | bf16 [B, H, W, C8] (from u8, bf16) | with dst == kDstNHWC bf16
// [B, H, W, C] (from u8, bf16). dst < 0 takes the destination kind from out's dtype, as the first 11
// arguments always did. rx | ry > 0 selects translation mode (NHWC only, pad == 0).
void augment_gather(const Tensor& src, const c10::optional<Tensor>& lut, const Tensor& idx, const Tensor& out,
                    int64_t pad, bool flip, int64_t seed_lo, int64_t seed_hi, int64_t stream, int64_t epoch,
                    const c10::optional<Tensor>& epoch_t, int64_t rx, int64_t ry, int64_t dst) {
  TORCH_CHECK(src.dim() == 4 && out.dim() == 4 && idx.dim() == 1, "augment_gather: src / out are 4-D, idx is [B]");
  TORCH_CHECK(pad >= 0 && pad <= A_::kMaxPad, "augment_gather: 0 <= pad <= ", A_::kMaxPad, ", got ", pad);
  A_::Args a{};
  int sk = 0, dk = 0;
  const int64_t B = idx.size(0);
  int64_t C = 0, H = 0, W = 0;
  if (src.scalar_type() == at::kByte) {
    sk = A_::kSrcU8;
    TORCH_CHECK(lut.has_value(), "augment_gather: a u8 source needs its lut [C, 256]");
    chk(*lut, at::kFloat, "lut", out);
    TORCH_CHECK(lut->dim() == 2 && lut->size(1) == 256 && lut->size(0) >= 1 && lut->size(0) <= A_::kLutChannels,
                "augment_gather: lut must be [C <= ", A_::kLutChannels, ", 256]");
    TORCH_CHECK(src.size(3) == 4, "augment_gather: a u8 source is packed [N, H, W, 4]");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(src.data_ptr()) % 4 == 0, "augment_gather: src must be 4-byte aligned");
    C = lut->size(0), H = src.size(1), W = src.size(2);
    a.lut = lut->data_ptr<float>();
  } else if (src.scalar_type() == at::kFloat) {
    sk = A_::kSrcF32;
    C = src.size(1), H = src.size(2), W = src.size(3);
  } else if (src.scalar_type() == at::kBFloat16) {
    sk = A_::kSrcBf16;
    H = src.size(1), W = src.size(2), C = src.size(3);
  } else {
    TORCH_CHECK(false, "augment_gather: src must be uint8, float32 or bfloat16");
  }
  chk(src, src.scalar_type(), "src", out);
  chk(idx, at::kLong, "idx", out);
  TORCH_CHECK(C >= 1 && H >= 1 && W >= 1, "augment_gather: empty image");
  TORCH_CHECK(rx >= 0 && rx <= 128 * W, "augment_gather: 0 <= rx <= 128 * W = ", 128 * W, ", got ", rx);
  TORCH_CHECK(ry >= 0 && ry <= 128 * H, "augment_gather: 0 <= ry <= 128 * H = ", 128 * H, ", got ", ry);
  const bool translate = rx > 0 || ry > 0;
  TORCH_CHECK(!translate || pad == 0, "augment_gather: translation (rx, ry) needs pad == 0, got pad = ", pad);
  TORCH_CHECK(dst < 0 || dst == A_::kDstNHWC, "augment_gather: dst is -1 (from out's dtype) or ", (int)A_::kDstNHWC,
              " (NHWC), got ", dst);
  TORCH_CHECK(!translate || dst == A_::kDstNHWC, "augment_gather: translation (rx, ry) is built for the NHWC dst");
  int64_t C8 = 0;
  if (dst == A_::kDstNHWC) {
    dk = A_::kDstNHWC;
    TORCH_CHECK(sk != A_::kSrcF32, "augment_gather: bf16 [B, H, W, C] output is built for u8 and bf16 sources");
    TORCH_CHECK(out.scalar_type() == at::kBFloat16 && out.size(0) == B && out.size(1) == H && out.size(2) == W &&
                    out.size(3) == C,
                "augment_gather: an NHWC out must be bfloat16 [B, H, W, C] = [", B, ", ", H, ", ", W, ", ", C, "]");
    TORCH_CHECK(H * W * C < (1ll << 31), "augment_gather: image too large");
  } else if (out.scalar_type() == at::kFloat) {
    dk = A_::kDstNCHW;
    TORCH_CHECK(sk != A_::kSrcBf16, "augment_gather: fp32 [B, C, H, W] output is built for u8 and f32 sources");
    TORCH_CHECK(out.size(0) == B && out.size(1) == C && out.size(2) == H && out.size(3) == W,
                "augment_gather: out must be [B, C, H, W] = [", B, ", ", C, ", ", H, ", ", W, "]");
    TORCH_CHECK(B * C * H * W < (1ll << 40), "augment_gather: batch too large");
  } else if (out.scalar_type() == at::kBFloat16) {
    dk = A_::kDstC8;
    TORCH_CHECK(sk != A_::kSrcF32, "augment_gather: bf16 [B, H, W, C8] output is built for u8 and bf16 sources");
    C8 = out.size(3);
    TORCH_CHECK(C8 % 8 == 0 && C <= C8, "augment_gather: C8 % 8 == 0 and C <= C8, got C8 = ", C8, ", C = ", C);
    TORCH_CHECK(out.size(0) == B && out.size(1) == H && out.size(2) == W,
                "augment_gather: out must be [B, H, W, C8] = [", B, ", ", H, ", ", W, ", C8]");
    TORCH_CHECK(H * W * C8 < (1ll << 31), "augment_gather: image too large");
  } else {
    TORCH_CHECK(false, "augment_gather: out must be float32 [B, C, H, W] or bfloat16 [B, H, W, C8]");
  }
  chk(out, out.scalar_type(), "out", out);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(out.data_ptr()) % 16 == 0, "augment_gather: out must be 16-byte aligned");
  TORCH_CHECK(B * H * W < (1ll << 31), "augment_gather: batch too large (B * H * W < 2^31)");
  if (epoch_t.has_value()) {
    chk(*epoch_t, at::kInt, "epoch", out);
    TORCH_CHECK(epoch_t->numel() == 1, "augment_gather: the device epoch is one int32");
    a.epoch_ptr = epoch_t->data_ptr<int32_t>();
  }
  a.src = src.data_ptr();
  a.idx = idx.data_ptr<int64_t>();
  a.out = out.data_ptr();
  a.epoch_imm = (uint32_t)epoch;
  a.n_src = src.size(0);
  a.B = (int)B, a.C = (int)C, a.H = (int)H, a.W = (int)W, a.C8 = (int)C8;
  a.pad = (int)pad, a.flip = flip ? 1 : 0;
  a.rx = (int)rx, a.ry = (int)ry;
  a.seed_lo = (uint32_t)seed_lo, a.seed_hi = (uint32_t)seed_hi, a.stream = (uint32_t)stream;
  TORCH_CHECK(A_::launch(sk, dk, a, c10::hip::getCurrentHIPStream().stream()) == hipSuccess,
              "augment_gather launch failed");
}

}  // namespace

void register_augment(py::module& m) {
  m.def("augment_gather", &augment_gather,
        "batch gather by data-set index with Philox-keyed random crop + flip, or flip + bilinear translation "
        "(+ u8 table normalisation)",
        py::arg("src"), py::arg("lut"), py::arg("idx"), py::arg("out"), py::arg("pad"), py::arg("flip"),
        py::arg("seed_lo"), py::arg("seed_hi"), py::arg("stream"), py::arg("epoch"), py::arg("epoch_t"),
        py::arg("rx") = 0, py::arg("ry") = 0, py::arg("dst") = -1);
}
