// torch bindings of the NHWC depthwise convolution kernels (dwconv.hip). The geometry is
// checked against every tensor before launch: the kernels' gathers are bounds-checked per
// tap, and these checks keep the grid and the 16-byte vector accesses inside the tensors.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include "dwconv.h"
#include "enas_concat.h"
#include "enas_head.h"
#include "pool_nhwc.h"

namespace py = pybind11;
using at::Tensor;
namespace D = katib_hip::dwconv;

namespace {

D::Geom make_geom(const std::vector<int64_t>& v) {
  TORCH_CHECK(v.size() == 11, "geometry: N,H,W,C,DM,K,S,pt,pl,OH,OW");
  D::Geom g{};
  int* f[11] = {&g.N, &g.H, &g.W, &g.C, &g.DM, &g.K, &g.S, &g.pt, &g.pl, &g.OH, &g.OW};
  for (int i = 0; i < 11; ++i) {
    TORCH_CHECK(v[i] >= 0 && v[i] < (1 << 30), "geometry value out of range");
    *f[i] = (int)v[i];
  }
  TORCH_CHECK(g.N > 0 && g.H > 0 && g.W > 0 && g.OH > 0 && g.OW > 0, "empty geometry");
  TORCH_CHECK(g.C % 8 == 0, "depthwise conv: C must be a multiple of 8");
  TORCH_CHECK(g.DM == 1 || g.DM == 2, "depth multiplier must be 1 or 2");
  TORCH_CHECK(g.K == 3 || g.K == 5 || g.K == 7, "kernel size must be 3, 5 or 7");
  TORCH_CHECK(g.S == 1 || g.S == 2, "stride must be 1 or 2");
  TORCH_CHECK(g.pt < g.K && g.pl < g.K, "padding must be smaller than the kernel");
  TORCH_CHECK((int64_t)(g.OH - 1) * g.S - g.pt < g.H && (int64_t)(g.OW - 1) * g.S - g.pl < g.W,
              "output size inconsistent with the geometry");
  TORCH_CHECK((int64_t)g.N * g.H * g.W * g.C * g.DM < (1ll << 40), "tensor too large");
  return g;
}

void check(const Tensor& t, at::ScalarType ty, int64_t numel, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == ty && t.is_contiguous(), name, " must be a contiguous ",
              ty == at::kBFloat16 ? "bf16" : "fp32", " GPU tensor");
  TORCH_CHECK(t.numel() == numel, name, " has ", t.numel(), " elements, geometry needs ", numel);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name, " must be 16-byte aligned");
}

hipStream_t stream() { return c10::hip::getCurrentHIPStream().stream(); }

const __hip_bfloat16* bf(const Tensor& t) { return reinterpret_cast<const __hip_bfloat16*>(t.data_ptr()); }
__hip_bfloat16* bfm(const Tensor& t) { return reinterpret_cast<__hip_bfloat16*>(t.data_ptr()); }

// x [N,H,W,C] bf16, w [K*K][C*DM] fp32 (tap-major), bias [C*DM] fp32 or None, y [N,OH,OW,C*DM] bf16
void dw_fwd(const Tensor& x, const Tensor& w, const c10::optional<Tensor>& bias, const Tensor& y,
            const std::vector<int64_t>& geom) {
  const D::Geom g = make_geom(geom);
  const int64_t Co = (int64_t)g.C * g.DM;
  check(x, at::kBFloat16, (int64_t)g.N * g.H * g.W * g.C, "x");
  check(w, at::kFloat, g.K * g.K * Co, "w");
  check(y, at::kBFloat16, (int64_t)g.N * g.OH * g.OW * Co, "y");
  const float* b = nullptr;
  if (bias.has_value() && bias->defined()) {
    check(*bias, at::kFloat, Co, "bias");
    b = bias->data_ptr<float>();
  }
  TORCH_CHECK(D::launch_fwd(g, bf(x), w.data_ptr<float>(), b, bfm(y), stream()) == hipSuccess, "dw_fwd launch failed");
}

void dw_dgrad(const Tensor& gy, const Tensor& w, const Tensor& gx, const std::vector<int64_t>& geom) {
  const D::Geom g = make_geom(geom);
  const int64_t Co = (int64_t)g.C * g.DM;
  check(gy, at::kBFloat16, (int64_t)g.N * g.OH * g.OW * Co, "gy");
  check(w, at::kFloat, g.K * g.K * Co, "w");
  check(gx, at::kBFloat16, (int64_t)g.N * g.H * g.W * g.C, "gx");
  TORCH_CHECK(D::launch_dgrad(g, bf(gy), w.data_ptr<float>(), bfm(gx), stream()) == hipSuccess, "dw_dgrad launch failed");
}

// part [rows][C*DM][K*K] fp32 partial weight gradients (rows = dw_wgrad_rows(geom))
void dw_wgrad(const Tensor& x, const Tensor& gy, const Tensor& part, const std::vector<int64_t>& geom) {
  const D::Geom g = make_geom(geom);
  const int64_t Co = (int64_t)g.C * g.DM;
  const int rows = D::wgrad_rows(g);
  check(x, at::kBFloat16, (int64_t)g.N * g.H * g.W * g.C, "x");
  check(gy, at::kBFloat16, (int64_t)g.N * g.OH * g.OW * Co, "gy");
  check(part, at::kFloat, (int64_t)rows * Co * g.K * g.K, "part");
  TORCH_CHECK(D::launch_wgrad(g, bf(x), bf(gy), part.data_ptr<float>(), rows, stream()) == hipSuccess,
              "dw_wgrad launch failed");
}

// ---- NHWC bf16 pooling (pool_nhwc.hip): geometry (N, H, W, C, P, S)
katib_hip::poolnhwc::Geom pool_geom(const std::vector<int64_t>& v) {
  TORCH_CHECK(v.size() == 6, "pool geometry: N,H,W,C,P,S");
  for (int64_t e : v) TORCH_CHECK(e > 0 && e < (1 << 30), "pool geometry value out of range");
  katib_hip::poolnhwc::Geom g{(int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], (int)v[5], 0, 0};
  TORCH_CHECK(g.C % 8 == 0, "pool: C must be a multiple of 8");
  TORCH_CHECK(g.P <= 16 && g.P <= g.H && g.P <= g.W, "pool window must fit the input (and be <= 16)");
  g.OH = (g.H - g.P) / g.S + 1;
  g.OW = (g.W - g.P) / g.S + 1;
  TORCH_CHECK((int64_t)g.N * g.H * g.W * g.C < (1ll << 40), "tensor too large");
  return g;
}

// x [N,H,W,C] bf16 -> y [N,OH,OW,C] bf16 (+ arg uint8, max pooling)
void pool_fwd(const Tensor& x, const Tensor& y, const c10::optional<Tensor>& arg, bool is_max,
              const std::vector<int64_t>& geom) {
  const auto g = pool_geom(geom);
  check(x, at::kBFloat16, (int64_t)g.N * g.H * g.W * g.C, "x");
  check(y, at::kBFloat16, (int64_t)g.N * g.OH * g.OW * g.C, "y");
  void* a = nullptr;
  if (is_max) {
    TORCH_CHECK(arg.has_value() && arg->defined(), "max pooling needs the argmax buffer");
    check(*arg, at::kByte, (int64_t)g.N * g.OH * g.OW * g.C, "arg");
    a = arg->data_ptr();
  }
  TORCH_CHECK(katib_hip::poolnhwc::launch_fwd(g, is_max, x.data_ptr(), y.data_ptr(), a, stream()) == hipSuccess,
              "pool_fwd launch failed");
}

void pool_bwd(const Tensor& gy, const c10::optional<Tensor>& arg, const Tensor& gx, bool is_max,
              const std::vector<int64_t>& geom) {
  const auto g = pool_geom(geom);
  check(gy, at::kBFloat16, (int64_t)g.N * g.OH * g.OW * g.C, "gy");
  check(gx, at::kBFloat16, (int64_t)g.N * g.H * g.W * g.C, "gx");
  const void* a = nullptr;
  if (is_max) {
    TORCH_CHECK(arg.has_value() && arg->defined(), "max pooling backward needs the argmax buffer");
    check(*arg, at::kByte, (int64_t)g.N * g.OH * g.OW * g.C, "arg");
    a = arg->data_ptr();
  }
  TORCH_CHECK(katib_hip::poolnhwc::launch_bwd(g, is_max, gy.data_ptr(), a, gx.data_ptr(), stream()) == hipSuccess,
              "pool_bwd launch failed");
}

// ---- layer-input builder (enas_concat.hip): ReLU + zero-pad + concat of NHWC bf16 sources
namespace EC = katib_hip::enasconcat;

void concat_src(const Tensor& t, int64_t B, int64_t H, int64_t C, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16 && t.is_contiguous(), name,
              " must be a contiguous bf16 GPU tensor");
  TORCH_CHECK(t.dim() == 4 && t.size(0) == B && t.size(1) == H && t.size(2) == H && t.size(3) == C, name,
              " must be [B, H, H, C] with a square map and the common batch size");
}

// xs[i] [B, H_i, H_i, C_i] -> out [B, m, m, Cs]: Cs = sum C_i, with pad8 rounded up to a multiple of 8
void enas_concat_fwd(const std::vector<Tensor>& xs, const Tensor& out, bool relu, bool pad8) {
  TORCH_CHECK(!xs.empty() && (int64_t)xs.size() <= EC::kMaxSrc, "enas_concat: 1 to ", EC::kMaxSrc, " sources, got ",
              xs.size());
  TORCH_CHECK(xs[0].dim() == 4, "enas_concat: sources are [B, H, H, C]");
  EC::Table tb{};
  tb.n = (int)xs.size();
  tb.B = (int)xs[0].size(0);
  for (int i = 0; i < tb.n; ++i) {
    TORCH_CHECK(xs[i].dim() == 4 && xs[i].size(1) < (1 << 20) && xs[i].size(3) < (1 << 20), "enas_concat: bad source");
    concat_src(xs[i], tb.B, xs[i].size(1), xs[i].size(3), "source");
    TORCH_CHECK(xs[i].device() == out.device(), "enas_concat: tensors on different devices");
    tb.s[i].x = xs[i].data_ptr();
    tb.s[i].H = (int)xs[i].size(1);
    tb.s[i].C = (int)xs[i].size(3);
  }
  TORCH_CHECK(EC::finish(tb, 0, pad8), "enas_concat: empty source or B * m * m * C >= 2^31");
  concat_src(out, tb.B, tb.m, tb.Cs, "out");
  TORCH_CHECK(EC::launch_fwd(tb, relu, out.data_ptr(), stream()) == hipSuccess, "enas_concat_fwd launch failed");
}

// geom[i] = (H_i, C_i); xs[i] (read only with relu) and gxs[i] [B, H_i, H_i, C_i], gxs[i] None where no
// gradient is wanted; gout [B, m, m, Cs] whose pixels lie gs >= Cs elements apart (Cs as in the forward;
// channels >= Ct are never read into a gx)
void enas_concat_bwd(const std::vector<std::vector<int64_t>>& geom, int64_t B,
                     const std::vector<c10::optional<Tensor>>& xs, const std::vector<c10::optional<Tensor>>& gxs,
                     const Tensor& gout, bool relu, bool pad8) {
  const size_t n = geom.size();
  TORCH_CHECK(n >= 1 && (int64_t)n <= EC::kMaxSrc, "enas_concat: 1 to ", EC::kMaxSrc, " sources, got ", n);
  TORCH_CHECK(xs.size() == n && gxs.size() == n && B >= 1 && B < (1ll << 31), "enas_concat_bwd: list lengths differ");
  TORCH_CHECK(gout.is_cuda() && gout.scalar_type() == at::kBFloat16 && gout.dim() == 4, "gout must be 4-D bf16 on a GPU");
  EC::Table tb{};
  tb.n = (int)n;
  tb.B = (int)B;
  for (size_t i = 0; i < n; ++i) {
    TORCH_CHECK(geom[i].size() == 2 && geom[i][0] >= 1 && geom[i][0] < (1 << 20) && geom[i][1] >= 1 &&
                    geom[i][1] < (1 << 20), "enas_concat_bwd: geometry is (H, C) per source");
    tb.s[i].H = (int)geom[i][0];
    tb.s[i].C = (int)geom[i][1];
    if (gxs[i].has_value() && gxs[i]->defined()) {
      concat_src(*gxs[i], B, tb.s[i].H, tb.s[i].C, "gx");
      TORCH_CHECK(gxs[i]->device() == gout.device(), "enas_concat: tensors on different devices");
      tb.s[i].gx = gxs[i]->data_ptr();
      if (relu) {
        TORCH_CHECK(xs[i].has_value() && xs[i]->defined(), "enas_concat_bwd: ReLU needs the sources");
        concat_src(*xs[i], B, tb.s[i].H, tb.s[i].C, "source");
        TORCH_CHECK(xs[i]->device() == gout.device(), "enas_concat: tensors on different devices");
        tb.s[i].x = xs[i]->data_ptr();
      }
    }
  }
  // the pixel stride, from the first dimension that has one (a dimension of size 1 has no say)
  TORCH_CHECK(gout.size(3) == 1 || gout.stride(3) == 1, "gout channels must be adjacent");
  int64_t gs = 0;
  {
    EC::Table probe = tb;
    TORCH_CHECK(EC::finish(probe, 0, pad8), "enas_concat: B * m * m * C >= 2^31");
    const int64_t m = probe.m;
    TORCH_CHECK(gout.size(0) == B && gout.size(1) == m && gout.size(2) == m && gout.size(3) == probe.Cs,
                "gout must be [B, m, m, Cs]");
    gs = m > 1 ? gout.stride(2) : (B > 1 ? gout.stride(0) : probe.Cs);
    TORCH_CHECK(gs >= probe.Cs && (m == 1 || gout.stride(1) == m * gs) && (B == 1 || gout.stride(0) == m * m * gs),
                "gout must be dense up to a pixel stride >= Cs");
    const int64_t last = (B * m * m - 1) * gs + probe.Cs;  // one past the last element read
    TORCH_CHECK((gout.storage_offset() + last) * 2 <= (int64_t)gout.storage().nbytes(), "gout reaches past its storage");
  }
  TORCH_CHECK(EC::finish(tb, gs, pad8), "enas_concat: B * m * m * gs >= 2^31");
  TORCH_CHECK(EC::launch_bwd(tb, relu, gout.data_ptr(), (int)gs, stream()) == hipSuccess, "enas_concat_bwd launch failed");
}

// ---- head of the child (enas_head.hip): pooling, dropout, dense, softmax cross-entropy
namespace EH = katib_hip::enashead;

void head_t(const Tensor& t, at::ScalarType ty, int64_t numel, const Tensor& on, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == ty && t.is_contiguous() && t.numel() == numel &&
                  t.device() == on.device(),
              "enas_head: ", name, " must be a contiguous tensor of ", numel, " elements on the activation's GPU");
}

void head_sizes(int64_t B, int64_t HW, int64_t C, int64_t K) {
  TORCH_CHECK(B >= 1 && HW >= 1 && C >= 1 && K >= 1, "enas_head: empty tensor");
  TORCH_CHECK(K <= EH::kMaxK, "enas_head: K = ", K, " classes, the kernels serve K <= ", EH::kMaxK);
  TORCH_CHECK(C <= EH::kMaxC, "enas_head: C = ", C, " channels, the kernels serve C <= ", EH::kMaxC);
  TORCH_CHECK(B * HW * C < (1ll << 31), "enas_head: B * H * W * C >= 2^31");
}

// x [B, H, W, C] bf16 dense. thr > 0: dropout with round(p 2^32) = thr and `scale`, the draw keyed by
// (seed, site, *step). mean: out[0] = loss / B and *step += 1 (training); else the sum (evaluation).
// Returns out [2] (loss, hits), feat, keep, logits, dl, loss_b, hit_b.
std::vector<Tensor> enas_head_fwd(const Tensor& x, const Tensor& w, const Tensor& bias, const Tensor& y, int64_t thr,
                                  double scale, int64_t site, int64_t seed_lo, int64_t seed_hi,
                                  const c10::optional<Tensor>& step, bool mean, const c10::optional<Tensor>& stats) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.dim() == 4 && x.is_contiguous(),
              "enas_head: x must be a dense [B, H, W, C] bf16 GPU tensor");
  TORCH_CHECK(w.dim() == 2, "enas_head: weight is [K, C]");
  const int64_t B = x.size(0), HW = x.size(1) * x.size(2), C = x.size(3), K = w.size(0);
  head_sizes(B, HW, C, K);
  head_t(w, at::kFloat, K * C, x, "weight");
  head_t(bias, at::kFloat, K, x, "bias");
  head_t(y, at::kLong, B, x, "labels");
  TORCH_CHECK(thr >= 0 && thr < (1ll << 32) && site >= 0 && site < (1ll << 32) && seed_lo >= 0 &&
                  seed_lo < (1ll << 32) && seed_hi >= 0 && seed_hi < (1ll << 32), "enas_head: dropout words are 32-bit");
  const bool has_step = step.has_value() && step->defined();
  if (has_step) head_t(*step, at::kInt, 1, x, "step");
  TORCH_CHECK(thr == 0 || has_step, "enas_head: dropout needs the device step counter");
  const bool has_stats = stats.has_value() && stats->defined();
  if (has_stats) head_t(*stats, at::kFloat, 2, x, "stats");
  const auto f32 = x.options().dtype(at::kFloat);
  Tensor out = at::empty({2}, f32), feat = at::empty({B, C}, f32), keep = at::empty({B, C}, x.options().dtype(at::kByte)),
         logits = at::empty({B, K}, f32), dl = at::empty({B, K}, f32), loss_b = at::empty({B}, f32),
         hit_b = at::empty({B}, f32);
  EH::Fwd a{};
  a.x = x.data_ptr();
  a.w = w.data_ptr<float>();
  a.bias = bias.data_ptr<float>();
  a.y = y.data_ptr<int64_t>();
  a.step = has_step ? step->data_ptr<int32_t>() : nullptr;
  a.feat = feat.data_ptr<float>();
  a.keep = keep.data_ptr<uint8_t>();
  a.logits = logits.data_ptr<float>();
  a.dl = dl.data_ptr<float>();
  a.loss_b = loss_b.data_ptr<float>();
  a.hit_b = hit_b.data_ptr<float>();
  a.B = (int)B, a.HW = (int)HW, a.C = (int)C, a.K = (int)K;
  a.seed = (uint64_t)seed_lo | ((uint64_t)seed_hi << 32);
  a.site = (uint32_t)site, a.thr = (uint32_t)thr, a.scale = (float)scale;
  TORCH_CHECK(EH::launch_fwd(a, thr > 0, stream()) == hipSuccess, "enas_head_fwd launch failed");
  EH::Sum s{loss_b.data_ptr<float>(), hit_b.data_ptr<float>(), out.data_ptr<float>(),
            has_stats ? stats->data_ptr<float>() : nullptr, mean && has_step ? step->data_ptr<int32_t>() : nullptr,
            (int)B, mean ? 1 : 0};
  TORCH_CHECK(EH::launch_sum(s, stream()) == hipSuccess, "enas_head_sum launch failed");
  return {out, feat, keep, logits, dl, loss_b, hit_b};
}

// g: the loss's upstream gradient, one fp32 on the GPU. Returns dx [B, H, W, C] bf16, dW, db; an
// undefined tensor where none is wanted. segs > 0 sets the data role's segments per sample (A/B).
std::vector<Tensor> enas_head_bwd(const Tensor& g, const Tensor& dl, const Tensor& w, const Tensor& feat,
                                  const Tensor& keep, int64_t H, int64_t W, double scale, bool need_dx, bool need_dw,
                                  bool need_db, int64_t segs) {
  TORCH_CHECK(dl.is_cuda() && dl.dim() == 2 && feat.dim() == 2 && H >= 1 && W >= 1 && H < (1 << 20) && W < (1 << 20),
              "enas_head_bwd: dl [B, K], feat [B, C], H, W");
  const int64_t B = dl.size(0), K = dl.size(1), C = feat.size(1), HW = H * W;
  head_sizes(B, HW, C, K);
  head_t(g, at::kFloat, 1, dl, "grad");
  head_t(dl, at::kFloat, B * K, dl, "dl");
  head_t(w, at::kFloat, K * C, dl, "weight");
  head_t(feat, at::kFloat, B * C, dl, "feat");
  head_t(keep, at::kByte, B * C, dl, "keep");
  TORCH_CHECK(segs >= 0 && segs <= HW, "enas_head_bwd: 0 <= segs <= H * W");
  Tensor dx, dw, db;
  if (need_dx) dx = at::empty({B, H, W, C}, dl.options().dtype(at::kBFloat16));
  if (need_dw) dw = at::empty({K, C}, dl.options());
  if (need_db) db = at::empty({K}, dl.options());
  EH::Bwd a{};
  a.g = g.data_ptr<float>();
  a.dl = dl.data_ptr<float>();
  a.w = w.data_ptr<float>();
  a.feat = feat.data_ptr<float>();
  a.keep = keep.data_ptr<uint8_t>();
  a.dx = need_dx ? dx.data_ptr() : nullptr;
  a.dw = need_dw ? dw.data_ptr<float>() : nullptr;
  a.db = need_db ? db.data_ptr<float>() : nullptr;
  a.B = (int)B, a.HW = (int)HW, a.C = (int)C, a.K = (int)K;
  a.mscale = (float)scale / (float)HW;
  a.S = segs > 0 ? (int)segs : EH::segments((int)B, (int)HW, (int)C);
  TORCH_CHECK(EH::launch_bwd(a, stream()) == hipSuccess, "enas_head_bwd launch failed");
  return {dx, dw, db};
}

}  // namespace

void register_dwconv(py::module& m) {
  m.def("enas_head_fwd", &enas_head_fwd, "child head forward: pool, dropout, dense, softmax cross-entropy, sums");
  m.def("enas_head_bwd", &enas_head_bwd, "its backward: dx, dW, db in one launch");
  m.attr("ENAS_HEAD_MAX_K") = EH::kMaxK;
  m.attr("ENAS_HEAD_MAX_C") = EH::kMaxC;
  m.def("enas_concat_fwd", &enas_concat_fwd, "ReLU + zero-pad + channel concat of NHWC bf16 sources");
  m.def("enas_concat_bwd", &enas_concat_bwd, "its backward: one gradient per source that wants one");
  m.attr("ENAS_CONCAT_MAX_SRC") = EC::kMaxSrc;
  m.def("pool_nhwc_fwd", &pool_fwd, "max / avg pooling forward (NHWC bf16, valid padding)");
  m.def("pool_nhwc_bwd", &pool_bwd, "max / avg pooling backward (NHWC bf16, gather, no atomics)");
  m.def("dw_fwd", &dw_fwd, "depthwise conv forward (NHWC bf16)", py::arg("x"), py::arg("w"), py::arg("bias"),
        py::arg("y"), py::arg("geom"));
  m.def("dw_dgrad", &dw_dgrad, "depthwise conv input gradient (NHWC bf16)");
  m.def("dw_wgrad", &dw_wgrad, "depthwise conv weight gradient partials (fp32)");
  m.def("dw_wgrad_rows", [](const std::vector<int64_t>& geom) { return D::wgrad_rows(make_geom(geom)); });
}
