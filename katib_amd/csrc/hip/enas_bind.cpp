// torch bindings for the ENAS controller kernel and the child's one-launch Adam (module
// katib_amd._hipkern, enas_* entry points). Shapes, dtypes, devices and the LDS budget are validated
// here before the launch.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include <cstring>

#include "enas_ctrl.h"
#include "enas_fanin.h"
#include "enas_optim.h"

using at::Tensor;
namespace E = katib_hip::enas;

namespace {

void check(const Tensor& t, at::ScalarType ty, int64_t n, const char* name, const Tensor& ref) {
  TORCH_CHECK(t.is_cuda() && t.device() == ref.device(), name, " must be on the controller's GPU");
  TORCH_CHECK(t.scalar_type() == ty, name, " has the wrong dtype");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.numel() >= n, name, " is too small (", t.numel(), " < ", n, ")");
}

E::Args make_args(Tensor P, int64_t L, int64_t n_ops, int64_t H, py::dict cfg) {
  TORCH_CHECK(H >= 1 && H <= E::kMaxH, "controller_hidden_size must be in [1, ", E::kMaxH, "] for the HIP controller");
  TORCH_CHECK(n_ops >= 1 && n_ops <= E::kMaxOps, "number of operations out of range for the HIP controller");
  TORCH_CHECK(L >= 1 && L <= E::kMaxLayers, "num_layers out of range for the HIP controller");
  TORCH_CHECK(E::lds_bytes(H, n_ops, L) <= 160 * 1024, "controller does not fit the 160 KB LDS");
  const E::Offsets o = E::offsets(H, n_ops);
  check(P, at::kFloat, o.n, "params", P);
  E::Args a{};
  a.P = P.data_ptr<float>();
  a.L = L;
  a.n_ops = n_ops;
  a.H = H;
  auto opt = [&](const char* k, int& use, float& val) {
    py::object v = cfg[k];
    use = v.is_none() ? 0 : 1;
    val = v.is_none() ? 0.f : v.cast<float>();
  };
  opt("temperature", a.use_temp, a.temperature);
  opt("tanh_const", a.use_tanh, a.tanh_c);
  opt("entropy_weight", a.use_ew, a.entropy_weight);
  opt("skip_weight", a.use_sw, a.skip_weight);
  a.skip_target = cfg["skip_target"].cast<float>();
  a.baseline_decay = cfg["baseline_decay"].cast<float>();
  a.lr = cfg["lr"].cast<float>();
  a.beta1 = cfg["beta1"].cast<float>();
  a.beta2 = cfg["beta2"].cast<float>();
  a.eps = cfg["eps"].cast<float>();
  const double decay = cfg["baseline_decay"].cast<double>(), b1 = cfg["beta1"].cast<double>(),
               b2 = cfg["beta2"].cast<double>();
  a.baseline_rate = (float)(1.0 - decay);  // as torch: the Python-double difference, then fp32
  a.omb1 = (float)(1.0 - b1);
  a.omb2 = (float)(1.0 - b2);
  TORCH_CHECK(a.skip_target > 0.f && a.skip_target < 1.f, "skip_target must be in (0, 1)");
  TORCH_CHECK(!a.use_temp || a.temperature != 0.f, "temperature must be non-zero");
  TORCH_CHECK(!a.use_tanh || a.tanh_c != 0.f, "tanh_const must be non-zero");
  return a;
}

void set_forced(E::Args& a, const c10::optional<Tensor>& forced, int64_t rows, const Tensor& P) {
  if (!forced.has_value() || !forced->defined()) return;
  const int alen = E::arc_len(a.L);
  check(*forced, at::kInt, alen, "forced", P);
  TORCH_CHECK(forced->numel() == alen || forced->numel() == rows * alen, "forced arcs: one arc or one per row");
  a.forced = forced->data_ptr<int>();
  a.forced_stride = forced->numel() == alen ? 0 : alen;
  auto f = forced->cpu();
  const int* fp = f.data_ptr<int>();
  for (int64_t r = 0; r < forced->numel() / alen; ++r)
    for (int l = 0, pos = 0; l < a.L; pos += l + 1, ++l) {
      TORCH_CHECK(fp[r * alen + pos] >= 0 && fp[r * alen + pos] < a.n_ops, "forced op index out of range");
      for (int i = 0; i < l; ++i) TORCH_CHECK(fp[r * alen + pos + 1 + i] == 0 || fp[r * alen + pos + 1 + i] == 1,
                                              "forced skip must be 0 or 1");
    }
}

// one arc per row of `arcs` [n, arc_len] (int32); tape [n, tape_floats]
void enas_sample(Tensor P, Tensor arcs, Tensor tape, int64_t L, int64_t n_ops, int64_t H, py::dict cfg,
                 int64_t seed, int64_t rng_offset, c10::optional<Tensor> forced) {
  E::Args a = make_args(P, L, n_ops, H, cfg);
  const int64_t n = arcs.size(0);
  TORCH_CHECK(arcs.dim() == 2 && arcs.size(1) == E::arc_len(L) && n >= 1, "arcs must be [n, arc_len]");
  check(arcs, at::kInt, n * E::arc_len(L), "arcs", P);
  check(tape, at::kFloat, n * E::tape_floats(H, n_ops, L), "tape", P);
  a.arcs = arcs.data_ptr<int>();
  a.tape = tape.data_ptr<float>();
  a.seed = (unsigned long long)seed;
  a.rng_offset = (unsigned long long)rng_offset;
  a.nsteps = 0;
  set_forced(a, forced, n, P);
  E::launch(a, (int)n, c10::hip::getCurrentHIPStream().stream());
}

// `nsteps` REINFORCE steps in one launch: arcs [nsteps, arc_len], logs [nsteps, 8]
void enas_train(Tensor P, Tensor M, Tensor V, Tensor G, Tensor tape, Tensor arcs, Tensor logs, Tensor baseline,
                int64_t L, int64_t n_ops, int64_t H, py::dict cfg, double reward, int64_t nsteps, int64_t adam_t0,
                int64_t seed, int64_t rng_offset, c10::optional<Tensor> forced, c10::optional<Tensor> phase_clocks) {
  E::Args a = make_args(P, L, n_ops, H, cfg);
  const int64_t n = E::offsets(H, n_ops).n;
  if (phase_clocks.has_value() && phase_clocks->defined()) {
    check(*phase_clocks, at::kLong, 5, "phase_clocks", P);
    a.phase_clocks = reinterpret_cast<long long*>(phase_clocks->data_ptr<int64_t>());
  }
  TORCH_CHECK(nsteps >= 1, "nsteps >= 1");
  check(M, at::kFloat, n, "adam m", P);
  check(V, at::kFloat, n, "adam v", P);
  check(G, at::kFloat, n, "grad", P);
  check(tape, at::kFloat, E::tape_floats(H, n_ops, L), "tape", P);
  check(arcs, at::kInt, nsteps * E::arc_len(L), "arcs", P);
  check(logs, at::kFloat, nsteps * E::kLogFields, "logs", P);
  check(baseline, at::kFloat, 1, "baseline", P);
  a.M = M.data_ptr<float>();
  a.V = V.data_ptr<float>();
  a.G = G.data_ptr<float>();
  a.tape = tape.data_ptr<float>();
  a.arcs = arcs.data_ptr<int>();
  a.logs = logs.data_ptr<float>();
  a.baseline = baseline.data_ptr<float>();
  a.reward = (float)reward;
  a.nsteps = (int)nsteps;
  a.adam_t0 = (int)adam_t0;
  a.seed = (unsigned long long)seed;
  a.rng_offset = (unsigned long long)rng_offset;
  set_forced(a, forced, nsteps, P);
  E::launch(a, 1, c10::hip::getCurrentHIPStream().stream());
}

// ---- the child's optimizer (enas_optim.hip)
namespace EO = katib_hip::enasoptim;

void adam_t(const Tensor& t, at::ScalarType ty, int64_t n, const char* name, const Tensor& ref) {
  TORCH_CHECK(t.is_cuda() && t.device() == ref.device() && t.scalar_type() == ty && t.is_contiguous() && t.numel() == n,
              "enas_adam: ", name, " must be a contiguous tensor of ", n, " elements on the parameters' GPU");
}

// One entry per parameter tensor: (kind, p, g, m, v, img or None, wt or None, K, C, RS, rows) with kind
// 0 = flat, 1 = conv, 2 = depthwise (enas_optim.h). Returns (device table as a uint8 tensor, segment
// count, total workgroups).
py::tuple adam_table(const std::vector<py::tuple>& entries) {
  TORCH_CHECK(!entries.empty(), "enas_adam_table: no parameters");
  std::vector<EO::Seg> segs;
  int64_t tiles = 0;
  const Tensor first = entries[0][1].cast<Tensor>();
  for (const auto& e : entries) {
    TORCH_CHECK(e.size() == 11, "enas_adam_table: entries are (kind, p, g, m, v, img, wt, K, C, RS, rows)");
    const int64_t kind = e[0].cast<int64_t>(), K = e[7].cast<int64_t>(), C = e[8].cast<int64_t>(),
                  RS = e[9].cast<int64_t>(), rows = e[10].cast<int64_t>();
    const Tensor p = e[1].cast<Tensor>(), g = e[2].cast<Tensor>(), m = e[3].cast<Tensor>(), v = e[4].cast<Tensor>();
    const int64_t n = p.numel();
    TORCH_CHECK(n >= 1 && n < (1ll << 31), "enas_adam_table: a parameter has 1 to 2^31 - 1 elements");
    adam_t(p, at::kFloat, n, "p", first);
    adam_t(m, at::kFloat, n, "m", first);
    adam_t(v, at::kFloat, n, "v", first);
    EO::Seg s{};
    s.kind = (int)kind;
    s.n = (int)n;
    if (kind == EO::kFlat) {
      TORCH_CHECK(e[5].is_none() && e[6].is_none(), "enas_adam_table: a flat segment has no image");
      adam_t(g, at::kFloat, n, "g", first);
    } else if (kind == EO::kConv) {
      const int64_t C8 = (C + 7) / 8 * 8;
      TORCH_CHECK(K >= 1 && C >= 1 && RS >= 1 && n == K * RS * C, "enas_adam_table: filter geometry does not match p");
      TORCH_CHECK(K * RS * C8 < (1ll << 31), "enas_adam_table: K * RS * C8 >= 2^31");
      TORCH_CHECK(!e[5].is_none(), "enas_adam_table: a conv segment needs its [K][RS][C8] image");
      adam_t(g, at::kFloat, K * RS * C8, "g", first);
      const Tensor wk = e[5].cast<Tensor>();
      adam_t(wk, at::kBFloat16, K * RS * C8, "wk", first);
      s.img = wk.data_ptr();
      if (!e[6].is_none()) {
        const Tensor wt = e[6].cast<Tensor>();
        adam_t(wt, at::kBFloat16, K * RS * C8, "wt", first);
        s.wt = wt.data_ptr();
      }
      s.K = (int)K, s.C = (int)C, s.C8 = (int)C8, s.RS = (int)RS;
    } else {
      TORCH_CHECK(kind == EO::kDepthwise, "enas_adam_table: kind is 0, 1 or 2");
      TORCH_CHECK(K >= 1 && RS >= 1 && n == K * RS && rows >= 1 && rows <= EO::kMaxRows,
                  "enas_adam_table: depthwise geometry does not match p, or rows outside [1, ", EO::kMaxRows, "]");
      TORCH_CHECK(rows * n < (1ll << 31), "enas_adam_table: rows * Co * KK >= 2^31");
      TORCH_CHECK(!e[5].is_none() && e[6].is_none(), "enas_adam_table: a depthwise segment has one image");
      adam_t(g, at::kFloat, rows * n, "partials", first);
      const Tensor img = e[5].cast<Tensor>();
      adam_t(img, at::kFloat, n, "image", first);
      s.img = img.data_ptr();
      s.K = (int)K, s.RS = (int)RS, s.rows = (int)rows;
    }
    s.p = p.data_ptr<float>();
    s.g = g.data_ptr<float>();
    s.m = m.data_ptr<float>();
    s.v = v.data_ptr<float>();
    s.tile0 = (int)tiles;
    tiles += EO::tiles(s);
    TORCH_CHECK(tiles < (1ll << 31), "enas_adam_table: too many workgroups");
    segs.push_back(s);
  }
  auto host = at::empty({(int64_t)(segs.size() * sizeof(EO::Seg))}, at::TensorOptions().dtype(at::kByte));
  std::memcpy(host.data_ptr(), segs.data(), segs.size() * sizeof(EO::Seg));
  return py::make_tuple(host.to(first.device()), (int64_t)segs.size(), tiles);
}

// counters: int32 [2] = (completed updates t, ticket word)
void adam(const Tensor& table, int64_t nseg, int64_t tiles, const Tensor& counters, double lr, double beta1,
          double beta2, double eps, bool update) {
  TORCH_CHECK(table.is_cuda() && table.scalar_type() == at::kByte && table.is_contiguous() &&
                  table.numel() == nseg * (int64_t)sizeof(EO::Seg) && nseg >= 1 && tiles >= 1 && tiles < (1ll << 31),
              "enas_adam: table must come from enas_adam_table");
  adam_t(counters, at::kInt, 2, "counters", table);
  TORCH_CHECK(EO::launch(reinterpret_cast<const EO::Seg*>(table.data_ptr()), (int)nseg, (int)tiles,
                         counters.data_ptr<int32_t>(), (float)lr, (float)beta1, (float)beta2, (float)eps,
                         update ? 1 : 0, c10::hip::getCurrentHIPStream().stream()) == hipSuccess,
              "enas_adam launch failed");
}

// ---- the child's gradient fan-in (enas_fanin.hip)
namespace EF = katib_hip::enasfanin;

void fanin_t(const Tensor& t, const Tensor& gx, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == gx.device() && t.scalar_type() == at::kBFloat16 && t.dim() == 4, "enas_fanin: ",
              name, " must be a 4-D bf16 tensor on the GPU of gx");
}

// x [B, H, H, C] (None when no term has a ReLU), gx like it; terms = (g, off, relu) with g [B, m, m, Cg] read in
// place: channels adjacent, pixels gs >= Cg elements apart, rows and images dense over that stride
void enas_fanin(const c10::optional<Tensor>& x, const std::vector<py::tuple>& terms, const Tensor& gx) {
  TORCH_CHECK(gx.defined() && gx.dim() == 4, "enas_fanin: gx is [B, H, H, C]");
  fanin_t(gx, gx, "gx");
  const int64_t B = gx.size(0), H = gx.size(1), C = gx.size(3);
  TORCH_CHECK(gx.is_contiguous() && gx.size(2) == H && gx.numel() > 0 && C % 8 == 0,
              "enas_fanin: gx must be a contiguous [B, H, H, C] with a square map and C % 8 == 0");
  TORCH_CHECK(B < (1 << 20) && H < (1 << 20) && C < (1 << 20), "enas_fanin: producer out of range");
  TORCH_CHECK(!terms.empty() && (int64_t)terms.size() <= EF::kMaxTerms, "enas_fanin: 1 to ", EF::kMaxTerms,
              " terms, got ", terms.size());
  EF::Table tb{};
  tb.n = (int)terms.size();
  tb.B = (int)B, tb.H = (int)H, tb.C8 = (int)(C / 8);
  for (int k = 0; k < tb.n; ++k) {
    TORCH_CHECK(terms[k].size() == 3, "enas_fanin: terms are (g, off, relu)");
    const Tensor g = terms[k][0].cast<Tensor>();
    const int64_t off = terms[k][1].cast<int64_t>();
    fanin_t(g, gx, "a term's gradient");
    const int64_t m = g.size(1), Cg = g.size(3);
    TORCH_CHECK(g.size(0) == B && g.size(2) == m && m >= H && m < (1 << 20) && Cg < (1 << 24),
                "enas_fanin: a term's gradient is [B, m, m, Cg] with m >= H");
    TORCH_CHECK(off >= 0 && off + C <= Cg, "enas_fanin: channels off .. off + C reach past the term's gradient");
    TORCH_CHECK(Cg == 1 || g.stride(3) == 1, "enas_fanin: a term's channels must be adjacent");
    // the pixel stride, from the first dimension that has one (a dimension of size 1 has no say)
    const int64_t gs = m > 1 ? g.stride(2) : (B > 1 ? g.stride(0) : (Cg + 7) / 8 * 8);
    TORCH_CHECK(gs >= Cg && gs % 8 == 0 && gs < (1ll << 31) && (m == 1 || g.stride(1) == m * gs) &&
                    (B == 1 || g.stride(0) == m * m * gs),
                "enas_fanin: a term's gradient must be dense up to a pixel stride >= Cg that is a multiple of 8");
    const int sh = (int)(off % 8);
    const int64_t last = (B * m * m - 1) * gs + (off / 8 + C / 8 + (sh ? 1 : 0)) * 8;  // one past the last element read
    TORCH_CHECK((g.storage_offset() + last) * 2 <= (int64_t)g.storage().nbytes(), "enas_fanin: a term reaches past its storage");
    if (sh) {
      TORCH_CHECK(tb.sh == 0 || tb.sh == sh, "enas_fanin: the shifted terms of a launch share one off % 8");
      tb.sh = sh;
      tb.shift |= 1u << k;
    }
    if (terms[k][2].cast<bool>()) tb.relu |= 1u << k;
    tb.k[k] = EF::Term{g.data_ptr(), (int)(gs / 8), (int)m, (int)((m - H) / 2), (int)(off / 8)};
  }
  if (tb.relu) {
    TORCH_CHECK(x.has_value() && x->defined(), "enas_fanin: a ReLU term needs x");
    fanin_t(*x, gx, "x");
    TORCH_CHECK(x->is_contiguous() && x->sizes() == gx.sizes(), "enas_fanin: x must be contiguous and shaped like gx");
    tb.x = x->data_ptr();
  }
  const char* why = EF::finish(tb, gx.data_ptr());
  TORCH_CHECK(why == nullptr, "enas_fanin: ", why ? why : "");
  TORCH_CHECK(EF::launch(tb, gx.data_ptr(), c10::hip::getCurrentHIPStream().stream()) == hipSuccess,
              "enas_fanin launch failed");
}

}  // namespace

void register_enas(py::module& m) {
  m.def("enas_fanin", &enas_fanin,
        "gradient of one layer output summed over all its readers: fp32 sum of up to 16 (g, off, relu) terms, the ReLU "
        "terms behind the mask x > 0, one rounding to bf16");
  m.def("enas_adam_table", &adam_table, "validate + upload the segment table of the child's one-launch Adam");
  m.def("enas_adam", &adam,
        "one-launch Adam over every segment: zeroes the gradient buffers, sums the depthwise partials, re-emits "
        "the weight images and advances the device step counter (update=False: images only)");
  m.def("enas_sample", &enas_sample, "ENAS controller: sample one arc per workgroup");
  m.def("enas_train", &enas_train, "ENAS controller: nsteps REINFORCE steps (sample, BPTT, Adam) in one workgroup",
        py::arg("P"), py::arg("M"), py::arg("V"), py::arg("G"), py::arg("tape"), py::arg("arcs"), py::arg("logs"),
        py::arg("baseline"), py::arg("L"), py::arg("n_ops"), py::arg("H"), py::arg("cfg"), py::arg("reward"),
        py::arg("nsteps"), py::arg("adam_t0"), py::arg("seed"), py::arg("rng_offset"), py::arg("forced"),
        py::arg("phase_clocks") = py::none());
  m.def("enas_tape_floats", [](int64_t H, int64_t n_ops, int64_t L) { return E::tape_floats(H, n_ops, L); });
  m.def("enas_n_params", [](int64_t H, int64_t n_ops) { return E::offsets(H, n_ops).n; });
  m.def("enas_lds_bytes", [](int64_t H, int64_t n_ops, int64_t L) { return E::lds_bytes(H, n_ops, L); });
  m.attr("ENAS_LOG_FIELDS") = E::kLogFields;
  m.attr("ENAS_MAX_H") = E::kMaxH;
  m.attr("ENAS_MAX_OPS") = E::kMaxOps;
  m.attr("ENAS_MAX_LAYERS") = E::kMaxLayers;
  m.attr("ENAS_LDS_LIMIT") = 160 * 1024;
}
