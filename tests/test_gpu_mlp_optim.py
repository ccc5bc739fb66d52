"""The B1 search space on the fused MLP kernels (csrc/hip/mlp.hip): the Adam and FTRL-proximal
weight-gradient epilogues against torch.optim.Adam / the trial's Ftrl in fp64, the device step counter
of xent_small, the depth-generic HipMLP against tests/mlp_step_oracle.py, and the trial's
``--impl hip`` with ``--num-layers`` / ``--optimizer``.

Bounds. States and shadows: 1e-2, the bar test_gpu_mlp.py::test_wgrad_sgd puts on them. Adam's update
(w_new - w_old): the larger of 1e-2 and four times the error, against the same fp64 oracle, of the
same optimizer stepped in fp32 on an fp32 torch GEMM (the rule of tests/test_gpu_darts_optim.py).
Model level: the larger of 1e-2 and four times the distance between the oracle with fp32 GEMMs and
the oracle with fp64 GEMMs at the same bf16 rounding points - accumulation order and the rounding
flips it causes, measured on the reference alone. FTRL's weight has a kink at |z| = l1: elements
whose oracle z_new lies within 0.05 of it are left out of the weight and shadow comparisons (never
of z and n), and may be at most 1 % of the elements compared. At the model level the gradients are of
order 1e-2 (the loss is a mean over the batch), so z ~ N(0, 1) alone would leave 5.6 % of the elements
within 0.05 of the kink before any kernel ran (measured: 3246 of 57688 for L = 1); there z is drawn as
u + 0.2 sign(u), u ~ N(0, 1), which keeps the margin and the cap as they are. What is still left out
is mostly the padded output rows (z = 0 exactly), which are compared exactly further down.

Every test prints the figures it measured (``pytest -s``) before it asserts.
"""
import math
import re

import pytest
import torch

import mlp_step_oracle as O
from katib_amd.workloads import mnist_mlp

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
LR = 0.02
B1, B2, EPS = 0.9, 0.999, 1e-8
L1, FBETA, WD = 0.01, 1.0, 0.0
KINK = 0.05
# (M, N, K): one partial-N tile and two K tiles (the second does not touch the bias); a row tail in the
# fourth 64-row stage, a second N tile of 8 columns and a third K tile of 8 columns
SHAPES = [(64, 16, 128), (200, 72, 136)]


def _rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-6))


@pytest.fixture(scope="module")
def k():
    from katib_amd.ops.conv import kernels

    return kernels()


def _operands(M, N, K, gather, seed):
    """dy, x, idx as test_wgrad_sgd draws them; without a gather x holds the same rows, gathered."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(1000, K, device=DEV, generator=g).to(BF16)
    idx = torch.randint(0, 1000, (M,), device=DEV, generator=g)
    dy = torch.randn(M, N, device=DEV, generator=g).to(BF16)
    if not gather:
        x, idx = x[idx].contiguous(), None
    return g, dy, x, idx


def _grads(dy, x, idx, dtype):
    xg = x[idx] if idx is not None else x
    dy, xg = dy.cpu().to(dtype), xg.cpu().to(dtype)
    return dy.t() @ xg, dy.sum(0)


def _step_ref(optimizer, dtype, values, grads, s0, s1, t=1, steps=1):
    """``steps`` steps of the real optimizer on CPU copies in ``dtype`` with preset state; ``grads`` is a
    list (one per step) of lists (one per value). Returns [(value, state 0, state 1)]."""
    cur = [(v.cpu().to(dtype), a.cpu().to(dtype), b.cpu().to(dtype)) for v, a, b in zip(values, s0, s1)]
    for i in range(steps):
        cur = O.optimizer_step(optimizer, [(v, g.to(dtype), a, b) for (v, a, b), g in zip(cur, grads[i])],
                               LR, 0.0, t + i)
    return cur


def _rand_state(g, N, K, pos):
    """(weight state, bias state): N(0, 1), or U(0.1, 1.1) for the non-negative accumulators."""
    if pos:
        return torch.rand(N, K, device=DEV, generator=g) + 0.1, torch.rand(N, device=DEV, generator=g) + 0.1
    return torch.randn(N, K, device=DEV, generator=g), torch.randn(N, device=DEV, generator=g)


def _shadows(N, K):
    return torch.empty(N, K, device=DEV, dtype=BF16), torch.empty(K, N, device=DEV, dtype=BF16)


# ------------------------------------------------------------------------------ Adam
@pytest.mark.parametrize("t", [1, 2, 1000])
@pytest.mark.parametrize("gather", [True, False])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_wgrad_adam(k, M, N, K, gather, t):
    g, dy, x, idx = _operands(M, N, K, gather, 11)
    w, b = torch.randn(N, K, device=DEV, generator=g), torch.randn(N, device=DEV, generator=g)
    m, bm = _rand_state(g, N, K, False)
    v, bv = _rand_state(g, N, K, True)
    w16, w16t = _shadows(N, K)
    lr = torch.full((1,), LR, device=DEV)
    step_t = torch.full((1,), t, device=DEV, dtype=torch.int32)
    ref64 = _step_ref("adam", F64, [w, b], [list(_grads(dy, x, idx, F64))], [m, bm], [v, bv], t)
    ref32 = _step_ref("adam", F32, [w, b], [list(_grads(dy, x, idx, F32))], [m, bm], [v, bv], t)
    w0, b0 = w.clone(), b.clone()
    k.lin_wgrad_adam(dy, x, idx, w, m, v, w16, w16t, b, bm, bv, lr, step_t, B1, B2, EPS)
    assert int(step_t) == t  # the weight gradient reads the counter, it never advances it
    (rw, rm, rv), (rb, rbm, rbv) = ref64
    fig = {"m": _rel(m, rm), "v": _rel(v, rv), "bm": _rel(bm, rbm), "bv": _rel(bv, rbv),
           "w16": _rel(w16, rw), "w16t": _rel(w16t, rw.t()),
           "upd": _rel(w - w0, rw - w0.cpu().double()), "bupd": _rel(b - b0, rb - b0.cpu().double())}
    bar = {"upd": max(1e-2, 4 * _rel(ref32[0][0].double() - w0.cpu().double(), rw - w0.cpu().double())),
           "bupd": max(1e-2, 4 * _rel(ref32[1][0].double() - b0.cpu().double(), rb - b0.cpu().double()))}
    print("adam M%d N%d K%d gather=%d t=%d" % (M, N, K, gather, t),
          " ".join("%s=%.2e/%.2e" % (n, f, bar.get(n, 1e-2)) for n, f in fig.items()))
    for n, f in fig.items():
        assert f < bar.get(n, 1e-2), (n, f)


def test_wgrad_adam_state_carries(k):
    """Three steps from zero state with the counter advanced on the device by xent_small."""
    M, N, K = SHAPES[1]
    g, _, x, idx = _operands(M, N, K, True, 12)
    w, b = torch.randn(N, K, device=DEV, generator=g), torch.randn(N, device=DEV, generator=g)
    m, v, bm, bv = torch.zeros_like(w), torch.zeros_like(w), torch.zeros_like(b), torch.zeros_like(b)
    w16, w16t = _shadows(N, K)
    lr = torch.full((1,), LR, device=DEV)
    step_t = torch.zeros(1, device=DEV, dtype=torch.int32)
    lg = torch.randn(8, 16, device=DEV, generator=g).to(BF16)
    lab, dl, st = torch.randint(0, 10, (8,), device=DEV, generator=g), torch.empty_like(lg), torch.zeros(2, device=DEV)
    dys = [torch.randn(M, N, device=DEV, generator=g).to(BF16) for _ in range(3)]
    g64 = [list(_grads(dy, x, idx, F64)) for dy in dys]
    g32 = [list(_grads(dy, x, idx, F32)) for dy in dys]
    gmin = min(float(t_.abs().min()) for t_ in g64[0])
    print("adam carry min|g| of step 1 = %.3e" % gmin)
    assert gmin > 1e-3  # from zero state the first update is lr * sign(g)
    ref64 = _step_ref("adam", F64, [w, b], g64, [m, bm], [v, bv], 1, steps=3)
    ref32 = _step_ref("adam", F32, [w, b], g32, [m, bm], [v, bv], 1, steps=3)
    w0, b0 = w.cpu().double(), b.cpu().double()
    for dy in dys:
        k.xent_small(lg, lab, None, dl, 10, st, step_t)
        k.lin_wgrad_adam(dy, x, idx, w, m, v, w16, w16t, b, bm, bv, lr, step_t, B1, B2, EPS)
    assert int(step_t) == 3
    (rw, rm, rv), (rb, rbm, rbv) = ref64
    fig = {"m": _rel(m, rm), "v": _rel(v, rv), "bm": _rel(bm, rbm), "bv": _rel(bv, rbv),
           "w16": _rel(w16, rw), "w16t": _rel(w16t, rw.t()),
           "upd": _rel(w.cpu().double() - w0, rw - w0), "bupd": _rel(b.cpu().double() - b0, rb - b0)}
    bar = {"upd": max(1e-2, 4 * _rel(ref32[0][0].double() - w0, rw - w0)),
           "bupd": max(1e-2, 4 * _rel(ref32[1][0].double() - b0, rb - b0))}
    print("adam carry 3 steps", " ".join("%s=%.2e/%.2e" % (n, f, bar.get(n, 1e-2)) for n, f in fig.items()))
    for n, f in fig.items():
        assert f < bar.get(n, 1e-2), (n, f)


# ------------------------------------------------------------------------------ FTRL
def _kink_keep(z_new):
    return ((z_new.abs() - L1).abs() >= KINK)


@pytest.mark.parametrize("gather", [True, False])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_wgrad_ftrl(k, M, N, K, gather):
    g, dy, x, idx = _operands(M, N, K, gather, 13)
    w, b = torch.randn(N, K, device=DEV, generator=g), torch.randn(N, device=DEV, generator=g)
    z, bz = _rand_state(g, N, K, False)
    n, bn = _rand_state(g, N, K, True)
    w16, w16t = _shadows(N, K)
    lr = torch.full((1,), LR, device=DEV)
    (rw, rz, rn), (rb, rbz, rbn) = _step_ref("ftrl", F64, [w, b], [list(_grads(dy, x, idx, F64))], [z, bz], [n, bn])
    k.lin_wgrad_ftrl(dy, x, idx, w, z, n, w16, w16t, b, bz, bn, lr, L1, FBETA, WD)
    keep, bkeep = _kink_keep(rz), _kink_keep(rbz)
    left_out = 1.0 - (int(keep.sum()) + int(bkeep.sum())) / (keep.numel() + bkeep.numel())
    wc, w16c, w16tc, bc = w.cpu(), w16.cpu(), w16t.cpu().t(), b.cpu()
    fig = {"z": _rel(z, rz), "n": _rel(n, rn), "bz": _rel(bz, rbz), "bn": _rel(bn, rbn),
           "w": _rel(wc[keep], rw[keep]), "w16": _rel(w16c[keep], rw[keep]), "w16t": _rel(w16tc[keep], rw[keep]),
           "b": _rel(bc[bkeep], rb[bkeep])}
    print("ftrl M%d N%d K%d gather=%d left out %.3f%%" % (M, N, K, gather, 100 * left_out),
          " ".join("%s=%.2e/1e-2" % (n_, f) for n_, f in fig.items()), "max|z|=%.0f" % float(rz.abs().max()))
    assert left_out <= 0.01
    for n_, f in fig.items():
        assert f < 1e-2, (n_, f)


# ------------------------------------------------------------------------------ zero rows, counter
@pytest.mark.parametrize("optimizer", ["adam", "ftrl"])
def test_zero_rows_stay_zero(k, optimizer):
    """Rows 10..15 of a padded output layer: zero gradient, zero state, zero weight - twice."""
    M, N, K = 64, 16, 128
    g, dy, x, idx = _operands(M, N, K, True, 14)
    dy[:, 10:] = 0
    w, b = torch.randn(N, K, device=DEV, generator=g), torch.randn(N, device=DEV, generator=g)
    s0, bs0 = _rand_state(g, N, K, False)
    s1, bs1 = _rand_state(g, N, K, True)
    for t_ in (w, b, s0, bs0, s1, bs1):
        t_[10:] = 0
    w16, w16t = _shadows(N, K)
    lr = torch.full((1,), LR, device=DEV)
    step_t = torch.zeros(1, device=DEV, dtype=torch.int32)
    for call in (1, 2):
        step_t.fill_(call)
        if optimizer == "adam":
            k.lin_wgrad_adam(dy, x, idx, w, s0, s1, w16, w16t, b, bs0, bs1, lr, step_t, B1, B2, EPS)
        else:
            k.lin_wgrad_ftrl(dy, x, idx, w, s0, s1, w16, w16t, b, bs0, bs1, lr, L1, FBETA, WD)
    for name, t_ in (("w", w), ("b", b), ("s0", s0), ("bs0", bs0), ("s1", s1), ("bs1", bs1), ("w16", w16)):
        assert bool(torch.isfinite(t_.float()).all()), name
        assert float(t_[10:].float().abs().max()) == 0.0, name
    assert bool(torch.isfinite(w16t.float()).all()) and float(w16t[:, 10:].float().abs().max()) == 0.0
    assert float(w[:10].abs().max()) > 0 and torch.equal(w16, w.to(BF16)) and torch.equal(w16t, w.to(BF16).t())


def test_xent_small_advances_the_counter(k):
    g = torch.Generator(device=DEV).manual_seed(15)
    M = 300  # two blocks: only thread 0 of block 0 may count
    lg = torch.randn(M, 16, device=DEV, generator=g).to(BF16)
    y = torch.randint(0, 10, (M,), device=DEV, generator=g)
    step_t = torch.zeros(1, device=DEV, dtype=torch.int32)
    for call in range(3):
        # each call into its own zeroed stats: the two blocks' atomic adds then commute exactly
        dl_a, dl_b = torch.empty_like(lg), torch.empty_like(lg)
        st_a, st_b = torch.zeros(2, device=DEV), torch.zeros(2, device=DEV)
        k.xent_small(lg, y, None, dl_a, 10, st_a, step_t)
        k.xent_small(lg, y, None, dl_b, 10, st_b)
        assert torch.equal(st_a, st_b) and torch.equal(dl_a, dl_b), call
        assert int(step_t) == call + 1
    assert int(step_t) == 3
    with pytest.raises(RuntimeError):
        k.xent_small(lg, y, None, dl_a, 10, st_a, torch.zeros(1, device=DEV, dtype=torch.int64))


# ------------------------------------------------------------------------------ model level
def _hip_layers_to_cpu(net):
    return [{n: t_.detach().cpu().clone() for n, t_ in l.items()} for l in net.layers]


@pytest.mark.parametrize("optimizer", ["sgd", "adam", "ftrl"])
@pytest.mark.parametrize("num_layers", [1, 3, 0])  # 0: the MLP module; its 784-80-40-10 keeps every width % 8 == 0
def test_hipmlp_steps_like_the_oracle(optimizer, num_layers):
    torch.manual_seed(16)
    model = mnist_mlp.MLP(80) if num_layers == 0 else mnist_mlp.DeepMLP(72, num_layers)
    net = mnist_mlp.HipMLP(model, LR, 0.9, DEV, optimizer)
    assert len(net.layers) == (3 if num_layers == 0 else num_layers + 1) and net.layers[-1]["w"].shape[0] == 16
    g = torch.Generator(device=DEV).manual_seed(17)
    x = torch.randn(300, 784, device=DEV, generator=g).to(BF16)
    y = torch.randint(0, 10, (300,), device=DEV, generator=g)
    idx = torch.randint(0, 300, (96,), device=DEV, generator=g)
    names = O.STATE[optimizer]
    for i, l in enumerate(net.layers):  # well-conditioned state; the padded output rows keep zero state
        N, K = l["w"].shape
        for wn, bn, pos in ((names[0], names[2], False), (names[1], names[3], True)):
            if wn is None:
                continue
            sw, sb = _rand_state(g, N, K, pos)
            if optimizer == "ftrl" and not pos:  # see the module docstring: keep z off the kink
                sw, sb = sw + 0.2 * torch.sign(sw), sb + 0.2 * torch.sign(sb)
            if i == len(net.layers) - 1:
                sw[10:], sb[10:] = 0, 0
            l[wn].copy_(sw)
            l[bn].copy_(sb)
    if optimizer == "adam":
        net.step_t.fill_(9)
    before = _hip_layers_to_cpu(net)
    o32, o64 = _hip_layers_to_cpu(net), _hip_layers_to_cpu(net)
    xg, yg = x[idx].cpu().float(), y[idx].cpu()
    for s in range(2):
        O.train_step(o32, xg, yg, optimizer, LR, momentum=0.9, t=10 + s, gemm_dtype=F32, round=BF16)
        O.train_step(o64, xg, yg, optimizer, LR, momentum=0.9, t=10 + s, gemm_dtype=F64, round=BF16)
    assert torch.equal(net.forward(x, idx), net.forward(x[idx].contiguous()))  # the gather inside the first GEMM
    for s in range(2):
        net.train_step(x, y, idx)
    torch.cuda.synchronize()
    if optimizer == "adam":
        assert int(net.step_t) == 11
    after = _hip_layers_to_cpu(net)
    kept = total = 0
    failures = []
    for i, (l0, l1, a, b) in enumerate(zip(before, after, o32, o64)):
        keep = {"w": torch.ones_like(l0["w"], dtype=torch.bool), "b": torch.ones_like(l0["b"], dtype=torch.bool)}
        if optimizer == "ftrl":
            keep = {"w": _kink_keep(a["z"]), "b": _kink_keep(a["bz"])}
            kept += int(keep["w"].sum()) + int(keep["b"].sum())
            total += keep["w"].numel() + keep["b"].numel()
        cmp = []  # (name, kernel, oracle fp32, oracle fp64)
        for n in [n_ for n_ in names if n_ is not None]:
            cmp.append((n, l1[n], a[n], b[n]))
        if optimizer == "ftrl":  # FTRL overwrites the weight: compare the whole of it, away from the kink
            cmp.append(("w", l1["w"][keep["w"]], a["w"][keep["w"]], b["w"][keep["w"]]))
            cmp.append(("b", l1["b"][keep["b"]], a["b"][keep["b"]], b["b"][keep["b"]]))
        else:
            cmp.append(("w upd", l1["w"] - l0["w"], a["w"] - l0["w"], b["w"] - l0["w"]))
            cmp.append(("b upd", l1["b"] - l0["b"], a["b"] - l0["b"], b["b"] - l0["b"]))
        cmp.append(("w16", l1["w16"][keep["w"]], a["w16"][keep["w"]], b["w16"][keep["w"]]))
        cmp.append(("w16t", l1["w16t"].t()[keep["w"]], a["w16"][keep["w"]], b["w16"][keep["w"]]))
        for n, got, ref32, ref64 in cmp:
            bar = max(1e-2, 4 * _rel(ref32, ref64))
            f = _rel(got, ref32)
            print("model %s L=%d layer %d %-5s %.2e/%.2e" % (optimizer, num_layers, i, n, f, bar))
            if not f < bar:
                failures.append((i, n, f, bar))
    if optimizer == "ftrl":
        print("model ftrl L=%d left out %.3f%%" % (num_layers, 100 * (1 - kept / total)))
        assert 1 - kept / total <= 0.01
    assert not failures, failures
    out = after[-1]
    for n, t_ in out.items():
        pad = t_[:, 10:] if n == "w16t" else t_[10:]
        assert float(pad.float().abs().max()) == 0.0, n
    for l in after:
        for n, t_ in l.items():
            assert bool(torch.isfinite(t_.float()).all()), n


# ------------------------------------------------------------------------------ trial level
TRIAL = ["--num-train", "20000", "--num-valid", "2000", "--epochs", "2", "--batch-size", "64", "--hidden", "256"]
EPOCH_LINE = re.compile(r"^epoch=(\d+) loss=(\S+) Validation-accuracy=(\S+) Train-accuracy=(\S+)$")


@pytest.mark.parametrize("optimizer,lr", [("sgd", "0.02"), ("adam", "0.001")])
def test_trial_hip_learns_like_module(optimizer, lr):
    common = TRIAL + ["--num-layers", "2", "--optimizer", optimizer, "--lr", lr]
    a_hip = mnist_mlp.main(common + ["--impl", "hip"])
    a_mod = mnist_mlp.main(common + ["--impl", "module"])
    print("trial %s acc hip %.4f module %.4f" % (optimizer, a_hip, a_mod))
    assert a_hip > 0.5 and abs(a_hip - a_mod) < 0.05, (a_hip, a_mod)


def _epoch_lines(out):
    return [m_ for m_ in (EPOCH_LINE.match(ln) for ln in out.splitlines()) if m_]


def test_trial_hip_ftrl_five_layers_completes(capsys):
    mnist_mlp.main(TRIAL + ["--num-layers", "5", "--optimizer", "ftrl", "--lr", "0.02", "--impl", "hip"])
    out = capsys.readouterr().out
    lines = _epoch_lines(out)
    assert [int(m_.group(1)) for m_ in lines] == [0, 1], out
    for m_ in lines:
        assert all(math.isfinite(float(m_.group(i))) for i in (2, 3, 4)), m_.group(0)


def test_trial_hip_default_net_reports_train_accuracy(capsys):
    acc = mnist_mlp.main(TRIAL + ["--lr", "0.05", "--impl", "hip"])
    out = capsys.readouterr().out
    lines = _epoch_lines(out)
    assert [int(m_.group(1)) for m_ in lines] == [0, 1], out
    assert float(lines[-1].group(3)) == pytest.approx(acc, abs=1e-5)
    assert all(0.0 < float(m_.group(4)) <= 1.0 for m_ in lines)
    assert re.search(r"^train_seconds=\S+$", out, re.M)
