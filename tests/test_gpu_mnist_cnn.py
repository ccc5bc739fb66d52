"""The MNIST CNN trial on the fused kernels of csrc/hip/mnist_cnn.hip (+ csrc/hip/mlp.hip for fc1 / fc2):
each kernel through its binding against tests/mnist_cnn_oracle.py, ``HipCNN`` over three steps through
``state_dict()``, eager against a replayed graph, and the trial's ``--impl hip``.

B is the only free size: O.BATCHES = 1, 3 (with a repeated gather index), 17 and 65 (see the oracle file).

Exact arm. Small-integer / power-of-two operands (O.exact_case), so every sum is exact in fp32 in any
order (tests/test_mnist_cnn_oracle.py proves that on the reference): p1, p2, the winners, dp1, the
pre-SGD gradients (the momentum buffer after a step from zero momentum) and, with lr = 2^-10, the new
masters and shadows are compared with torch.equal. Ties abound there, and the filters are asymmetric.

Generic arm. Gaussian images, ``Net``'s initialisation. Every output is held, against the oracle with
fp32 GEMMs, to the larger of 1e-2 relative (max norm) and four times that oracle's own distance from the
oracle with fp64 GEMMs at the same rounding points (the rule of tests/test_gpu_mlp_optim.py). Every
kernel gets the fp32 oracle's rounded outputs as inputs, so the arms differ by accumulation alone. A
pooled element whose window is a near tie (O.near_tie) is left out of the value and winner comparisons,
never of the padding checks; at most 1 % may be (the CPU file counts them on the reference: none).
Momentum and shadows: 1e-2. Model level: the same rule on momentum and update of every parameter.

Every test prints the figures it measured (``pytest -s``) before it asserts.
"""
import math
import re

import pytest
import torch

import mnist_cnn_oracle as O
from katib_amd.workloads import mnist_cnn
from katib_amd.workloads.common import CapturedStep

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
EXACT_LR = 2.0 ** -10


@pytest.fixture(scope="module")
def k():
    from katib_amd.ops.conv import kernels

    return kernels()


def _lr(v):
    return torch.full((1,), v, device=DEV, dtype=F32)


def _packed(w1, b1, w2, b2):
    """Kernel-layout masters and shadows on the device from conv tensors in torch's layout."""
    sd = {n: t.clone() for n, t in mnist_cnn.Net().state_dict().items()}
    sd.update({"conv1.weight": w1, "conv1.bias": b1, "conv2.weight": w2, "conv2.bias": b2})
    P = mnist_cnn.pack_state(sd, DEV)
    return (P,) + mnist_cnn.conv_shadows(P["conv1.weight"], P["conv2.weight"])


def _w1_torch(t):  # [24][25] -> ([20, 1, 5, 5], pad rows)
    return t[:20].reshape(20, 1, 5, 5).cpu(), t[20:].cpu()


def _w2_torch(t):  # [50][600] -> ([50, 20, 5, 5], pad channels)
    v = t.view(50, 5, 5, 24).cpu()
    return v[..., :20].permute(0, 3, 1, 2).contiguous(), v[..., 20:]


def _zero(*ts):
    return all(float(t.float().abs().max()) == 0.0 for t in ts if t.numel())


def _fwd1(k, x, idx, w1s, b1, B, save=True):
    p1 = torch.empty(B, 12, 12, 24, device=DEV, dtype=BF16)
    a1 = torch.empty(B, 12, 12, 24, device=DEV, dtype=torch.uint8) if save else None
    k.cnn_conv1_pool_fwd(x, idx, w1s, b1, p1, a1)
    return p1, a1


def _fwd2(k, p1, w2f, b2, B, save=True):
    p2 = torch.empty(B, 800, device=DEV, dtype=BF16)
    a2 = torch.empty(B, 800, device=DEV, dtype=torch.uint8) if save else None
    k.cnn_conv2_pool_fwd(p1, w2f, b2, p2, a2)
    return p2, a2


def _wgrad2(k, dp2, a2, p1, P, M, w2f, w2d, lr, mom, B):
    part = torch.empty(k.cnn_part_sizes(B)[1], device=DEV, dtype=F32)
    k.cnn_conv2_wgrad_sgd(dp2, a2, p1, part, P["conv2.weight"], M["conv2.weight"], P["conv2.bias"],
                          M["conv2.bias"], w2f, w2d, lr, mom)


def _wgrad1(k, dp1, a1, x, idx, P, M, w1s, lr, mom, B):
    part = torch.empty(k.cnn_part_sizes(B)[0], device=DEV, dtype=F32)
    k.cnn_conv1_wgrad_sgd(dp1, a1, x, idx, part, P["conv1.weight"], M["conv1.weight"], P["conv1.bias"],
                          M["conv1.bias"], w1s, lr, mom)


# ------------------------------------------------------------------------------ exact arm
@pytest.mark.parametrize("B", O.BATCHES)
def test_kernels_exact(k, B):
    c = O.exact_case(B, 20 + B)
    P, w1s, w2f, w2d = _packed(c["w1"], c["b1"], c["w2"], c["b2"])
    M = {n: torch.zeros_like(t) for n, t in P.items()}
    x = c["x"].view(O.ROWS, 784).to(DEV, BF16)
    idx = c["idx"].to(DEV)
    xg = c["x"][c["idx"]]
    if B == 3:
        assert int(idx[0]) == int(idx[1])
    bad = []

    # conv1 forward, gathered
    rp1, ra1, _ = O.conv_pool_fwd(xg, c["w1"], c["b1"], F32, BF16)
    p1k, a1k = _fwd1(k, x, idx, w1s, P["conv1.bias"], B)
    gp1, pad_p1 = O.from_nhwc(p1k.cpu().float(), 20)
    ga1, pad_a1 = O.from_nhwc(a1k.cpu().long(), 20)
    bad += O.exact_mismatches({"p1": gp1, "a1": ga1}, {"p1": rp1, "a1": ra1}, ["p1", "a1"])
    assert _zero(pad_p1, pad_a1)
    p1n, _ = _fwd1(k, x[c["idx"]].contiguous(), None, w1s, P["conv1.bias"], B, save=False)
    assert torch.equal(p1n, p1k)  # no gather, no winners: the same values
    print("B=%d conv1: winners by position %s" % (B, torch.bincount(ra1.flatten(), minlength=4).tolist()))

    # conv2 forward on a drawn p1
    p1d = O.nhwc_pad(c["p1"], 24, BF16).to(DEV)
    rp2, ra2, _ = O.conv_pool_fwd(c["p1"], c["w2"], c["b2"], F32, BF16)
    p2k, a2k = _fwd2(k, p1d, w2f, P["conv2.bias"], B)
    bad += O.exact_mismatches({"p2": O.from_p2_rows(p2k.cpu().float()), "a2": O.from_p2_rows(a2k.cpu().long())},
                              {"p2": rp2, "a2": ra2}, ["p2", "a2"])
    assert torch.equal(_fwd2(k, p1d, w2f, P["conv2.bias"], B, save=False)[0], p2k)
    print("B=%d conv2: winners by position %s, max |p2| %.0f" % (
        B, torch.bincount(ra2.flatten(), minlength=4).tolist(), float(rp2.abs().max())))

    # conv2 data gradient
    dp2 = O.p2_rows(c["dp2"], BF16).to(DEV)
    a2 = O.p2_rows(ra2, torch.uint8).to(DEV)
    rdp1 = O.conv_dgrad(c["dp2"], ra2, c["w2"], c["p1"], F32, BF16)
    dp1k = torch.empty(B, 12, 12, 24, device=DEV, dtype=BF16)
    k.cnn_conv2_dgrad(dp2, a2, w2d, p1d, dp1k)
    gdp1, pad_dp1 = O.from_nhwc(dp1k.cpu().float(), 20)
    bad += O.exact_mismatches({"dp1": gdp1}, {"dp1": rdp1}, ["dp1"])
    assert _zero(pad_dp1)

    # conv2 weight gradient + SGD from zero momentum: the buffer is the gradient
    rg2w, rg2b = O.conv_wgrad(c["dp2"], ra2, c["p1"], F32, BF16)
    (rw2, _), (rb2, _) = O.sgd_step([(c["w2"], rg2w, torch.zeros_like(rg2w)), (c["b2"], rg2b, torch.zeros_like(rg2b))],
                                    EXACT_LR, 0.5)
    _wgrad2(k, dp2, a2, p1d, P, M, w2f, w2d, _lr(EXACT_LR), 0.5, B)
    g2w, pad_g2 = _w2_torch(M["conv2.weight"])
    n2w, pad_n2 = _w2_torch(P["conv2.weight"])
    got = {"g.conv2.weight": g2w, "g.conv2.bias": M["conv2.bias"].cpu(), "conv2.weight": n2w,
           "conv2.bias": P["conv2.bias"].cpu()}
    ref = {"g.conv2.weight": rg2w, "g.conv2.bias": rg2b, "conv2.weight": rw2, "conv2.bias": rb2}
    bad += O.exact_mismatches(got, ref, list(ref))
    assert _zero(pad_g2, pad_n2)
    _, ew2f, ew2d = mnist_cnn.conv_shadows(P["conv1.weight"], P["conv2.weight"])
    assert torch.equal(w2f, ew2f) and torch.equal(w2d, ew2d)  # both shadows: the new master, rounded; pads zero

    # conv1 weight gradient + SGD
    dp1 = O.nhwc_pad(c["dp1"], 24, BF16).to(DEV)
    a1 = O.nhwc_pad(ra1, 24, torch.uint8).to(DEV)
    rg1w, rg1b = O.conv_wgrad(c["dp1"], ra1, xg, F32, BF16)
    (rw1, _), (rb1, _) = O.sgd_step([(c["w1"], rg1w, torch.zeros_like(rg1w)), (c["b1"], rg1b, torch.zeros_like(rg1b))],
                                    EXACT_LR, 0.5)
    _wgrad1(k, dp1, a1, x, idx, P, M, w1s, _lr(EXACT_LR), 0.5, B)
    g1w, pad_g1 = _w1_torch(M["conv1.weight"])
    n1w, pad_n1 = _w1_torch(P["conv1.weight"])
    got = {"g.conv1.weight": g1w, "g.conv1.bias": M["conv1.bias"][:20].cpu(), "conv1.weight": n1w,
           "conv1.bias": P["conv1.bias"][:20].cpu()}
    ref = {"g.conv1.weight": rg1w, "g.conv1.bias": rg1b, "conv1.weight": rw1, "conv1.bias": rb1}
    bad += O.exact_mismatches(got, ref, list(ref))
    assert _zero(pad_g1, pad_n1, M["conv1.bias"][20:], P["conv1.bias"][20:])
    assert torch.equal(w1s, mnist_cnn.conv_shadows(P["conv1.weight"], P["conv2.weight"])[0])
    print("B=%d exact arm: max |dW2| %.0f, max |dW1| %.0f, mismatches %s" % (
        B, float(rg2w.abs().max()), float(rg1w.abs().max()), bad))
    assert bad == []


# ------------------------------------------------------------------------------ generic arm
def _held(name, got, r32, r64, floor=1e-2, keep=None):
    if keep is not None:
        got, r32, r64 = got[keep], r32[keep], r64[keep]
    bar, fig = max(floor, 4 * O.rel(r32, r64)), O.rel(got, r32)
    print("  %-22s %.2e/%.2e" % (name, fig, bar))
    return [] if fig < bar else [(name, fig, bar)]


@pytest.mark.parametrize("B", O.BATCHES)
def test_kernels_generic(k, B):
    x, y, idx, net = O.generic_case(B, 40 + B)
    p, _ = O.state_from_module(net)
    g = torch.Generator().manual_seed(90 + B)
    msd = {n: 0.01 * torch.randn(t.shape, generator=g) for n, t in p.items()}  # a momentum state to carry
    P, w1s, w2f, w2d = _packed(p["conv1.weight"], p["conv1.bias"], p["conv2.weight"], p["conv2.bias"])
    M = mnist_cnn.pack_state(msd, DEV)
    xd, idxd, xg = x.view(O.ROWS, 784).to(DEV, BF16), idx.to(DEV), x[idx]
    print("B=%d generic arm (figure/bar)" % B)
    fails = []

    # conv1 / conv2 forward
    p1_32, a1_32, z32 = O.conv_pool_fwd(xg, p["conv1.weight"], p["conv1.bias"], F32, BF16)
    p1_64, a1_64, z64 = O.conv_pool_fwd(xg, p["conv1.weight"], p["conv1.bias"], F64, BF16)
    near1, err1 = O.near_tie(z32, z64)
    p1k, a1k = _fwd1(k, xd, idxd, w1s, P["conv1.bias"], B)
    gp1, pad_p1 = O.from_nhwc(p1k.cpu().float(), 20)
    ga1, pad_a1 = O.from_nhwc(a1k.cpu().long(), 20)
    fails += _held("p1", gp1, p1_32, p1_64, keep=~near1)
    p1d = O.nhwc_pad(p1_32, 24, BF16).to(DEV)
    p2_32, a2_32, v32 = O.conv_pool_fwd(p1_32, p["conv2.weight"], p["conv2.bias"], F32, BF16)
    p2_64, a2_64, v64 = O.conv_pool_fwd(p1_32, p["conv2.weight"], p["conv2.bias"], F64, BF16)
    near2, err2 = O.near_tie(v32, v64)
    p2k, a2k = _fwd2(k, p1d, w2f, P["conv2.bias"], B)
    gp2, ga2 = O.from_p2_rows(p2k.cpu().float()), O.from_p2_rows(a2k.cpu().long())
    fails += _held("p2", gp2, p2_32, p2_64, keep=~near2)
    wrong1 = int((ga1 != a1_64)[~near1].sum())
    wrong2 = int((ga2 != a2_64)[~near2].sum())
    s1, s2 = float(near1.float().mean()), float(near2.float().mean())
    print("  near ties left out: conv1 %.4f%% (err %.1e) conv2 %.4f%% (err %.1e); winners off: %d, %d" % (
        100 * s1, err1, 100 * s2, err2, wrong1, wrong2))
    assert s1 <= 0.01 and s2 <= 0.01
    assert wrong1 == 0 and wrong2 == 0
    assert _zero(pad_p1, pad_a1)

    # conv2 data gradient: a pooled gradient of the model's size, masked as fc1's dgrad leaves it
    dp2 = ((0.1 * torch.randn(p2_32.shape, generator=g)) * (p2_32 > 0)).to(BF16).float()
    dp2d, a2d = O.p2_rows(dp2, BF16).to(DEV), O.p2_rows(a2_32, torch.uint8).to(DEV)
    d32 = O.conv_dgrad(dp2, a2_32, p["conv2.weight"], p1_32, F32, BF16)
    d64 = O.conv_dgrad(dp2, a2_32, p["conv2.weight"], p1_32, F64, BF16)
    dp1k = torch.empty(B, 12, 12, 24, device=DEV, dtype=BF16)
    k.cnn_conv2_dgrad(dp2d, a2d, w2d, p1d, dp1k)
    gdp1, pad_dp1 = O.from_nhwc(dp1k.cpu().float(), 20)
    fails += _held("dp1", gdp1, d32, d64)
    assert _zero(pad_dp1)
    assert _zero(gdp1[p1_32 <= 0])  # the ReLU mask is exact

    # weight gradients + SGD on a carried momentum state
    def ref_update(name, gd, dp, win, inp):
        gw, gb = O.conv_wgrad(dp, win, inp, gd, BF16)
        return O.sgd_step([(p[name + ".weight"], gw.float(), msd[name + ".weight"]),
                           (p[name + ".bias"], gb.float(), msd[name + ".bias"])], O.LR, O.MOMENTUM)

    lr = _lr(O.LR)
    (w32, m32), (b32, bm32) = ref_update("conv2", F32, dp2, a2_32, p1_32)
    (w64, m64), (b64, bm64) = ref_update("conv2", F64, dp2, a2_32, p1_32)
    _wgrad2(k, dp2d, a2d, p1d, P, M, w2f, w2d, lr, O.MOMENTUM, B)
    gw, pad_w = _w2_torch(P["conv2.weight"])
    gm, pad_m = _w2_torch(M["conv2.weight"])
    w0, b0 = p["conv2.weight"], p["conv2.bias"]
    fails += _held("conv2 momentum", gm, m32, m64) + _held("conv2 bias momentum", M["conv2.bias"].cpu(), bm32, bm64)
    fails += _held("conv2 upd", gw - w0, w32 - w0, w64 - w0) + _held("conv2 bias upd", P["conv2.bias"].cpu() - b0, b32 - b0, b64 - b0)
    sf, _ = _w2_torch(w2f[:50, :600].float().contiguous())
    sdg, _ = _w2_torch(w2d[:, :, :50].permute(2, 1, 0).float().contiguous())
    fails += _held("w2f shadow", sf, w32.to(BF16).float(), w64.to(BF16).float())
    fails += _held("w2d shadow", sdg, w32.to(BF16).float(), w64.to(BF16).float())
    assert _zero(pad_w, pad_m, w2f[50:], w2f[:, 600:], w2d[:, :, 50:], w2d[20:],
                 w2f[:50, :600].view(50, 25, 24)[:, :, 20:])

    dp1 = d32
    dp1d, a1d = O.nhwc_pad(dp1, 24, BF16).to(DEV), O.nhwc_pad(a1_32, 24, torch.uint8).to(DEV)
    (w32, m32), (b32, bm32) = ref_update("conv1", F32, dp1, a1_32, xg)
    (w64, m64), (b64, bm64) = ref_update("conv1", F64, dp1, a1_32, xg)
    _wgrad1(k, dp1d, a1d, xd, idxd, P, M, w1s, lr, O.MOMENTUM, B)
    gw, pad_w = _w1_torch(P["conv1.weight"])
    gm, pad_m = _w1_torch(M["conv1.weight"])
    w0, b0 = p["conv1.weight"], p["conv1.bias"]
    fails += _held("conv1 momentum", gm, m32, m64) + _held("conv1 bias momentum", M["conv1.bias"][:20].cpu(), bm32, bm64)
    fails += _held("conv1 upd", gw - w0, w32 - w0, w64 - w0)
    fails += _held("conv1 bias upd", P["conv1.bias"][:20].cpu() - b0, b32 - b0, b64 - b0)
    s1w, pad_s = _w1_torch(w1s.t().float().contiguous())
    fails += _held("w1s shadow", s1w, w32.to(BF16).float(), w64.to(BF16).float())
    assert _zero(pad_w, pad_m, pad_s, P["conv1.bias"][20:], M["conv1.bias"][20:])
    assert fails == []


# ------------------------------------------------------------------------------ model level
def _pads_zero(net):
    p, m = net.p, net.m
    for d in (p, m):
        assert _zero(d["conv1.weight"][20:], d["conv1.bias"][20:], d["conv2.weight"].view(50, 25, 24)[:, :, 20:],
                     d["fc1.weight"][500:], d["fc1.bias"][500:], d["fc2.weight"][10:], d["fc2.weight"][:, 500:],
                     d["fc2.bias"][10:])
    f1, f2 = net.fc
    assert _zero(net.w1s[:, 20:], net.w2f[50:], net.w2f[:, 600:], net.w2f[:50, :600].view(50, 25, 24)[:, :, 20:],
                 net.w2d[20:], net.w2d[:, :, 50:], f1["w16"][500:], f1["w16t"][:, 500:], f2["w16"][10:],
                 f2["w16"][:, 500:], f2["w16t"][:, 10:], f2["w16t"][500:])


def _cpu(sd):
    return {n: t.detach().cpu().clone() for n, t in sd.items()}


def test_hipcnn_steps_like_the_oracle_eager_and_replayed():
    x, y, idx, net = O.generic_case(17, 3)
    xg, yg = x[idx], y[idx]
    before = O.state_dict(*O.state_from_module(net))
    refs, losses = [], []
    for gd in (F32, F64):
        p, m = O.state_from_module(net)
        losses.append(sum(O.train_step(p, m, xg, yg, O.LR, O.MOMENTUM, gd, BF16)["loss"] for _ in range(O.STEPS)))
        refs.append(O.state_dict(p, m))
    xd, yd, idxd = x.view(O.ROWS, 784).to(DEV, BF16), y.to(DEV), idx.to(DEV)

    def run(captured):
        hip = mnist_cnn.HipCNN(net, O.LR, O.MOMENTUM, DEV)
        step = CapturedStep(lambda: hip.train_step(xd, yd, idxd), enabled=captured, warmup=0)
        for _ in range(O.STEPS):
            step()
        torch.cuda.synchronize()
        assert (step.graph is not None) == captured
        return hip, _cpu(hip.state_dict()), hip.stats.cpu()

    hip, got, stats = run(False)
    assert set(got) == set(refs[0]) and all(got[n].shape == refs[0][n].shape and got[n].dtype == F32 for n in got)
    loss_bar = max(1e-2, 4 * abs(losses[0] - losses[1]) / losses[1])
    print("summed loss hip %.5f oracle fp32 %.5f fp64 %.5f; correct %d" % (float(stats[0]), losses[0], losses[1], int(stats[1])))
    fails = O.state_failures(got, refs[0], refs[1], before, "model")
    assert fails == []
    assert abs(float(stats[0]) - losses[0]) / losses[0] < loss_bar
    _pads_zero(hip)
    for n, t in got.items():
        assert bool(torch.isfinite(t).all()), n
    _, again, stats2 = run(False)
    hip_g, replayed, stats3 = run(True)
    for n in got:
        assert torch.equal(got[n], again[n]), ("second eager run", n)
        assert torch.equal(got[n], replayed[n]), ("replayed", n)
    assert torch.equal(stats, stats2) and torch.equal(stats, stats3)
    _pads_zero(hip_g)


def test_forward_of_a_batch_equals_the_rows_alone():
    x, y, idx, net = O.generic_case(1, 7)
    g = torch.Generator().manual_seed(8)
    x70 = torch.randn(70, 784, generator=g).to(DEV, BF16)
    hip = mnist_cnn.HipCNN(net, O.LR, O.MOMENTUM, DEV)
    whole = hip.forward(x70)
    rows = torch.cat([hip.forward(x70[i:i + 1]) for i in range(70)])
    gathered = hip.forward(x70, torch.arange(69, -1, -1, device=DEV)).flip(0)
    ref = net(x70.float().cpu().view(70, 1, 28, 28)).detach()
    got = whole[:, :10].float().log_softmax(1).cpu()
    print("forward B=70: log-softmax against the fp32 module %.2e; padded logits max %.1f" % (
        O.rel(got, ref), float(whole[:, 10:].float().abs().max())))
    assert whole.shape == (70, 16) and whole.dtype == BF16
    assert torch.equal(whole, rows) and torch.equal(whole, gathered)
    assert _zero(whole[:, 10:])
    assert O.rel(got, ref) < 5e-2  # bf16 operands against fp32: a plumbing bound, the numerics are held above


# ------------------------------------------------------------------------------ trial level
METRIC = re.compile(r"^\{metricName: accuracy, metricValue: (\d\.\d{4})\};\{metricName: loss, metricValue: (\S+)\}$", re.M)
TRAIN = re.compile(r"^Train Epoch: 1 \[(\d+)/1280 \((\d+)%\)\]\tloss=(\S+)$", re.M)


def test_trial_hip_prints_the_metric_lines_and_learns(capsys):
    common = ["--epochs", "1", "--num-train", "1280", "--num-test", "500", "--batch-size", "64",
              "--test-batch-size", "200", "--lr", "0.05", "--momentum", "0.9", "--log-interval", "5"]
    a_hip = mnist_cnn.main(common + ["--impl", "hip"])
    out_hip = capsys.readouterr().out
    a_mod = mnist_cnn.main(common + ["--impl", "module"])
    out_mod = capsys.readouterr().out
    print(out_hip)
    print("trial accuracy hip %.4f module %.4f (chance 0.1)" % (a_hip, a_mod))
    mh, mm = METRIC.search(out_hip), METRIC.search(out_mod)
    assert mh and mm, out_hip
    assert math.isfinite(float(mh.group(2))) and abs(float(mh.group(1)) - a_hip) < 1e-4
    th, tm = TRAIN.findall(out_hip), TRAIN.findall(out_mod)
    assert [t[:2] for t in th] == [t[:2] for t in tm] and len(th) == 4
    assert all(math.isfinite(float(t[2])) for t in th)
    assert abs(float(th[0][2]) - float(tm[0][2])) < 0.05  # the first batch, before any update: the same loss
    assert a_hip >= 0.1 + 0.5 * (a_mod - 0.1), (a_hip, a_mod)
