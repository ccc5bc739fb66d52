"""The kernels at the two ends of the DARTS network - fused head (gap + classifier + cross-entropy)
and stem (3x3 conv + BN statistics, weight gradient through the BN backward) - against fp64 truth
computed on the GPU, at the smallest shapes that reach each of their code paths.

Tolerances are the ones tests/test_gpu_darts.py uses for these kernels
(test_fused_head_matches_torch, test_stem_conv_bn_matches_torch, test_stem_conv_vs_torch), applied
against the fp64 truth cast to fp32. Two quantities have no tolerance there:
  dl (d loss / d logits): dx = dl W / HW is linear in it, so it gets dx's 1e-4 / 1e-7.
  BN statistics (sum z, sum z^2): an fp32 conv output carries at most 27 roundings and the fp32
    wave / workgroup sums 8 more levels, 35 * 2^-24 = 2.1e-6 of the sum of the terms' magnitudes;
    the bound is 1e-5 of that magnitude sum, per channel.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


def _close(a, b, name, rtol, atol):
    b = b.to(a.dtype)
    scale = b.abs().max().item() + 1e-12
    err = (a - b).abs().max().item()
    assert err <= atol + rtol * scale, "%s: max err %.3e (scale %.3e)" % (name, err, scale)


# ------------------------------------------------------------------------------------- head
G_UP = 3.0  # upstream gradient of the loss

HEAD_SHAPES = [(3, 6, 16, 10, 3),     # B5's layout in small: node-major, HW 256, one quad per lane
               (2, 8, 10, 10, 1),     # HW 100: vector path with a partial wave
               (5, 7, 18, 4, 1),      # HW 324: more than one quad per lane, plus a tail
               (2, 5, 3, 3, 1),       # HW 9: scalar path
               (1, 1024, 2, 64, 1)]   # kMaxC and kMaxK


@functools.lru_cache(maxsize=None)
def _head_case(N, C, H, K, nodes):
    """Inputs (x as [N][C][H][H]) and the fp64 truth, computed once per shape."""
    dev = _dev()
    gen = torch.Generator(device=dev).manual_seed(1000 * N + C + H + K)
    x = torch.randn(N, C, H, H, device=dev, generator=gen)
    y = torch.randint(0, K, (N,), device=dev, generator=gen)
    w = 0.1 * torch.randn(K, C, device=dev, generator=gen)
    b = 0.1 * torch.randn(K, device=dev, generator=gen)
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    logits = F.linear(xr.mean((2, 3)), wr, br)
    loss = F.cross_entropy(logits, y)
    (G_UP * loss).backward()
    truth = dict(logits=logits.detach(), loss=float(loss.detach()), dx=xr.grad, dw=wr.grad, db=br.grad,
                 dl=(torch.softmax(logits.detach(), 1) - F.one_hot(y, K)) / N)
    return x, y, w, b, truth


def _node_major(x, nodes):
    """[N][C][H][W] -> node-major [nodes][N][C / nodes][H][W] (and back with the same call on dim 0/1)."""
    N, C, H, W = x.shape
    return x.view(N, nodes, C // nodes, H, W).transpose(0, 1).contiguous()


def _head_kernels(xk, w, b, y, with_dx=True):
    """The three bindings on ``xk`` ([N][C][H][W] or node-major 5-D) with temporary replica rows."""
    from katib_amd.ops import hip_darts as hd

    dev = xk.device
    N, (K, C) = y.shape[0], w.shape
    pooled, logits, dl = torch.empty(N, C, device=dev), torch.empty(N, K, device=dev), torch.empty(N, K, device=dev)
    loss_n, loss = torch.empty(N, device=dev), torch.empty((), device=dev)
    hd._K.head_fwd(xk, w, b, y, pooled, logits, dl, loss_n)
    hd._K.head_loss(loss_n, loss)
    off = xk.data_ptr() % 16 // 4  # dx shares the alignment of x
    dx = torch.full((xk.numel() + off,), float("nan"), device=dev)[off:].view_as(xk) if with_dx else None
    rep = torch.zeros(hd.REP, K * C + K, device=dev)
    g = torch.full((), G_UP, device=dev)
    hd._K.head_bwd(xk, dl, pooled, w, g, dx, rep[0, :K * C], K * C + K, rep[0, K * C:], K * C + K)
    grads = rep.double().sum(0)
    return dict(logits=logits, loss=float(loss), loss_n=loss_n, dl=dl, dx=dx, pooled=pooled,
                dw=grads[:K * C].view(K, C).float(), db=grads[K * C:].float())


def _check_head(got, truth, dx_truth):
    _close(got["logits"], truth["logits"], "logits", 1e-5, 1e-5)
    assert abs(got["loss"] - truth["loss"]) < 1e-5 * max(1.0, abs(truth["loss"]))
    _close(got["dl"], truth["dl"], "dl", 1e-4, 1e-7)
    _close(got["dx"], dx_truth, "dx", 1e-4, 1e-7)
    _close(got["dw"], truth["dw"], "dW", 1e-4, 1e-6)
    _close(got["db"], truth["db"], "db", 1e-4, 1e-6)


@pytest.mark.parametrize("N,C,H,K,nodes", HEAD_SHAPES)
def test_head_matches_fp64(N, C, H, K, nodes):
    x, y, w, b, truth = _head_case(N, C, H, K, nodes)
    xk = _node_major(x, nodes) if nodes > 1 else x
    dx_truth = _node_major(truth["dx"], nodes) if nodes > 1 else truth["dx"]
    got = _head_kernels(xk, w, b, y)
    _close(got["pooled"], x.double().mean((2, 3)), "pooled", 1e-5, 1e-6)
    _check_head(got, truth, dx_truth)
    # the classifier gradients alone (no dx): the kernel must not touch a feature gradient
    only = _head_kernels(xk, w, b, y, with_dx=False)
    _close(only["dw"], truth["dw"], "dW (no dx)", 1e-4, 1e-6)
    _close(only["db"], truth["db"], "db (no dx)", 1e-4, 1e-6)


def test_head_misaligned_takes_fallback():
    """x and dx one float off 16-byte alignment: the one-pixel path, same results as the aligned run."""
    N, C, H, K, nodes = HEAD_SHAPES[1]
    x, y, w, b, truth = _head_case(N, C, H, K, nodes)
    buf = torch.empty(x.numel() + 1, device=x.device)
    xo = buf[1:].view_as(x).copy_(x)
    assert xo.data_ptr() % 16 == 4 and xo.is_contiguous()
    got = _head_kernels(xo, w, b, y)
    assert got["dx"].data_ptr() % 16 == 4
    _check_head(got, truth, truth["dx"])
    ref = _head_kernels(x, w, b, y)
    _close(got["logits"], ref["logits"], "logits vs aligned", 1e-5, 1e-5)
    assert abs(got["loss"] - ref["loss"]) < 1e-5 * max(1.0, abs(ref["loss"]))
    _close(got["dx"], ref["dx"], "dx vs aligned", 1e-4, 1e-7)
    _close(got["dw"], ref["dw"], "dW vs aligned", 1e-4, 1e-6)
    _close(got["db"], ref["db"], "db vs aligned", 1e-4, 1e-6)


def test_head_registered_gradients_accumulate():
    """Gradients through a registered replicated buffer; a second forward + backward doubles them."""
    from katib_amd.ops import hip_darts as hd

    N, C, H, K, nodes = HEAD_SHAPES[2]
    x, y, w0, b0, truth = _head_case(N, C, H, K, nodes)
    dev = x.device
    rep = torch.zeros(hd.REP, K * C + K, device=dev)
    hd.register_grad_replicas(rep)
    w = w0.clone().requires_grad_(True)
    b = b0.clone().requires_grad_(True)
    w.grad = rep[0, :K * C].view(K, C)
    b.grad = rep[0, K * C:]
    for times in (1, 2):
        xh = x.clone().requires_grad_(True)
        loss, logits = hd.head_loss(xh, w, b, y)
        (G_UP * loss).backward()
        total = rep.double().sum(0)  # the replica rows, summed without folding them
        _close(total[:K * C].view(K, C).float(), times * truth["dw"], "dW x%d" % times, 1e-4, 1e-6)
        _close(total[K * C:].float(), times * truth["db"], "db x%d" % times, 1e-4, 1e-6)
        _close(xh.grad, truth["dx"], "dx", 1e-4, 1e-7)
        _close(logits, truth["logits"], "logits", 1e-5, 1e-5)
    hd.fold(rep)
    _close(rep[0, :K * C].view(K, C), 2 * truth["dw"], "folded dW", 1e-4, 1e-6)
    _close(rep[0, K * C:], 2 * truth["db"], "folded db", 1e-4, 1e-6)


def test_head_out_of_range_labels():
    """Labels -1 and K: NaN per-sample loss for those samples only, dl = softmax / N in their rows."""
    N, C, H, K, nodes = HEAD_SHAPES[2]
    x, y, w, b, truth = _head_case(N, C, H, K, nodes)
    yb = y.clone()
    yb[1], yb[3] = -1, K
    got = _head_kernels(x, w, b, yb)
    bad = torch.zeros(N, dtype=torch.bool, device=x.device)
    bad[1] = bad[3] = True
    assert torch.isnan(got["loss_n"][bad]).all()
    assert torch.isfinite(got["loss_n"][~bad]).all()
    assert torch.isfinite(got["dl"]).all() and torch.isfinite(got["logits"]).all()
    lse = torch.logsumexp(truth["logits"], 1)
    want_n = lse - truth["logits"].gather(1, y.view(-1, 1)).view(-1)
    _close(got["loss_n"][~bad], want_n[~bad], "loss_n", 1e-5, 1e-5)
    want_dl = truth["dl"].clone()
    want_dl[bad] = torch.softmax(truth["logits"], 1)[bad] / N
    _close(got["dl"], want_dl, "dl", 1e-4, 1e-7)
    _close(got["dl"][bad], want_dl[bad], "dl of the bad rows", 1e-4, 1e-7)


# ------------------------------------------------------------------------------------- stem
STEM_SHAPES = [(2, 3, 4, 8),     # B5's channel count
               (5, 3, 7, 9),     # Cout not a multiple of the channel group, odd sizes
               (3, 1, 20, 28),   # Cin 1
               (2, 3, 64, 6),    # largest Cout
               (1, 3, 4, 1)]     # every tap in the halo
MOM, EPS = 0.1, 1e-5


@functools.lru_cache(maxsize=None)
def _stem_case(N, Cin, Cout, H):
    """Inputs and the fp64 truth of conv + training BN with loss = sum(out * R), computed once per shape."""
    dev = _dev()
    gen = torch.Generator(device=dev).manual_seed(100 * N + 10 * Cout + H)
    x = torch.randn(N, Cin, H, H, device=dev, generator=gen)
    w = 0.3 * torch.randn(Cout, Cin, 3, 3, device=dev, generator=gen)
    gamma = 1.0 + 0.1 * torch.randn(Cout, device=dev, generator=gen)
    beta = 0.1 * torch.randn(Cout, device=dev, generator=gen)
    R = torch.randn(N, Cout, H, H, device=dev, generator=gen)
    M = N * H * H
    wr, gr, br = (t.double().requires_grad_(True) for t in (w, gamma, beta))
    z = F.conv2d(x.double(), wr, padding=1)
    rm, rv = torch.zeros(Cout, device=dev, dtype=torch.float64), torch.ones(Cout, device=dev, dtype=torch.float64)
    if M > 1:
        out = F.batch_norm(z, rm, rv, gr, br, True, MOM, EPS)
    else:
        # batch_norm refuses a single value per channel in training mode; this is the formula it
        # implements (biased variance; the running variance has no unbiased form for one value)
        mean, var = z.mean((0, 2, 3)), z.var((0, 2, 3), unbiased=False)
        out = (z - mean.view(1, -1, 1, 1)) * torch.rsqrt(var + EPS).view(1, -1, 1, 1) * gr.view(1, -1, 1, 1) \
            + br.view(1, -1, 1, 1)
        rm = (1 - MOM) * rm + MOM * mean.detach()
        rv = (1 - MOM) * rv + MOM * var.detach()
    (out * R.double()).sum().backward()
    # plain conv weight gradient (no BN) for the same upstream gradient
    w2 = w.double().requires_grad_(True)
    F.conv2d(x.double(), w2, padding=1).backward(R.double())
    zabs = F.conv2d(x.double().abs(), w.double().abs(), padding=1)
    zd = z.detach()
    truth = dict(z=zd, out=out.detach(), rm=rm, rv=rv, dw=wr.grad, dgamma=gr.grad, dbeta=br.grad, dw_plain=w2.grad,
                 s1=zd.sum((0, 2, 3)), s2=(zd * zd).sum((0, 2, 3)),
                 s1_mag=zabs.sum((0, 2, 3)), s2_mag=(zabs * zabs).sum((0, 2, 3)))
    return x, w, gamma, beta, R, truth


def _stem_bn_forward(x, w, gamma, beta, R):
    """stem_conv_fwd_stats + BN apply, then the BN-backward reduction: everything the weight-gradient
    kernel reads."""
    from katib_amd.ops import hip_darts as hd

    dev = x.device
    C = w.shape[0]
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    out, state = hd._stem_fwd(x, w, gamma, beta, rm, rv, MOM, EPS)
    z, zs, bn, stats = state[4], state[5], state[6], state[8]
    nred = 2 * C + 1
    red = hd.zeros64(hd.REP * nred, dev)
    hd._K.combine_bwd_reduce([(R, [zs], [bn], None, red, [0], -1, None)])
    hd._fold([(red, nred, nred)])
    return dict(out=out, z=z, stats=stats, red=red, rm=rm, rv=rv)


def _stem_bn_wgrad(x, w, gamma, R, fwd, accumulate, dw0, dg0, db0):
    """stem_conv_wgrad_bn into gradient buffers that start at dw0 / dg0 / db0."""
    from katib_amd.ops import hip_darts as hd

    partial = torch.empty(hd.stem_chunks(x, w.shape[0]), w.numel(), device=x.device)
    dw, dg, db = dw0.clone(), dg0.clone(), db0.clone()
    hd._K.stem_conv_wgrad_bn(x, R, fwd["z"], fwd["red"], fwd["stats"], gamma, EPS, dg, db, partial, dw, 1, accumulate)
    return dw, dg, db


@pytest.mark.parametrize("N,Cin,Cout,H", STEM_SHAPES)
def test_stem_bn_matches_fp64(N, Cin, Cout, H):
    x, w, gamma, beta, R, t = _stem_case(N, Cin, Cout, H)
    gen = torch.Generator(device=x.device).manual_seed(7)
    dw0 = torch.randn(w.shape, device=x.device, generator=gen)
    dg0 = torch.randn(Cout, device=x.device, generator=gen)
    db0 = torch.randn(Cout, device=x.device, generator=gen)
    fwd = _stem_bn_forward(x, w, gamma, beta, R)
    _close(fwd["z"], t["z"], "conv", 1e-4, 1e-5)
    _close(fwd["out"], t["out"], "out", 1e-4, 1e-5)
    s1, s2 = fwd["stats"][:Cout], fwd["stats"][Cout:2 * Cout]
    assert ((s1 - t["s1"]).abs() <= 1e-5 * t["s1_mag"]).all(), "sum z: %s vs %s" % (s1, t["s1"])
    assert ((s2 - t["s2"]).abs() <= 1e-5 * t["s2_mag"]).all(), "sum z^2: %s vs %s" % (s2, t["s2"])
    _close(fwd["rm"], t["rm"], "running_mean", 1e-5, 1e-6)
    _close(fwd["rv"], t["rv"], "running_var", 1e-5, 1e-6)
    runs = {}
    for accumulate in (False, True):
        dw, dg, db = runs[accumulate] = _stem_bn_wgrad(x, w, gamma, R, fwd, accumulate, dw0, dg0, db0)
        # d gamma / d beta always add to their rows; dW adds only with accumulate
        _close(dw - (dw0 if accumulate else 0), t["dw"], "dW accumulate=%s" % accumulate, 1e-3, 1e-4)
        _close(dg - dg0, t["dgamma"], "dgamma", 1e-4, 1e-4)
        _close(db - db0, t["dbeta"], "dbeta", 1e-4, 1e-4)
    # the same inputs (the statistics themselves come from float atomics) give the same bits
    for accumulate in (False, True):
        again = _stem_bn_wgrad(x, w, gamma, R, fwd, accumulate, dw0, dg0, db0)
        assert torch.equal(again[0], runs[accumulate][0]), "weight gradient differs between two runs"


@pytest.mark.parametrize("N,Cin,Cout,H", STEM_SHAPES)
def test_stem_plain_matches_fp64(N, Cin, Cout, H):
    """stem_conv_fwd (the validation forward) and stem_conv_wgrad without BN."""
    from katib_amd.ops import hip_darts as hd

    x, w, _, _, R, t = _stem_case(N, Cin, Cout, H)
    assert hd.stem_supported(x, w)
    w1 = w.clone().requires_grad_(True)
    y = hd.stem_conv(x, w1)
    y.backward(R)
    _close(y.detach(), t["z"], "conv", 1e-4, 1e-5)
    torch.testing.assert_close(w1.grad, t["dw_plain"].float(), rtol=1e-4, atol=1e-3 * (N * H * H) ** 0.5)
    w2 = w.clone().requires_grad_(True)
    hd.stem_conv(x, w2).backward(R)
    assert torch.equal(w1.grad, w2.grad), "weight gradient differs between two runs"
