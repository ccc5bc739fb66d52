"""The fused separable convolution (``csrc/hip/enas_sepconv.hip``) against ``ops.enas_sepconv.reference``:
TRUTH is the reference in fp64 with no intermediate rounding, REF the reference in fp32 with the kernels'
bf16 roundings (both on the CPU); every row of every output within 4 times REF's own worst row error, at
least one ulp, at the smallest shapes at which each path of the kernels can go wrong."""
import functools

import pytest
import torch

import gpt2_kernel_oracle as O

gpu = pytest.mark.gpu
MARGINS = {}  # output name -> derived margin; empty: every output is held to the project's 4
SHAPES = [(2, 5, 5, 8, 1, 3, 1, 16),      # one chunk, map smaller than a band, halo on every side
          (2, 7, 9, 8, 2, 5, 2, 32),      # non-square, dm = 2, stride 2 with odd sizes
          (2, 8, 8, 16, 1, 3, 2, 16),     # even size at stride 2: the asymmetric 'same' pad
          (1, 6, 6, 72, 1, 7, 1, 48),     # kernel wider than the map, ragged second chunk, three column blocks
          (3, 32, 32, 16, 1, 3, 1, 128),  # several bands per image and per backward workgroup, largest F
          (2, 16, 16, 136, 2, 3, 1, 64),  # Cd = 272, five chunks
          (1, 16, 16, 8, 1, 7, 1, 16)]    # a 14 x 22 patch: more vectors than the prefetch registers hold
NAMES = ("y", "gx", "gwd", "gwp", "gb")


def _signed(gen, *shape):  # no zeros, no zero mean: one sign per (sample, channel)
    return (torch.rand(*shape, generator=gen) + 0.25) * (torch.randint(0, 2, shape[:2] + (1, 1), generator=gen) * 2 - 1)


@functools.lru_cache(maxsize=None)
def _case(shape, bias):
    """Seeded bf16-valued inputs, and the TRUTH and REF arms as rows: (inputs, truth, ref), computed once."""
    from katib_amd.ops.enas_sepconv import reference, round_bf16

    N, H, W, C, dm, K, S, F = shape
    gen = torch.Generator().manual_seed(sum(shape) * 1000 + C)
    x = _signed(gen, N, C, H, W).to(torch.bfloat16).float()
    wd = torch.randn(C * dm, 1, K, K, generator=gen) * 0.3
    wp = (torch.randn(F, C * dm, 1, 1, generator=gen) * 0.2).to(torch.bfloat16).float()
    b = torch.randn(F, generator=gen) if bias else None
    gy = _signed(gen, N, F, -(-H // S), -(-W // S)).to(torch.bfloat16).float()

    def arm(dtype, rounding):
        leaves = [t.to(dtype, copy=True).requires_grad_(True) for t in (x, wd, wp) + ((b,) if bias else ())]
        y = reference(*leaves, *(() if bias else (None,)), S, dm, rounding)
        return _rows(shape, y.detach(), *torch.autograd.grad(y, leaves, gy.to(dtype)))

    return (x, wd, wp, b, gy), arm(torch.float64, None), arm(torch.float32, round_bf16)


def _rows(shape, y, gx, gwd, gwp, gb=None):
    N, H, W, C, dm, K, S, F = shape
    out = {"y": y.permute(0, 2, 3, 1).reshape(-1, F), "gwd": gwd.reshape(C * dm, K * K), "gwp": gwp.reshape(F, C * dm)}
    if gx is not None:
        out["gx"] = gx.permute(0, 2, 3, 1).reshape(-1, C)
    if gb is not None:
        out["gb"] = gb[None]
    return out


def _run(shape, bias, xg=True):
    """The fused Function on the GPU from the case's inputs -> rows like the arms'."""
    from katib_amd.ops import enas_sepconv as hs

    dev = torch.device("cuda", 0)
    x, wd, wp, b, gy = (t.to(dev) if t is not None else None for t in _case(shape, bias)[0])
    x = x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last).requires_grad_(xg)
    leaves = [t.requires_grad_(True) for t in (wd, wp) + ((b,) if bias else ())]
    assert hs.supported(x, wd, wp, shape[6])
    y = hs.separable_same(x, wd, wp, b, shape[6])
    y.backward(gy.to(torch.bfloat16))
    return _rows(shape, y.detach(), x.grad, *(t.grad for t in leaves))


def _check(got, shape, bias, names=NAMES):
    _, truth, ref = _case(shape, bias)
    for name in names:
        if name in got:
            O.assert_rows_close(got[name].cpu(), ref[name], truth[name], margin=MARGINS.get(name, O.DEFAULT_MARGIN),
                                what="%s %s" % (name, "x".join(map(str, shape))))


@gpu
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_and_backward_against_fp64(shape, bias):
    got = _run(shape, bias)
    assert set(got) == set(NAMES) - (set() if bias else {"gb"})
    _check(got, shape, bias)


@gpu
def test_bits_and_skipped_gradients():
    """Two runs from one state agree in every bit of y, gx and the depthwise weight gradient (gd and the
    depthwise partials have no atomics). gwp is summed by fp32 atomic adds, whose order is free: it is
    only held to the rule of the first test, here as there."""
    from katib_amd.ops import enas_sepconv as hs
    from katib_amd.ops.enas_optim import ChildAdam
    from katib_amd.workloads.enas_child import Op

    shape = SHAPES[4]
    one, two, nox = _run(shape, True), _run(shape, True), _run(shape, True, xg=False)
    assert all(torch.equal(one[k], two[k]) for k in ("y", "gx", "gwd", "gb"))
    _check(two, shape, True, ("gwp",))
    assert "gx" not in nox and torch.equal(nox["gwd"], one["gwd"]) and torch.equal(nox["y"], one["y"])
    _check(nox, shape, True, ("gwp",))
    # the ChildAdam records: images read from, gradients written into, the optimizer's buffers
    dev = torch.device("cuda", 0)
    x, wd, wp, b, gy = (t.to(dev) for t in _case(shape, True)[0])
    op = Op({"opt_type": "separable_convolution", "num_filter": 128}, 16, 32, sep="fused").to(dev)
    with torch.no_grad():
        op.body[0].conv.weight.copy_(wd), op.body[1].weight.copy_(wp), op.body[1].bias.copy_(b)
    opt = ChildAdam(op)
    dw, pw = op.body[0], op.body[1]
    x = x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = hs.separable_same(x, dw.conv.weight, pw.weight, pw.bias, 1, dw.prep, pw.prep)
    y.backward(gy.to(torch.bfloat16))
    g = opt.grads()
    assert dw.conv.weight.grad is None and pw.weight.grad is None
    assert torch.equal(y.detach().permute(0, 2, 3, 1).reshape(-1, 128), one["y"])
    _check(_rows(shape, y.detach(), x.grad, g["body.0.conv.weight"], g["body.1.weight"], g["body.1.bias"]), shape, True)


ARCH = [[0], [1, 1], [2, 0, 0]]  # separable k3 s1; separable k5 s2 dm 2 on layer 1 and the input; convolution
CFG = {"num_layers": 3, "input_sizes": [8, 16, 16], "output_sizes": [10], "embedding": {
    "0": {"opt_type": "separable_convolution", "num_filter": 16, "filter_size": 3, "stride": 1},
    "1": {"opt_type": "separable_convolution", "num_filter": 32, "filter_size": 5, "stride": 2, "depth_multiplier": 2},
    "2": {"opt_type": "convolution", "num_filter": 16, "filter_size": 3, "stride": 1}}}


def _net_grads(net, x, gl, dtype=None):
    net.train()
    net.drop.p = 0.0  # the three nets must compute the same function
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype is None):
        logits = net(x if dtype is None else x.to(dtype))
    (logits.to(gl.dtype) * gl).sum().backward()
    return dict({"logits": logits.detach()}, **{n: p.grad for n, p in net.named_parameters()})


@gpu
def test_through_the_trial(monkeypatch):
    from katib_amd.ops import conv as hconv, enas_sepconv as hs
    from katib_amd.workloads.enas_child import ChildNet, ChildTrainer

    dev, k, calls = torch.device("cuda", 0), hconv.kernels(), []
    gen = torch.Generator().manual_seed(5)
    x, gl = torch.randn(8, 8, 16, 16, generator=gen).to(torch.bfloat16), torch.randn(8, 10, generator=gen)
    fused = ChildNet(ARCH, CFG, sep="fused").to(dev).to(memory_format=torch.channels_last)
    nets = {"split": ChildNet(ARCH, CFG).to(dev).to(memory_format=torch.channels_last), "truth": ChildNet(ARCH, CFG).double()}
    for net in nets.values():
        net.load_state_dict(fused.state_dict())
    xg = x.to(dev).contiguous(memory_format=torch.channels_last)
    ref, truth = _net_grads(nets["split"], xg, gl.to(dev)), _net_grads(nets["truth"], x, gl.double(), torch.float64)
    orig_sep, orig_conv = hs.separable_same, k.conv_fwd
    monkeypatch.setattr(hs, "separable_same", lambda *a: calls.append(1) or orig_sep(*a))
    monkeypatch.setattr(k, "dw_fwd", lambda *a, **kw: pytest.fail("dw_fwd reached from a fused layer"))
    monkeypatch.setattr(k, "conv_fwd", lambda xn, wk, y, geom: (geom[5] > 1 or pytest.fail("1x1 conv_fwd reached"))
                        and orig_conv(xn, wk, y, geom))
    got = _net_grads(fused, xg, gl.to(dev))
    assert len(calls) == 2
    for name in got:
        O.assert_rows_close(got[name].float().cpu().reshape(-1), ref[name].float().cpu().reshape(-1),
                            truth[name].reshape(-1), row=64, what=name)
    want = {n: tuple(t.shape) for n, t in nets["split"].state_dict().items()}
    for optim in ("module", "hip"):
        tr = ChildTrainer(ARCH, CFG, num_train=32, num_valid=8, batch_size=8, capture=True, optim=optim, sep="fused")
        for s in range(3):
            tr.step(torch.arange(8, device=dev) + 8 * s)
        torch.cuda.synchronize()
        assert torch.isfinite(tr.acc_buf).all() and len(calls) > 2
        assert {n: tuple(t.shape) for n, t in tr.model.state_dict().items()} == want
