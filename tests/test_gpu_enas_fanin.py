"""The ENAS child's gradient fan-in (``csrc/hip/enas_fanin.hip``, ``ops/enas_fanin.py``): the kernel against
its formula in fp64, bit for bit, on values whose sums are exact in fp32 (the grid k / 64, |k| <= 255); the
deferral through ``share`` / ``relu_pad_concat(..., fans=...)`` against autograd over ``reference`` in fp64;
and ``gradsum='hip'`` through the trial, under the per-row rule of ``test_gpu_enas_sepconv``."""
import pytest
import torch

import gpt2_kernel_oracle as O

gpu = pytest.mark.gpu
BF = torch.bfloat16
# name -> (H, C, x kind, terms); a term is (m, Cg, gs, off, relu): g is the [..., :Cg] slice of a [B, m, m, gs] buffer
CASES = {
    "one-relu": (5, 16, "grid", [(5, 16, 16, 0, True)]),
    "three+dense": (5, 8, "grid", [(8, 24, 24, 8, True), (5, 8, 8, 0, False), (5, 16, 24, 8, True), (5, 8, 8, 0, False)]),
    "pad8-funnel": (5, 8, "grid", [(6, 24, 24, 3, True), (5, 24, 24, 11, False), (5, 8, 8, 0, True)]),
    "16-terms": (3, 8, "grid", [(3 + k % 2, 16, 16, 8 * (k % 2), k % 3 == 0) for k in range(16)]),
    "long-row": (32, 528, "grid", [(32, 528, 528, 0, True), (33, 536, 536, 8, False)]),
    "no-relu": (4, 8, "nan", [(4, 8, 8, 0, False), (5, 16, 16, 8, False)]),
    "nan-in-g": (5, 8, "grid", [(8, 24, 24, 8, True), (5, 8, 8, 0, False), (5, 16, 24, 8, True)]),
}


def _grid(gen, *shape):
    return (torch.randint(-255, 256, shape, generator=gen) / 64).to(BF)


def _same(a, b):  # torch.equal that lets a NaN equal a NaN
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(), b.nan_to_num())


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_kernel_against_fp64(name):
    from katib_amd.ops.conv import kernels
    from katib_amd.ops.enas_concat import relu_pad_concat

    H, C, xkind, terms = CASES[name]
    B, dev, gen = 2, torch.device("cuda", 0), torch.Generator().manual_seed(len(name))
    x = _grid(gen, B, H, H, C) if xkind == "grid" else torch.full((B, H, H, C), float("nan"), dtype=BF)
    gs = [_grid(gen, B, m, m, s)[..., :Cg] for m, Cg, s, _, _ in terms]
    if name == "nan-in-g":  # through the first (ReLU) term, once where x > 0 and once where x <= 0
        x[0, 1, 1, 2], x[1, 2, 3, 5] = 1.5, -0.25
        gs[0][0, 2, 2, 10] = gs[0][1, 3, 4, 13] = float("nan")  # t = 1, off = 8
    masked, plain = torch.zeros(B, H, H, C, dtype=torch.float64), torch.zeros(B, H, H, C, dtype=torch.float64)
    for g, (m, _, _, off, relu) in zip(gs, terms):
        t = (m - H) // 2
        (masked if relu else plain).add_(g[:, t:t + H, t:t + H, off:off + C].double())
    want = (torch.where(x.double() > 0, masked, torch.zeros((), dtype=torch.float64)) + plain).to(BF)
    if name == "nan-in-g":
        assert want[0, 1, 1, 2].isnan() and not want[1, 2, 3, 5].isnan()
    got = torch.full((B, H, H, C), float("nan"), dtype=BF, device=dev)
    dg = [torch.empty(B, m, m, s, dtype=BF, device=dev)[..., :Cg].copy_(g) for g, (m, Cg, s, _, _) in zip(gs, terms)]
    kernels().enas_fanin(x.to(dev), [(g, off, relu) for g, (_, _, _, off, relu) in zip(dg, terms)], got)
    assert _same(got.cpu(), want)
    if name == "one-relu":  # the concat backward's own gx
        xc = x.to(dev).permute(0, 3, 1, 2).requires_grad_(True)
        relu_pad_concat([xc], relu=True).backward(dg[0].permute(0, 3, 1, 2))
        assert torch.equal(xc.grad.permute(0, 2, 3, 1), got)


@pytest.mark.parametrize("dev", ["cpu", pytest.param("cuda", marks=gpu)])
def test_mechanism(dev):
    from katib_amd.ops.enas_concat import reference, relu_pad_concat
    from katib_amd.ops.enas_fanin import share

    gen = torch.Generator().manual_seed(11)

    def nchw(*shape):  # channels-last memory
        return _grid(gen, *shape).permute(0, 3, 1, 2)

    a, b, c, img = nchw(2, 6, 6, 8), nchw(2, 4, 4, 16), nchw(2, 3, 3, 8), nchw(2, 6, 6, 3)
    w1, w2, w3, wb = nchw(2, 6, 6, 24), nchw(2, 6, 6, 32), nchw(2, 6, 6, 40), nchw(2, 4, 4, 16)

    def loss_of(outs, b_read):
        return sum((o * w).sum() for o, w in zip(outs, (w1, w2, w3))) + (b_read * wb).sum()

    ta, tb, tc = (t.double().requires_grad_(True) for t in (a, b, c))
    i64 = img.double()
    loss_of([reference([ta, tb], True), reference([tb, ta, tc], False), reference([tc, i64, ta, tb], True, pad8=True)],
            tb).backward()
    a, b, c, img, w1, w2, w3, wb = (t.to(dev) for t in (a, b, c, img, w1, w2, w3, wb))
    la, lb, lc = (t.requires_grad_(True) for t in (a, b, c))
    (va, fa), (vb, fb), (vc, fc) = share(la), share(lb), share(lc)
    loss = loss_of([relu_pad_concat([va, vb], True, fans=[fa, fb]),
                    relu_pad_concat([vb, va, vc], False, fans=[fb, fa, fc]),
                    relu_pad_concat([vc, img, va, vb], True, pad8=True, fans=[fc, None, fa, fb])], vb)
    loss.backward(retain_graph=True)
    assert fa.spent and fb.spent and fc.spent
    for leaf, truth in ((la, ta), (lb, tb), (lc, tc)):
        assert torch.equal(leaf.grad.cpu(), truth.grad.to(BF))
    with pytest.raises(RuntimeError, match="spent"):
        loss.backward()


ARCH = [[0], [1, 1], [2, 1, 1], [0, 1, 1, 1]]  # convolution, separable, reduction, convolution; every skip taken
CFG = {"num_layers": 4, "input_sizes": [8, 16, 16], "output_sizes": [10], "embedding": {
    "0": {"opt_type": "convolution", "num_filter": 16, "filter_size": 3, "stride": 1},
    "1": {"opt_type": "separable_convolution", "num_filter": 16, "filter_size": 3, "stride": 1},
    "2": {"opt_type": "reduction", "reduction_type": "max_pooling", "pool_size": 2}}}


def _net_grads(net, x, gl, dtype=None):
    net.train()
    net.drop.p = 0.0  # the three nets must compute the same function
    with torch.autocast("cuda", dtype=BF, enabled=dtype is None):
        logits = net(x if dtype is None else x.to(dtype))
    (logits.to(gl.dtype) * gl).sum().backward()
    return dict({"logits": logits.detach()}, **{n: p.grad for n, p in net.named_parameters()})


@gpu
def test_through_the_trial(monkeypatch):
    from katib_amd.ops.conv import kernels
    from katib_amd.workloads.enas_child import ChildNet, ChildTrainer

    dev, k, calls = torch.device("cuda", 0), kernels(), []
    gen = torch.Generator().manual_seed(5)
    x, gl = torch.randn(8, 8, 16, 16, generator=gen).to(BF), torch.randn(8, 10, generator=gen)
    hip = ChildNet(ARCH, CFG, gradsum="hip").to(dev).to(memory_format=torch.channels_last)
    nets = {"autograd": ChildNet(ARCH, CFG).to(dev).to(memory_format=torch.channels_last), "truth": ChildNet(ARCH, CFG).double()}
    for net in nets.values():
        net.load_state_dict(hip.state_dict())
    xg = x.to(dev).contiguous(memory_format=torch.channels_last)
    ref, truth = _net_grads(nets["autograd"], xg, gl.to(dev)), _net_grads(nets["truth"], x, gl.double(), torch.float64)
    orig = k.enas_fanin
    monkeypatch.setattr(k, "enas_fanin", lambda xn, terms, gx: calls.append(len(terms)) or orig(xn, terms, gx))
    got = _net_grads(hip, xg, gl.to(dev))
    assert sorted(calls) == [1, 2, 3]  # layer 3 read by layer 4; layer 2 by 3 and 4; layer 1 by 2, 3 and 4
    for name in got:
        O.assert_rows_close(got[name].float().cpu().reshape(-1), ref[name].float().cpu().reshape(-1),
                            truth[name].reshape(-1), row=64, what=name)
    want = {n: tuple(t.shape) for n, t in nets["autograd"].state_dict().items()}
    for optim in ("module", "hip"):
        tr = ChildTrainer(ARCH, CFG, num_train=32, num_valid=8, batch_size=8, capture=True, optim=optim, gradsum="hip")
        for s in range(3):
            tr.step(torch.arange(8, device=dev) + 8 * s)
        torch.cuda.synchronize()
        assert torch.isfinite(tr.acc_buf).all() and len(calls) > 3
        assert {n: tuple(t.shape) for n, t in tr.model.state_dict().items()} == want
