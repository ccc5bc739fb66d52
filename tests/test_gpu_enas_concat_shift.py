"""``relu_pad_concat(..., pad8=True)`` (``csrc/hip/enas_concat.hip``: the shifted 16-byte kernels for one
narrow source, the element kernels with a padded pixel otherwise) against ``reference(..., pad8=True)``,
bit for bit; the convolution that takes the padded input, and the child with ``PAD8_INPUT``."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 2
FULL = [(8, 2)] * 9 + [(8, 3)] + [(8, 2)] * 6
CASES = ([[(8, 8), (3, 8)]]                                      # narrow last: 3 values + 5 zeros
         + [[(8, 8), (c, 8), (16, 8)] for c in (1, 2, 3, 6, 7)]  # odd and even shifts, both funnel halves
         + [[(8, 4), (3, 8), (16, 5), (8, 8)],                   # halves of a chunk with different H, t, pad parity
            [(3, 8), (8, 8)],                                    # narrow first: every aligned source shifted
            FULL[:2] + [(3, 2)] + FULL[2:15],                    # sixteen sources
            [(128, 32), (3, 32), (128, 32), (8, 16)],            # a row of two blockIdx.y segments
            [(8, 8), (3, 8), (5, 8)],                            # two narrow sources: element path with pad8
            [(16, 8), (8, 4)]])                                  # aligned: Cs == Ct
PARAMS = [(s, False) for s in CASES] + [(CASES[3], True)]       # once with NaN in the gradient's pad channels


def _sources(srcs, dev, gen):
    xs = []
    for c, h in srcs:
        x = torch.randn(B, c, h, h, device=dev, generator=gen)
        x = torch.where(torch.rand(x.shape, device=dev, generator=gen) < 0.2, torch.zeros_like(x), x)
        xs.append(x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last).requires_grad_(c >= 8))
    return xs


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("srcs,nan_pad", PARAMS)
def test_pad8_equals_reference(srcs, nan_pad, relu):
    from katib_amd.ops.enas_concat import reference, relu_pad_concat

    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(len(srcs) * 10 + srcs[1][0])
    xs = _sources(srcs, dev, gen)
    xr = [x.detach().float().requires_grad_(x.requires_grad) for x in xs]
    out, ref = relu_pad_concat(xs, relu, pad8=True), reference(xr, relu, pad8=True)
    Ct, Cs, m = sum(c for c, _ in srcs), ref.shape[1], ref.shape[2]
    assert Cs == (Ct + 7) // 8 * 8 and out.dtype == torch.bfloat16 and out.shape == ref.shape
    assert out.permute(0, 2, 3, 1).is_contiguous() and torch.equal(out, ref.to(torch.bfloat16))
    if Cs == Ct:
        assert torch.equal(out, relu_pad_concat([x.detach() for x in xs], relu))
    g = torch.randn(B, m, m, Cs, device=dev, generator=gen).to(torch.bfloat16)  # dense, random in the pad
    if nan_pad:
        g[..., Ct:] = float("nan")
    g = g.permute(0, 3, 1, 2)
    out.backward(g)
    ref.backward(g.float())  # F.pad's backward is a slice: the pad never meets arithmetic
    for x, r in zip(xs, xr):
        if x.requires_grad:
            assert x.grad.shape == x.shape and torch.equal(x.grad, r.grad.to(torch.bfloat16))
        else:
            assert x.grad is None


def test_conv_takes_the_padded_input():
    from katib_amd.ops.conv import same_conv2d

    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(5)
    w = (torch.randn(16, 67, 3, 3, device=dev, generator=gen) * 0.05).requires_grad_(True)
    x = torch.randn(B, 67, 8, 8, device=dev, generator=gen).to(torch.bfloat16).contiguous(
        memory_format=torch.channels_last)
    xp = torch.nn.functional.pad(x, (0, 0, 0, 0, 0, 5)).contiguous(memory_format=torch.channels_last)
    got = {}
    for name, inp in (("plain", x), ("padded", xp)):
        inp = inp.clone().requires_grad_(True)
        y = same_conv2d(inp, w, None, 1)
        gy = torch.randn(y.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(6)).to(torch.bfloat16)
        gx, gw = torch.autograd.grad(y, (inp, w), gy)
        got[name] = (y, gw, gx)
    assert got["padded"][1].shape == (16, 67, 3, 3) and got["padded"][2].shape == (B, 72, 8, 8)
    assert got["padded"][2].permute(0, 2, 3, 1).is_contiguous()
    for a, b in zip(got["plain"], (got["padded"][0], got["padded"][1], got["padded"][2][:, :67])):
        assert torch.equal(a, b)


def test_child_does_not_depend_on_pad8_input(monkeypatch):
    """Three layers with every skip bit set: layer 3 is a convolution over 32 + 3 + 32 channels of two map
    sizes (the shifted path), layer 2 a separable one that keeps its path. Logits and every gradient."""
    from katib_amd.workloads import enas_child

    emb = {"0": {"opt_type": "convolution", "filter_size": "3", "num_filter": "32", "stride": "1"},
           "1": {"opt_type": "separable_convolution", "filter_size": "3", "num_filter": "32", "stride": "2"},
           "2": {"opt_type": "convolution", "filter_size": "3", "num_filter": "64", "stride": "1"}}
    cfg = {"num_layers": 3, "input_sizes": [32, 32, 3], "output_sizes": [10], "embedding": emb}
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    net = enas_child.ChildNet([[0], [1, 1], [2, 1, 1]], cfg).to(dev).to(memory_format=torch.channels_last).train()
    x = torch.randn(B, 3, 32, 32, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    monkeypatch.setattr(enas_child, "FUSED_INPUT", True)
    res = {}
    for pad8 in (True, False):
        monkeypatch.setattr(enas_child, "PAD8_INPUT", pad8)
        net.zero_grad(set_to_none=True)
        torch.manual_seed(1)  # the same dropout mask both times
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
            logits = net(x)
        logits.float().sum().backward()
        res[pad8] = [logits.detach()] + [p.grad.clone() for p in net.parameters()]
    assert torch.isfinite(res[True][0]).all() and len(res[True]) > 1
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b)
