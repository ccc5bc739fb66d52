"""The ENAS child's layer-input kernels (``csrc/hip/enas_concat.hip``) against ``reference`` - pad,
cat, ReLU in PyTorch: values and every source gradient bit for bit, at the smallest shapes at
which each path can go wrong."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 2
FULL = [(8, 2)] * 9 + [(8, 3)] + [(8, 2)] * 6  # sixteen sources, the full table
# (C, H) per source, and whether gout also comes with a pixel stride of Ct + 5 rounded up to 8
CASES = [([(8, 4)], False),                        # one source: the ReLU-only layer
         ([(16, 8), (8, 4)], True),                # even pad, 2 / 2
         ([(8, 8), (8, 5)], False),                # odd pad, 1 / 2
         ([(24, 7), (8, 32), (16, 16)], False),    # the largest map is not first, three sizes
         ([(8, 8), (3, 8)], True),                 # the image as a skip source: element path
         ([(64, 16), (3, 32)], False),
         (FULL, False)]
PARAMS = [(srcs, wide) for srcs, w in CASES for wide in ([False, True] if w else [False])]


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("srcs,wide", PARAMS)
def test_relu_pad_concat_equals_reference(srcs, wide, relu):
    from katib_amd.ops.enas_concat import reference, relu_pad_concat

    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(len(srcs) * 10 + srcs[0][0])
    xs = []
    for c, h in srcs:
        x = torch.randn(B, c, h, h, device=dev, generator=gen)
        x = torch.where(torch.rand(x.shape, device=dev, generator=gen) < 0.2, torch.zeros_like(x), x)
        x = x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        xs.append(x.requires_grad_(c != 3))  # the image gets no gradient
    xr = [x.detach().float().requires_grad_(x.requires_grad) for x in xs]
    out, ref = relu_pad_concat(xs, relu), reference(xr, relu)
    assert out.dtype == torch.bfloat16 and torch.equal(out, ref.to(torch.bfloat16))
    assert torch.equal(out, reference([x.detach() for x in xs], relu))
    Ct, m = ref.shape[1], ref.shape[2]
    gs = (Ct + 5 + 7) // 8 * 8 if wide else Ct
    g = torch.randn(B, m, m, gs, device=dev, generator=gen).to(torch.bfloat16)[..., :Ct].permute(0, 3, 1, 2)
    out.backward(g)
    ref.backward(g.float())
    for x, r in zip(xs, xr):
        if x.requires_grad:
            assert x.grad.shape == x.shape and torch.equal(x.grad, r.grad.to(torch.bfloat16))
        else:
            assert x.grad is None


def test_child_logits_do_not_depend_on_fused_input(monkeypatch):
    """Three layers with every skip bit set, so the image is a skip source of layers 2 and 3."""
    from katib_amd.workloads import enas_child

    emb = {"0": {"opt_type": "convolution", "filter_size": "3", "num_filter": "32", "stride": "1"},
           "1": {"opt_type": "separable_convolution", "filter_size": "3", "num_filter": "32", "stride": "2"},
           "2": {"opt_type": "convolution", "filter_size": "3", "num_filter": "64", "stride": "1"}}
    cfg = {"num_layers": 3, "input_sizes": [32, 32, 3], "output_sizes": [10], "embedding": emb}
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    net = enas_child.ChildNet([[0], [1, 1], [2, 1, 1]], cfg).to(dev).to(memory_format=torch.channels_last).eval()
    x = torch.randn(B, 3, 32, 32, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    logits = {}
    for fused in (True, False):
        monkeypatch.setattr(enas_child, "FUSED_INPUT", fused)
        with torch.no_grad(), torch.autocast(device_type="cuda", dtype=torch.bfloat16):
            logits[fused] = net(x)
    assert torch.isfinite(logits[True]).all() and torch.equal(logits[True], logits[False])


def test_seventeen_sources_raise():
    from katib_amd.ops.enas_concat import relu_pad_concat

    x = torch.zeros(B, 8, 2, 2, device="cuda", dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError, match="sources"):
        relu_pad_concat([x] * 17, True)
