"""``ops/enas_concat.py`` on the CPU: ``reference`` (pad, cat, ReLU) against the contract written
out index by index, and ``relu_pad_concat`` on CPU tensors against ``reference``."""
import pytest
import torch

from katib_amd.ops.enas_concat import reference, relu_pad_concat

# (C, H) per source: d = 3 (1 row above, 2 below), d = 2 with the largest map last, one source
CASES = [[(2, 5), (3, 2)], [(1, 2), (2, 4), (3, 4)], [(4, 3)]]


def _sources(case, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(2, c, h, h, generator=g) for c, h in case]


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("case", CASES)
def test_reference_is_the_contract(case, relu):
    xs = _sources(case, 1)
    m = max(h for _, h in case)
    want = torch.zeros(2, sum(c for c, _ in case), m, m)
    off = 0
    for x, (c, h) in zip(xs, case):
        t = (m - h) // 2
        for y in range(h):
            for xx in range(h):
                v = x[:, :, y, xx]
                want[:, off:off + c, y + t, xx + t] = torch.where(v > 0, v, torch.zeros(())) if relu else v
        off += c
    assert torch.equal(reference(xs, relu), want)


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("case", CASES)
def test_cpu_path_is_the_reference(case, relu):
    xs = [x.requires_grad_(True) for x in _sources(case, 2)]
    xr = [x.detach().clone().requires_grad_(True) for x in xs]
    out, ref = relu_pad_concat(xs, relu), reference(xr, relu)
    assert torch.equal(out, ref)
    g = torch.randn(ref.shape, generator=torch.Generator().manual_seed(3))
    out.backward(g)
    ref.backward(g)
    for a, b in zip(xs, xr):
        assert torch.equal(a.grad, b.grad)
