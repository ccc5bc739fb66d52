"""The HipMLP train-step oracle (tests/mlp_step_oracle.py), validated without a GPU: with no rounding
and fp64 everywhere it is two consecutive autograd steps of the trial's modules under the real
optimizers; and the trial's ``--impl hip`` refuses a width the kernels cannot read."""
import pytest
import torch
import torch.nn.functional as F

import mlp_step_oracle as O
from katib_amd.workloads import mnist_mlp


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-6))


def _module(num_layers, hidden):
    torch.manual_seed(5)
    return (mnist_mlp.MLP(hidden) if num_layers == 0 else mnist_mlp.DeepMLP(hidden, num_layers)).double()


def _params(model):
    fcs = [model.fc1, model.fc2, model.fc3] if isinstance(model, mnist_mlp.MLP) else list(model.hidden) + [model.out]
    return [(fc.weight, fc.bias) for fc in fcs]


@pytest.mark.parametrize("num_layers", [0, 1, 3])  # 0: the MLP module (784-h-h/2-10)
@pytest.mark.parametrize("optimizer", ["sgd", "adam", "ftrl"])
def test_oracle_is_two_autograd_steps(optimizer, num_layers):
    hidden, batch, lr, momentum = 24, 10, 0.02, 0.9
    model = _module(num_layers, hidden)
    layers = O.layers_from_module(model, optimizer, dtype=torch.float64)
    if optimizer == "adam":
        opt = torch.optim.Adam(model.parameters(), lr=lr)
    elif optimizer == "ftrl":
        opt = mnist_mlp.Ftrl(model.parameters(), lr=lr)
    else:
        opt = torch.optim.SGD(model.parameters(), lr=lr, momentum=momentum)
    g = torch.Generator().manual_seed(6)
    for t in (1, 2):
        x = torch.randn(batch, 784, generator=g, dtype=torch.float64)
        y = torch.randint(0, 10, (batch,), generator=g)
        logits = model(x)
        loss = F.cross_entropy(logits, y)
        opt.zero_grad()
        loss.backward()
        opt.step()
        o_logits, o_loss = O.train_step(layers, x, y, optimizer, lr, momentum=momentum, t=t,
                                        gemm_dtype=torch.float64, round=None)
        assert _rel(o_logits, logits) <= 1e-12 and abs(o_loss - loss.item()) <= 1e-12 * max(1.0, abs(loss.item()))
        for i, ((w, b), l) in enumerate(zip(_params(model), layers)):
            assert l["w"].dtype == torch.float64
            assert _rel(l["w"], w) <= 1e-12, (t, i, _rel(l["w"], w))
            assert _rel(l["b"], b) <= 1e-12, (t, i, _rel(l["b"], b))


def test_oracle_rounds_where_asked():
    """bf16 rounding keeps fp32 masters and state and bf16 shadows; the padded output rows stay zero."""
    model = _module(2, 24)
    layers = O.layers_from_module(model, "adam", pad_out=16)
    g = torch.Generator().manual_seed(7)
    x, y = torch.randn(10, 784, generator=g), torch.randint(0, 10, (10,), generator=g)
    logits, loss = O.train_step(layers, x, y, "adam", 0.02, t=1, gemm_dtype=torch.float64, round=torch.bfloat16)
    assert logits.shape == (10, 16) and torch.equal(logits, logits.to(torch.bfloat16).to(logits.dtype))
    for l in layers:
        assert l["w"].dtype == l["m"].dtype == l["bv"].dtype == torch.float32
        assert l["w16"].dtype == torch.bfloat16 and torch.equal(l["w16t"], l["w"].to(torch.bfloat16).t())
    out = layers[-1]
    for name in ("w", "b", "m", "v", "bm", "bv", "w16"):
        assert float(out[name][10:].abs().max()) == 0.0, name
    assert loss == loss


def test_hip_refuses_a_hidden_width_that_is_no_multiple_of_8():
    with pytest.raises(SystemExit) as e:
        mnist_mlp.main(["--impl", "hip", "--num-layers", "2", "--hidden", "100"])
    assert "multiple of 8" in str(e.value)
