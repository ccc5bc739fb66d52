"""Needed-gradient pruning of the hand-scheduled DARTS backward (hip_darts.needed_grads, NEEDED_GRADS /
DROP_D): the plan itself (CPU), and the pruned passes against the PyTorch fp32 oracle -
an alpha-only pass (the architect's finite-difference passes), mixed needs (one weight + alphas),
the eval forward that no longer stores depthwise outputs, and captured search steps with the
switches on against off.

Bounds of the oracle comparisons: the change removes only outputs nobody reads, so it cannot add
error. ``PARENT_ERR`` holds the error of the commit before the change against the same oracle on
exactly these inputs (max |hip - torch| / max |torch|, the larger of three runs); the tests allow
twice that (float-atomic order varies between runs), and never less than one fp32 rounding of the
compared value (2^-23: an error measured as 0 is below the format's resolution, not a bound).
"""
import pytest
import torch

ALL = ["max_pooling_3x3", "avg_pooling_3x3", "skip_connection", "separable_convolution_3x3",
       "separable_convolution_5x5", "dilated_convolution_3x3", "dilated_convolution_5x5"]
EPS32 = 2.0 ** -23

# (C, L, batch) -> quantity -> relative error of the parent commit against the torch backend
# (measured on one MI355X; "grad" = the one weight gradient of the mixed-needs cases)
PARENT_ERR = {
    "alpha_only": {
        (4, 2, 8): {"loss": 0.000e+00, "logits": 3.004e-07, "ga_n": 1.046e-06, "ga_r": 4.566e-07, "bn": 5.941e-08},
        (4, 3, 8): {"loss": 1.025e-07, "logits": 4.712e-07, "ga_n": 6.597e-07, "ga_r": 1.034e-06, "bn": 5.809e-08},
        (8, 2, 8): {"loss": 1.021e-07, "logits": 2.839e-07, "ga_n": 5.198e-07, "ga_r": 7.436e-07, "bn": 5.729e-08},
        (16, 2, 4): {"loss": 2.069e-07, "logits": 3.429e-07, "ga_n": 4.916e-04, "ga_r": 6.009e-07, "bn": 5.958e-08},
    },
    "alpha_only_per_cell": {
        (4, 2, 8): {"loss": 0.000e+00, "logits": 3.434e-07, "ga_n": 1.185e-06, "ga_r": 4.729e-07, "bn": 1.188e-07},
    },
    "mixed_stem": {
        (4, 2, 8): {"loss": 0.000e+00, "logits": 3.434e-07, "ga_n": 1.220e-06, "ga_r": 5.055e-07, "bn": 5.941e-08,
                    "grad": 5.420e-07},
    },
    "mixed_pw": {
        (4, 2, 8): {"loss": 0.000e+00, "logits": 3.148e-07, "ga_n": 1.115e-06, "ga_r": 5.218e-07, "bn": 5.941e-08,
                    "grad": 1.912e-06},
    },
    "eval": {(4, 2, 8): {"loss": 0.000e+00}},
}


def _layout(C, L, nodes=3):
    from katib_amd.models.darts import DartsLayout

    return DartsLayout(ALL, init_channels=C, num_layers=L, num_nodes=nodes, stem_multiplier=1)


# ------------------------------------------------------------------------------------ the plan (CPU)
def _net_spec(L, nodes):
    from katib_amd.models.darts import DartsNetwork
    from katib_amd.ops import hip_darts as hd

    layout = _layout(4, L, nodes)
    return hd, layout, DartsNetwork(layout)._net_spec(hd)


@pytest.mark.parametrize("L", [2, 3])
@pytest.mark.parametrize("nodes", [2, 3])
def test_plan_alpha_only(L, nodes):
    """Detached weights, alpha leaves: the alpha-free states - the stem output, both preprocessed
    inputs of cell 0 and t0 of cell 1 (the preprocess of the stem output) - are the only dead ones."""
    hd, layout, spec = _net_spec(L, nodes)
    stem, cells = hd.network_needed_grads(spec, lambda n: False, True, True)
    assert stem is False
    assert len(cells) == L and all(len(c) == 2 + nodes for c in cells)
    dead = {(ci, j) for ci, c in enumerate(cells) for j, v in enumerate(c) if not v}
    assert dead == {(0, 0), (0, 1), (1, 0)}
    if L == 3:  # its inputs are the outputs of cells 0 and 1
        assert cells[2][0] and cells[2][1]


@pytest.mark.parametrize("L", [2, 3])
@pytest.mark.parametrize("nodes", [2, 3])
def test_plan_weights_only_nothing_and_stem_only(L, nodes):
    hd, layout, spec = _net_spec(L, nodes)
    stem, cells = hd.network_needed_grads(spec, lambda n: True, False, False)  # weights only: all alive
    assert stem and all(all(c) for c in cells)
    stem, cells = hd.network_needed_grads(spec, lambda n: False, False, False)  # nothing: all dead
    assert not stem and not any(any(c) for c in cells)
    # only the stem convolution weight: everything downstream of the stem is alive
    stem, cells = hd.network_needed_grads(spec, lambda n: n == "stem.conv", False, False)
    assert stem and all(all(c) for c in cells)


def test_plan_single_cell_inputs_and_own_parameters():
    """One cell: a needed input keeps its preprocessed state and every node alive, the other
    preprocessed state stays dead; a parameter of a node-1 edge keeps nodes 1.. alive only."""
    hd, layout, spec = _net_spec(2, 3)
    c0 = spec.cells[0]
    assert hd.needed_grads(c0, True, False, lambda n: False, False) == [True, False, True, True, True]
    name = c0.nodes[1][0][1][0]  # first parameter of node 1's first edge
    assert hd.needed_grads(c0, False, False, lambda n: n == name, False) == [False, False, False, True, True]
    pre1 = c0.pre1[1][0]
    assert hd.needed_grads(c0, False, False, lambda n: n == pre1, False) == [False, True, True, True, True]


# ------------------------------------------------------------------------------------------- GPU
def _inputs(layout, batch, dev):
    g = torch.Generator().manual_seed(11)
    W = torch.zeros(layout.n_weights)
    layout.init_weights(W, g)
    A = 1e-1 * torch.randn(layout.n_alphas, generator=g)
    x = torch.randn(batch, 3, 32, 32, generator=g).to(dev)
    y = torch.randint(0, 10, (batch,), generator=g).to(dev)
    return W.to(dev), A.to(dev), x, y


def _run(backend, layout, W, A, x, y, grad_names=(), net_function=True):
    """One training-mode forward_loss + backward with detached weights (``layout.views(W.detach())``),
    leaf alpha matrices, and the parameters ``grad_names`` as leaves of their own."""
    from katib_amd.models.darts import BNState, DartsNetwork
    from katib_amd.ops import darts as dops

    dops.set_backend(backend)
    try:
        dev = x.device
        net = DartsNetwork(layout, ops=dops)
        net.net_function = net_function
        P = dict(layout.views(W.detach().clone()))
        leaves = []
        for n in grad_names:
            P[n] = P[n].clone().requires_grad_(True)
            leaves.append(P[n])
        rows, K = layout.n_alpha_rows, len(layout.prims)
        an = A[:rows * K].view(rows, K).clone().requires_grad_(True)
        ar = A[rows * K:].view(rows, K).clone().requires_grad_(True)
        an.grad, ar.grad = torch.zeros_like(an), torch.zeros_like(ar)
        bn = BNState(layout, dev)
        loss, logits = net.forward_loss(x, y, P, an, ar, bn, training=True)
        loss.backward(inputs=leaves + [an, ar])
        torch.cuda.synchronize()
        out = {"loss": loss.detach().clone(), "logits": logits.detach().clone(), "ga_n": an.grad.clone(),
               "ga_r": ar.grad.clone(), "bn": bn.buf.clone()}
        for n, p in zip(grad_names, leaves):
            out["g:" + n] = p.grad.clone()
        return out
    finally:
        dops.set_backend("torch")


def _rel_err(a, b):
    return (a.double() - b.double()).abs().max().item() / (b.double().abs().max().item() + 1e-300)


def _check(group, case, got, ref):
    """Print every figure, then assert each against twice the parent's error (module docstring)."""
    errs = {k: _rel_err(got[k], ref[k]) for k in ref}
    key = {k: ("grad" if k.startswith("g:") else k) for k in ref}
    print("%s %s: %s" % (group, case, {key[k]: "%.3e" % v for k, v in errs.items()}))
    bounds = PARENT_ERR[group][case]
    for k, v in errs.items():
        bound = 2.0 * max(bounds[key[k]], EPS32)
        assert v <= bound, "%s %s %s: rel err %.3e > %.3e" % (group, case, k, v, bound)


_REF = {}


def _reference(case, grad_names=()):
    """The torch-backend result of a case, computed once and shared (never modified)."""
    key = (case, tuple(grad_names))
    if key not in _REF:
        C, L, batch = case
        layout = _layout(C, L)
        inp = _inputs(layout, batch, torch.device("cuda", 0))
        _REF[key] = (layout, inp, _run("torch", layout, *inp, grad_names=grad_names))
    return _REF[key]


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(4, 2, 8), (4, 3, 8), (8, 2, 8), (16, 2, 4)])
def test_alpha_only_pass_matches_torch(case):
    """Detached weights, leaf alphas: loss, logits, both alpha gradients and the BN running statistics
    of the pruned pass against the torch backend; (16, 2) runs the split depthwise / GEMM path that
    keeps its depthwise output."""
    layout, inp, ref = _reference(case)
    _check("alpha_only", case, _run("hip", layout, *inp), ref)


@pytest.mark.gpu
def test_alpha_only_pass_per_cell_path_matches_torch():
    case = (4, 2, 8)
    layout, inp, ref = _reference(case)
    _check("alpha_only_per_cell", case, _run("hip", layout, *inp, net_function=False), ref)


def _t0_stage1_pw(layout):
    e = layout.cells[0]["edges"][0]
    assert e["src"] == 0  # node 0's edge from t0
    return e["prefix"] + ".separable_convolution_3x3.0.pw"


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["stem", "pw"])
def test_mixed_needs_match_torch(which):
    """Everything detached except the alphas and ONE weight: the stem convolution (every state
    downstream needs a gradient again), or the stage-1 pointwise weight of a separable convolution
    on cell 0's edge t0 -> node 0 (its edge's operator backward must run although t0 needs no
    gradient, and its depthwise output must have been kept)."""
    case = (4, 2, 8)
    name = "stem.conv" if which == "stem" else _t0_stage1_pw(_layout(4, 2))
    layout, inp, ref = _reference(case, (name,))
    assert ref["g:" + name].abs().max().item() > 0
    _check("mixed_" + which, case, _run("hip", layout, *inp, grad_names=(name,)), ref)


def _evaluate(backend):
    from katib_amd.models.darts_search import DartsSearch
    from katib_amd.ops import darts as dops

    dev = torch.device("cuda", 0)
    layout = _layout(4, 2)
    _, _, x, y = _inputs(layout, 8, dev)
    dops.set_backend(backend)
    try:
        s = DartsSearch(layout, dev, capture=False)
        out = [t.clone() for t in s.evaluate(x, y)]
        torch.cuda.synchronize()
        return out
    finally:
        dops.set_backend("torch")


@pytest.mark.gpu
def test_eval_forward_matches_torch():
    """DartsSearch.evaluate (the forward that no longer stores depthwise outputs): loss within the
    parent's error of the torch backend's, top-1 / top-5 correct counts equal."""
    case = (4, 2, 8)
    (lt, t1, t5), (lh, h1, h5) = _evaluate("torch"), _evaluate("hip")
    assert round(float(h1) * 8) == round(float(t1) * 8) and round(float(h5) * 8) == round(float(t5) * 8)
    _check("eval", case, {"loss": lh}, {"loss": lt})


@pytest.mark.gpu
@pytest.mark.parametrize("hessian", ["stacked", "concurrent", "sequential"])
def test_captured_step_switches_on_equal_off(hessian):
    """One graph-captured second-order search step with NEEDED_GRADS / DROP_D on against
    off: weights and alphas agree under the bounds of
    test_stacked_hessian_passes_match_concurrent_and_sequential."""
    from katib_amd.models.darts_search import DartsSearch
    from katib_amd.ops import darts as dops
    from katib_amd.ops import hip_darts as hd

    dev = torch.device("cuda", 0)
    layout = _layout(4, 2)
    gen = torch.Generator(device=dev).manual_seed(5)
    batch = (torch.randn(8, 3, 32, 32, device=dev, generator=gen), torch.randint(0, 10, (8,), device=dev, generator=gen),
             torch.randn(8, 3, 32, 32, device=dev, generator=gen), torch.randint(0, 10, (8,), device=dev, generator=gen))
    names = ("NEEDED_GRADS", "DROP_D")
    old = [getattr(hd, n) for n in names]
    res = {}
    dops.set_backend("hip")
    try:
        for on in (True, False):
            for n in names:
                setattr(hd, n, on)
            s = DartsSearch(layout, dev, capture=True, hessian=hessian)
            assert s.hessian == hessian
            s.step(*batch)
            torch.cuda.synchronize()
            res[on] = (s.W.clone(), s.A.clone())
    finally:
        for n, v in zip(names, old):
            setattr(hd, n, v)
        dops.set_backend("torch")
    for name_, a, b, rtol, atol in (("W", res[True][0], res[False][0], 1e-4, 1e-5),
                                    ("alpha", res[True][1], res[False][1], 1e-3, 5e-5)):
        scale = b.abs().max().item() + 1e-12
        err = (a - b).abs().max().item()
        print("%s %s: max err %.3e (scale %.3e)" % (hessian, name_, err, scale))
        assert err <= atol + rtol * scale, "%s: max err %.3e (scale %.3e)" % (name_, err, scale)
