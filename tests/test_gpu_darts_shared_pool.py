"""Pooling shared between the edges that read one DARTS cell state (hip_darts.pool_groups).

Kernel level: pool_bwd_multi with 1..4 gradient sources per entry against an fp64 reference of the
summed per-edge formula. Cell level: hip_darts.cell_forward against the torch backend (output, input
gradients, d(alpha), weight gradients, every edge's own running statistics), primitive subsets,
detached weights and eval mode with per-edge running statistics. Launch structure: one pool entry
per state, forward and backward.

Tolerances are those of test_gpu_darts.test_mixed_node_matches_torch (rtol 1e-3 of the largest
reference magnitude + atol 1e-4; running statistics atol 1e-5).
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ALL = ["max_pooling_3x3", "avg_pooling_3x3", "skip_connection", "separable_convolution_3x3",
       "separable_convolution_5x5", "dilated_convolution_3x3", "dilated_convolution_5x5"]
EPS = 1e-5


def _close(a, b, name, rtol=1e-3, atol=1e-4):
    scale = b.abs().max().item() + 1e-12
    err = (a - b).abs().max().item()
    assert err <= atol + rtol * scale, "%s: max err %.3e (scale %.3e)" % (name, err, scale)


# ------------------------------------------------------------------------------------- kernel level
def _pool_case(hd, K, S, HW, pools, C, ident, nextra, overwrite, rep, seed):
    """One pool_bwd_multi entry with K sources: (got, fp64 reference) of the state's gradient."""
    dev = torch.device("cuda", 0)
    REP = hd.REP
    N, H, W = 2, HW, HW
    Ho, Wo = (H - 1) // S + 1, (W - 1) // S + 1
    cnt = N * Ho * Wo
    g = torch.Generator().manual_seed(seed)
    n = N * C * H * W
    # distinct values: no pooling window has tied maxima
    x = ((torch.randperm(n, generator=g).double() / n) * 4 - 2).view(N, C, H, W)
    za = F.avg_pool2d(x, 3, S, 1, count_include_pad=False)
    zm, idx = F.max_pool2d(x, 3, S, 1, return_indices=True)
    oy = torch.arange(Ho).view(1, 1, Ho, 1)
    ox = torch.arange(Wo).view(1, 1, 1, Wo)
    tap = ((idx // W - oy * S + 1) * 3 + (idx % W - ox * S + 1)).to(torch.uint8)
    za_s, zm_s = za.to(hd.ZDT).to(dev), zm.to(hd.ZDT).to(dev)  # what the kernel reads
    zad, zmd = za_s.double().cpu(), zm_s.double().cpu()

    def moments(z):
        m = z.mean((0, 2, 3))
        v = (z * z).mean((0, 2, 3)) - m * m
        inv = 1 / torch.sqrt(v + EPS)
        stats = torch.zeros(REP, 2 * C, dtype=torch.float64)
        stats[0, :C], stats[0, C:] = z.sum((0, 2, 3)), (z * z).sum((0, 2, 3))
        return (z - m.view(1, C, 1, 1)) * inv.view(1, C, 1, 1), inv.view(1, C, 1, 1), stats.to(dev)

    zha, inva, stats_a = moments(zad)
    zhm, invm, stats_m = moments(zmd)
    has_a, has_m = pools in ("avg", "both"), pools in ("max", "both")
    dummy = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    bna = (stats_a, dummy[0], dummy[1], 1.0 / cnt, False, EPS, 1, 2 * C) if has_a else None
    bnm = (stats_m, dummy[0], dummy[1], 1.0 / cnt, False, EPS, 1, 2 * C) if has_m else None
    nred = 3 * C + 1
    dza, dzm = torch.zeros_like(zad), torch.zeros_like(zmd)
    ref = torch.zeros(N, C, H, W, dtype=torch.float64)
    srcs, keep = [], []
    for e in range(K):
        dout = torch.randn(N, C, Ho, Wo, generator=g)
        w = torch.softmax(torch.randn(8, generator=g), 0)
        gd = dout.double()
        sums = torch.cat([gd.sum((0, 2, 3)), (gd * zha).sum((0, 2, 3)), (gd * zhm).sum((0, 2, 3)), torch.zeros(1).double()])
        red = torch.zeros(REP, nred, dtype=torch.float64)
        if rep == 1:
            red[0] = sums
        else:  # the sums arrive unfolded: spread over the replicas
            frac = torch.rand(REP, 1, generator=g).double()
            red = sums.view(1, nred) * (frac / frac.sum())
        red = red.to(dev).contiguous().view(-1)
        wd = w.to(dev)
        # in "both" the second source has only the avg pool and the third only the max pool
        ea = has_a and not (pools == "both" and e == 2)
        em = has_m and not (pools == "both" and e == 1)
        m1 = (gd.sum((0, 2, 3)) / cnt).view(1, C, 1, 1)
        if ea:
            dza += w[1].double() * inva * (gd - m1 - zha * ((gd * zha).sum((0, 2, 3)) / cnt).view(1, C, 1, 1))
        if em:
            dzm += w[0].double() * invm * (gd - m1 - zhm * ((gd * zhm).sum((0, 2, 3)) / cnt).view(1, C, 1, 1))
        pa = (red[:C], red[C:2 * C], wd, 1, rep, nred, None) if ea else None
        pm = (red[:C], red[2 * C:3 * C], wd, 0, rep, nred, None) if em else None
        idn = ident and S == 1 and e % 2 == 0  # (every other source, the first included)
        if idn:
            ref += w[2].double() * gd
        extras = [torch.randn(N, C, H, W, generator=g) for _ in range(nextra if e != 1 else max(nextra - 1, 0))]
        for t in extras:
            ref += t.double()
        dd = dout.to(dev)
        ex = [t.to(dev) for t in extras]
        keep += [dd, ex, red, wd]
        srcs.append((dd, pa, pm, wd if idn else None, 2 if idn else -1, ex))
    for z_fn, dz, on in ((lambda t: F.avg_pool2d(t, 3, S, 1, count_include_pad=False), dza, has_a),
                         (lambda t: F.max_pool2d(t, 3, S, 1), dzm, has_m)):
        if on:
            xr = x.clone().requires_grad_(True)
            z_fn(xr).backward(dz)
            ref += xr.grad
    gx0 = torch.randn(N, C, H, W, generator=g)
    if not overwrite:
        ref += gx0.double()
    gx = gx0.to(dev)
    x32 = x.float().to(dev)
    hd._K.pool_bwd_multi([(za_s if has_a else None, zm_s if has_m else None, bna, bnm,
                           tap.to(dev) if has_m else None, x32, gx, overwrite, S, srcs)])
    torch.cuda.synchronize()
    return gx.cpu().double(), ref


# the options every (K, S, plane, pools) case runs through: (C, identity, extras per source,
# overwrite, replicas of the BN-backward sums) - each value of each option with both values of the others' neighbours
def _variants(REP):
    return [(4, False, 0, True, 1), (8, True, 1, False, REP), (4, True, 4, True, REP), (8, False, 4, False, 1),
            (4, False, 1, False, REP), (8, True, 0, True, 1), (4, True, 0, False, 1), (8, False, 1, True, REP)]


@pytest.mark.parametrize("pools", ["avg", "max", "both"])
@pytest.mark.parametrize("HW", [8, 6])  # 8 x 8: the 16-byte path; 6 x 6 (stride 2: 3 x 3): the scalar path
@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_pool_bwd_multi_sources_match_fp64(K, S, HW, pools):
    from katib_amd.ops import hip_darts as hd

    assert hd.POOL_SHARE == 4
    for i, (C, ident, nextra, overwrite, rep) in enumerate(_variants(hd.REP)):
        got, ref = _pool_case(hd, K, S, HW, pools, C, ident, nextra, overwrite, rep, seed=100 * K + 10 * S + i)
        _close(got, ref, "gx K=%d S=%d HW=%d %s C=%d id=%s extras=%d overwrite=%s rep=%d"
               % (K, S, HW, pools, C, ident, nextra, overwrite, rep))


def test_pool_bwd_multi_rejects_a_fifth_source():
    from katib_amd.ops import hip_darts as hd

    dev = torch.device("cuda", 0)
    x = torch.zeros(2, 4, 8, 8, device=dev)
    src = (torch.zeros(2, 4, 8, 8, device=dev), None, None, None, -1, [torch.zeros(2, 4, 8, 8, device=dev)])
    with pytest.raises(RuntimeError):
        hd._K.pool_bwd_multi([(None, None, None, None, None, x, torch.zeros_like(x), True, 1, [src] * 5)])


# --------------------------------------------------------------------------------------- cell level
def _layout(prims, C, nodes):
    from katib_amd.models.darts import DartsLayout

    layout = DartsLayout(prims, init_channels=C, num_layers=2, num_nodes=nodes, stem_multiplier=1)
    W = torch.zeros(layout.n_weights)
    layout.init_weights(W, torch.Generator().manual_seed(0))
    return layout, W.to(torch.device("cuda", 0))


def _run_cell(backend, layout, W, ci, s0, s1, wts, R, training=True, weights=True, inputs=True, bn_buf=None):
    """One cell (preprocess, nodes, concat) forward + backward on ``backend``."""
    from katib_amd.models.darts import BNState, DartsNetwork
    from katib_amd.ops import darts as dops

    dev = W.device
    dops.set_backend(backend)
    try:
        net = DartsNetwork(layout)
        Wl = W.clone()
        gW = torch.zeros_like(Wl)
        P, G = layout.views(Wl), layout.views(gW)
        if weights:
            for k, v in P.items():
                v.requires_grad_(True)
                v.grad = G[k]
        bn = BNState(layout, dev)
        if bn_buf is not None:
            bn.buf.copy_(bn_buf)
        a0, a1 = s0.clone().requires_grad_(inputs), s1.clone().requires_grad_(inputs)
        wl = wts.clone().requires_grad_(True)
        cell = layout.cells[ci]
        if backend == "hip":
            hd = dops.hip_module()
            spec = net._cell_spec(hd, ci)
            out = hd.cell_forward(spec, a0, a1, wl, [P[n] for n in spec.names], bn.get, training, net.momentum, net.eps)
        else:
            pre = "cells.%d" % ci
            states = [net.preprocess(a0, pre + ".pre0", cell["reduction_prev"], P, bn, training),
                      net.preprocess(a1, pre + ".pre1", False, P, bn, training)]
            rows, ei = net._split_rows(wl), 0
            for n in range(layout.N):
                edges = cell["edges"][ei:ei + 2 + n]
                ei += 2 + n
                states.append(net.mixed_node(states, edges, P, rows[n], bn, training))
            out = torch.cat(states[2:], dim=1)
        leaves = [wl] + ([a0, a1] if inputs else []) + (list(P.values()) if weights else [])
        (out * R).sum().backward(inputs=leaves)
        torch.cuda.synchronize()
        return {"out": out.detach(), "ds0": a0.grad, "ds1": a1.grad, "dalpha": wl.grad, "dW": gW if weights else None,
                "running_mean": bn.mean.clone(), "running_var": bn.var.clone()}
    finally:
        dops.set_backend("torch")


def _cell_inputs(layout, ci, seed=11):
    dev = torch.device("cuda", 0)
    cell = layout.cells[ci]
    gen = torch.Generator(device=dev).manual_seed(seed)
    H = 16 if cell["reduction"] else 8  # every node state is 8 x 8
    s0 = torch.randn(2, cell["cpp"], H, H, device=dev, generator=gen)
    s1 = torch.randn(2, cell["cp"], H, H, device=dev, generator=gen)
    wts = torch.softmax(torch.randn(layout.n_alpha_rows, len(layout.prims), device=dev, generator=gen), -1)
    R = torch.randn(2, cell["C"] * layout.N, 8, 8, device=dev, generator=gen)
    return s0, s1, wts, R


def _compare(got, ref, names):
    for name in names:
        a, b = got[name], ref[name]
        assert (a is None) == (b is None), name
        if b is not None:
            _close(a, b, name, atol=1e-5 if name.startswith("running") else 1e-4)


EVERYTHING = ["out", "ds0", "ds1", "dalpha", "dW", "running_mean", "running_var"]


@pytest.mark.parametrize("C", [4, 8])  # initial channels (the reduction cell is twice as wide)
@pytest.mark.parametrize("nodes", [3, 4])
@pytest.mark.parametrize("ci", [0, 1], ids=["normal", "reduction"])
def test_cell_matches_torch(ci, nodes, C):
    layout, W = _layout(ALL, C, nodes)
    args = _cell_inputs(layout, ci)
    _compare(_run_cell("hip", layout, W, ci, *args), _run_cell("torch", layout, W, ci, *args), EVERYTHING)


@pytest.mark.parametrize("prims", [["max_pooling_3x3"], ["avg_pooling_3x3"], ["skip_connection", "none"]],
                         ids=["max", "avg", "skip_none"])
@pytest.mark.parametrize("ci", [0, 1], ids=["normal", "reduction"])
def test_cell_primitive_subsets_match_torch(ci, prims):
    layout, W = _layout(prims, 4, 3)
    args = _cell_inputs(layout, ci, seed=12)
    _compare(_run_cell("hip", layout, W, ci, *args), _run_cell("torch", layout, W, ci, *args), EVERYTHING)


@pytest.mark.parametrize("ci", [0, 1], ids=["normal", "reduction"])
def test_cell_detached_weights_dalpha_only(ci):
    """The architect's finite-difference passes: nothing but the softmax weights needs a gradient, so
    only the node states' groups run and the edges from the cell inputs are pruned."""
    layout, W = _layout(ALL, 4, 3)
    args = _cell_inputs(layout, ci, seed=13)
    kw = dict(weights=False, inputs=False)
    _compare(_run_cell("hip", layout, W, ci, *args, **kw), _run_cell("torch", layout, W, ci, *args, **kw),
             ["out", "dalpha", "running_mean", "running_var"])


@pytest.mark.parametrize("ci", [0, 1], ids=["normal", "reduction"])
def test_cell_eval_mode_keeps_each_edges_running_statistics(ci):
    """Eval mode normalises every edge with its OWN running statistics, set to different values
    here: only the pre-BN pooled tensors are shared, forward and backward."""
    from katib_amd.models.darts import BNState

    layout, W = _layout(ALL, 4, 3)
    dev = W.device
    bn = BNState(layout, dev)
    bn.mean.normal_(generator=torch.Generator(device=dev).manual_seed(3))
    bn.var.uniform_(0.5, 2.0, generator=torch.Generator(device=dev).manual_seed(4))
    args = _cell_inputs(layout, ci, seed=14)
    kw = dict(training=False, bn_buf=bn.buf)
    got, ref = _run_cell("hip", layout, W, ci, *args, **kw), _run_cell("torch", layout, W, ci, *args, **kw)
    _compare(got, ref, EVERYTHING)
    assert torch.equal(got["running_mean"], bn.mean) and torch.equal(got["running_var"], bn.var)


# --------------------------------------------------------------------------------- launch structure
def test_one_pool_entry_per_state_forward_and_backward(monkeypatch):
    """A 3-node cell has 9 edges over 4 states (s0, s1, node 0, node 1): 4 pool entries each way,
    in one launch per node."""
    from katib_amd.ops import hip_darts as hd

    layout, W = _layout(ALL, 4, 3)
    seen = {"pool_fwd_multi": [], "pool_bwd_multi": []}
    real = hd._launch

    def launch(name, calls, *args):
        if name in seen and calls:
            seen[name].append(len(calls))
            if name == "pool_bwd_multi":
                seen.setdefault("sources", []).append(sorted(len(c[9]) for c in calls))
        return real(name, calls, *args)

    monkeypatch.setattr(hd, "_launch", launch)
    _run_cell("hip", layout, W, 0, *_cell_inputs(layout, 0))
    assert seen["pool_fwd_multi"] == [2, 1, 1]  # node 0: s0 and s1; node 1: node 0; node 2: node 1
    assert seen["pool_bwd_multi"] == [1, 1, 2]  # after node 2: node 1; after node 1: node 0; after node 0: s0, s1
    assert seen["sources"] == [[1], [2], [3, 3]]
