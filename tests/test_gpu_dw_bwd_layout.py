"""Depthwise plane kernels (``dw_bwd_multi``, ``dwpw_fwd_multi``) against an fp64 PyTorch reference
at the shapes where the LDS tile map of the stride-1 paths can go wrong: bands shorter than the
8-row cell (N = 2 makes the launcher cut 8 bands per image: 1-, 2- and 4-row bands), a width the
2-quad cell does not divide (W = 12: the generic loops), two channel groups (C = 8), every
(K, dilation, stride, input-BN) variant, mixed-variant launches as a node issues them, and one
launch at the workload's size (N = 128, 32 x 32) whose bands are taller than a cell and whose
entries differ in their workgroup counts.

The reference is autograd through ``conv2d(relu(x) or relu(bn(x)), groups=C)`` in fp64 on the CPU,
computed once per case. Tolerance as the mixed-edge tests: err <= 1e-4 + 1e-3 * max|ref|.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EPS = 1e-5
PLAIN = [(3, 1, 1), (3, 1, 2), (5, 1, 1), (5, 1, 2), (3, 2, 1), (3, 2, 2), (5, 2, 1), (5, 2, 2)]  # (K, dil, S)
PLAIN_S1 = [v for v in PLAIN if v[2] == 1]
PREBN = [(3, 1, 1), (5, 1, 1)]  # the separable second stages: input BN, stride 1

# (N, C, Ho = Wo, variants, input BN)
CASES = [(2, C, HW, PLAIN, False) for C in (4, 8) for HW in (8, 16, 32)]
CASES += [(2, C, HW, PREBN, True) for C in (4, 8) for HW in (8, 16, 32)]
CASES += [(3, 4, 12, PLAIN_S1, False), (3, 4, 12, PREBN, True), (3, 8, 12, PLAIN_S1, False)]
CASES += [(128, 4, 32, PLAIN_S1, False), (128, 4, 32, PREBN, True)]
# entries whose band counts (and so workgroup counts) differ inside one launch: at this size the
# LDS footprint alone sets the band count, and the stride-2 entries stage 64 x 64 inputs
CASES += [(128, 4, 32, [(3, 1, 1), (5, 2, 2), (5, 2, 1), (3, 1, 2)], False)]
IDS = ["N%d-C%d-%dx%d-%s-%s" % (n, c, hw, hw, "bn" if bn else "plain", "+".join("k%dd%ds%d" % t for t in v))
       for n, c, hw, v, bn in CASES]


def _close(got, ref, name):
    ref = ref.to(torch.float64)
    err = (got.detach().cpu().to(torch.float64) - ref).abs().max().item()
    bound = 1e-4 + 1e-3 * ref.abs().max().item()
    print("%s: max err %.3e (bound %.3e)" % (name, err, bound))
    assert err <= bound, "%s: max err %.3e > %.3e" % (name, err, bound)


def _bn_coeffs(x64):
    """(sum, sum of squares) per channel as the f64 statistics buffer a BN reference carries, and the
    (mean, 1 / std) the kernels derive from it."""
    cnt = x64.shape[0] * x64.shape[2] * x64.shape[3]
    s, s2 = x64.sum((0, 2, 3)), (x64 * x64).sum((0, 2, 3))
    mean = s / cnt
    var = (s2 / cnt - mean * mean).clamp_min(0)
    return torch.cat([s, s2]), mean, 1.0 / torch.sqrt(var + EPS), 1.0 / cnt


@functools.lru_cache(maxsize=None)
def _case(idx):
    """Inputs (fp32, CPU) and fp64 references of every entry of CASES[idx]."""
    N, C, HW, variants, bn = CASES[idx]
    g = torch.Generator().manual_seed(100 + idx)
    entries = []
    for K, dil, S in variants:
        H = HW * S
        x = torch.randn(N, C, H, H, generator=g)
        if bn:
            x = x * 1.5 + 0.3
        dw = torch.randn(C, 1, K, K, generator=g) * 0.3
        pw = torch.randn(C, C, 1, 1, generator=g) * 0.5
        dd = torch.randn(N, C, HW, HW, generator=g)
        x64 = x.double()
        sums, mean, inv, inv_count = _bn_coeffs(x64)
        y = ((x64 - mean.view(1, C, 1, 1)) * inv.view(1, C, 1, 1)) if bn else x64
        y = y.detach().requires_grad_(True)
        w64 = dw.double().requires_grad_(True)
        d = F.conv2d(torch.relu(y), w64, stride=S, padding=(K - 1) // 2 * dil, dilation=dil, groups=C)
        z = F.conv2d(d, pw.double())
        (d * dd.double()).sum().backward()
        gy = y.grad
        red = torch.cat([gy.sum((0, 2, 3)), (gy * y.detach()).sum((0, 2, 3))])
        stats = torch.cat([z.sum((0, 2, 3)), (z * z).sum((0, 2, 3))]).detach()
        entries.append(dict(K=K, dil=dil, S=S, x=x, dw=dw, pw=pw, dd=dd, sums=sums, inv_count=inv_count,
                            gy=gy, gw=w64.grad.reshape(-1), red=red, d=d.detach(), z=z.detach(), stats=stats))
    return entries


def _kernels():
    from katib_amd.ops import hip_darts as hd

    return hd._K, int(hd.REP), hd.ZDT


def _inbn(e, C, dev):
    return (e["sums"].to(dev), None, None, float(e["inv_count"]), False, EPS, 1, 2 * C)


@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_dw_bwd_multi_matches_fp64(idx):
    K_, REP, ZDT = _kernels()
    N, C, HW, variants, bn = CASES[idx]
    dev = torch.device("cuda", 0)
    calls, outs = [], []
    for e in _case(idx):
        x = e["x"].to(dev)
        gout = torch.full_like(x, float("nan"))  # every element must be written
        gW = torch.zeros(C * e["K"] * e["K"], device=dev)
        red = torch.zeros(REP * 2 * C, dtype=torch.float64, device=dev) if bn else None
        xin = x.to(ZDT) if bn else x
        calls.append((xin, _inbn(e, C, dev) if bn else None, e["dw"].to(dev), e["dd"].to(dev), gout, gW, red, 0,
                      not bn, e["K"], e["dil"], e["S"]))
        outs.append((gout, gW, red))
    K_.dw_bwd_multi(calls)
    torch.cuda.synchronize()
    for e, (gout, gW, red) in zip(_case(idx), outs):
        tag = "K%d dil%d S%d" % (e["K"], e["dil"], e["S"])
        _close(gout, e["gy"], tag + " input gradient")
        _close(gW, e["gw"], tag + " depthwise weight gradient")
        if bn:
            _close(red.view(REP, 2 * C).sum(0), e["red"], tag + " red sums")


@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_dwpw_fwd_multi_matches_fp64(idx):
    K_, REP, ZDT = _kernels()
    N, C, HW, variants, bn = CASES[idx]
    dev = torch.device("cuda", 0)
    calls, outs = [], []
    for e in _case(idx):
        x = e["x"].to(dev)
        d = torch.full((N, C, HW, HW), float("nan"), device=dev, dtype=ZDT)
        z = torch.full((N, C, HW, HW), float("nan"), device=dev, dtype=ZDT)
        stats = torch.zeros(REP * 2 * C, dtype=torch.float64, device=dev)
        xin = x.to(ZDT) if bn else x
        calls.append((xin, e["dw"].to(dev), e["pw"].reshape(C, C).contiguous().to(dev), _inbn(e, C, dev) if bn else None,
                      d, z, stats, e["K"], e["dil"], e["S"], (e["K"] - 1) // 2 * e["dil"]))
        outs.append((d, z, stats))
    K_.dwpw_fwd_multi(calls)
    torch.cuda.synchronize()
    for e, (d, z, stats) in zip(_case(idx), outs):
        tag = "K%d dil%d S%d" % (e["K"], e["dil"], e["S"])
        _close(d.float(), e["d"], tag + " depthwise output d")
        _close(z.float(), e["z"], tag + " pointwise output z")
        _close(stats.view(REP, 2 * C).sum(0), e["stats"], tag + " BN statistics")
