"""The GPT-2 kernel oracle (tests/gpt2_kernel_oracle.py) checked without a GPU: every fp64 truth
function against an independent torch formulation, the reference arm and TorchOps through the per-row
checker, and the checker itself against mutants it has to turn down at the default margin."""
import math

import pytest
import torch
import torch.nn.functional as F

import gpt2_kernel_oracle as O
from katib_amd.ops.transformer import TorchOps

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16


def _gen(seed=3):
    return torch.Generator().manual_seed(seed)


def _same(a, b, tol=1e-9):
    """The fp64 truth against an fp64 formulation from torch itself: far inside fp32 round-off."""
    a, b = a.to(F64), b.to(F64)
    d = float((a - b).detach().abs().max())
    assert d <= tol * max(float(b.detach().abs().max()), 1e-30), d


def _old_rel(a, b):
    """The metric the kernel tests used before: one number per tensor."""
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


# ------------------------------------------------------------------------------ shared inputs
def _ln_inputs(M, D, seed=3, big_mean=False):
    g = _gen(seed)
    x = torch.randn(M, D, generator=g) * (0.5 if big_mean else 2.0) + (300.0 if big_mean else 0.5)
    r = torch.randn(M, D, generator=g).to(BF16)
    gamma = (1 + 0.1 * torch.randn(D, generator=g)).to(BF16)
    beta = (0.1 * torch.randn(D, generator=g)).to(BF16)
    dy = torch.randn(M, D, generator=g).to(BF16)
    G0 = torch.randn(M, D, generator=g)
    return x, r, gamma, beta, dy, G0


_attn = {}


def _attn_case(B, T, H):
    """qkv, dout and both arms' forward and backward, computed once per shape and never modified. The
    backward of both arms takes the same given bf16 output, the reference arm's."""
    key = (B, T, H)
    if key not in _attn:
        g = _gen(B * T + H)
        qkv = torch.randn(B * T, 3 * H * 64, generator=g).to(BF16)
        do = torch.randn(B * T, H * 64, generator=g).to(BF16)
        ot, lt = O.TRUTH.attn_fwd(qkv, B, T, H)
        orf, lr = O.REF.attn_fwd(qkv, B, T, H)
        _attn[key] = {"qkv": qkv, "do": do, "o": (orf, ot), "lse": (lr, lt),
                      "d": (O.REF.attn_bwd(qkv, orf, do, B, T, H), O.TRUTH.attn_bwd(qkv, orf, do, B, T, H)),
                      "auto": (O.REF.attn_bwd_autograd(qkv, do, B, T, H), O.TRUTH.attn_bwd_autograd(qkv, do, B, T, H))}
    return _attn[key]


def _adamw_run(arm, p0, grads, lr=1e-2, wd=0.1, max_norm=1.0, **mutant):
    p, m, v = p0, torch.zeros_like(p0), torch.zeros_like(p0)
    for t, g in enumerate(grads, 1):
        p, m, v, w16 = arm.adamw(p, g, m, v, lr, t, 0.9, 0.95, 1e-8, wd, max_norm, **mutant)
    return p, m, v, w16


# ------------------------------------------------------------------------------ the oracle is right
@pytest.mark.parametrize("residual", [False, True])
def test_truth_layernorm(residual):
    M, D = 37, 256
    x, r, gamma, beta, dy, G0 = _ln_inputs(M, D)
    xin, y, mean, rstd = O.TRUTH.ln_fwd(x, r if residual else None, gamma, beta)
    with torch.enable_grad():
        xi = (x.double() + (r.double() if residual else 0)).requires_grad_(True)
        ga, be = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
        yy = F.layer_norm(xi, (D,), ga, be, 1e-5)
        dx, dga, dbe = torch.autograd.grad(yy, (xi, ga, be), dy.double())
    _same(xin, xi)
    _same(y, yy)
    _same(mean, xi.mean(-1))
    _same(rstd, (xi.var(-1, unbiased=False) + O.r32(1e-5)).rsqrt())
    for acc in (True, False):
        b = O.TRUTH.ln_bwd(dy, xin.float(), mean.float(), rstd.float(), gamma, G0, accumulate=acc)
        # the backward takes the fp32 statistics as inputs: the comparison is at fp32 round-off of those
        _same(b["G"], dx + (G0.double() if acc else 0), 1e-5)
        _same(b["dgamma"], dga, 1e-5)
        _same(b["dbeta"], dbe)
        _same(b["dr"], b["G"], 0.0)
        _same(b["dbias"], b["G"].to(BF16).double().sum(0), 0.0)


def test_truth_gelu():
    g = _gen()
    u = (torch.rand(4096, generator=g) * 24 - 12).to(BF16)
    dy = torch.randn(4096, generator=g).to(BF16)
    with torch.enable_grad():
        x = u.double().requires_grad_(True)
        y = F.gelu(x, approximate="tanh")
        (dx,) = torch.autograd.grad(y, x, dy.double())
    _same(O.TRUTH.gelu_fwd(u), y)
    _same(O.TRUTH.gelu_bwd(u, dy), dx)


def test_truth_cross_entropy():
    g = _gen()
    N, V, Vp = 9, 1000, 1024
    logits = (torch.randn(N, Vp, generator=g) * 3).to(BF16)
    logits[:, V:] = 100.0
    tgt = torch.randint(0, V, (N,), generator=g)
    logits[0, 17] = logits[0, 400] = 30.0  # a tie: the lowest index is the argmax
    tgt[0] = 17
    with torch.enable_grad():
        x = logits[:, :V].double().requires_grad_(True)
        loss = F.cross_entropy(x, tgt, reduction="none")
        (dx,) = torch.autograd.grad(loss.sum() * (O.r32(0.7) / N), x)
    lt, st = O.TRUTH.xent_fwd(logits, tgt, V)
    _same(lt, loss)
    _same(st, torch.logsumexp(logits[:, :V].double(), -1))
    d = O.TRUTH.xent_bwd(logits, tgt, 0.7, V)
    _same(d[:, :V], dx)
    assert float(d[:, V:].abs().max()) == 0.0
    le, hit = O.TRUTH.xent_eval(logits, tgt, V)
    _same(le, loss)
    assert torch.equal(hit.bool(), logits[:, :V].double().argmax(-1) == tgt) and bool(hit[0])


@pytest.mark.parametrize("B,T,H", [(1, 128, 1), (2, 256, 2)])
def test_truth_attention(B, T, H):
    c = _attn_case(B, T, H)
    with torch.enable_grad():
        x = c["qkv"].double().requires_grad_(True)
        q, k, v = x.view(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)
        o = F.scaled_dot_product_attention(q, k, v, is_causal=True).permute(0, 2, 1, 3).reshape(B * T, H * 64)
        (dx,) = torch.autograd.grad(o, x, c["do"].double())
    _same(c["o"][1], o)
    _same(c["auto"][1], dx)
    # the flash algebra with delta = rowsum(dO * o) is that derivative when o is the exact output ...
    _same(O.TRUTH.attn_bwd(c["qkv"], c["o"][1], c["do"], B, T, H), dx)
    # ... and what it gives for the bf16 output it is handed differs by the rounding of o only: for dQ
    # and dK by |dS - dS'| <= P |dO| |o - o'|, a bf16 ulp of the output
    diff = (c["d"][1] - dx).abs().max() / dx.abs().max()
    assert 0 < float(diff) < 2.0 ** -6, float(diff)
    s = (q @ k.transpose(-1, -2)).detach() / 8.0
    s = s.masked_fill(torch.ones(T, T, dtype=torch.bool).triu(1), float("-inf"))
    _same(c["lse"][1], torch.logsumexp(s, -1) * O.LOG2E)


@pytest.mark.parametrize("gscale", [1.0, 1e-4])  # the clip active / inactive
def test_truth_adamw(gscale):
    g = _gen()
    n = 1000
    p0 = torch.randn(n, generator=g)
    grads = [(torch.randn(n, generator=g) * gscale).to(BF16) for _ in range(3)]
    p = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.AdamW([p], lr=O.r32(1e-2), betas=(O.r32(0.9), O.r32(0.95)), eps=O.r32(1e-8),
                            weight_decay=O.r32(0.1))
    for gr in grads:
        p.grad = gr.double().clone()
        norm = torch.nn.utils.clip_grad_norm_([p], 1.0)
        assert (float(norm) > 1.0) == (gscale == 1.0)
        opt.step()
    pt, mt, vt, w16 = _adamw_run(O.TRUTH, p0, grads)
    _same(pt, p.detach())
    _same(mt, opt.state[p]["exp_avg"])
    _same(vt, opt.state[p]["exp_avg_sq"])
    assert torch.equal(w16, pt.to(BF16))


def test_truth_sums():
    g = _gen()
    x = torch.randn(77, 40, generator=g).to(BF16)
    part = torch.randn(9, 260, generator=g)
    _same(O.TRUTH.colsum(x), x.double().sum(0))
    _same(O.TRUTH.reduce_rows(part), part.double().sum(0))
    _same(O.TRUTH.ln_reduce(part), part.double().sum(0))
    _same(O.TRUTH.grad_sumsq(x), x.double().norm() ** 2)


# ------------------------------------------------------------------------------ the reference arm and TorchOps
def test_reference_arm_and_torchops_pass():
    """The reference arm passes at margin 1 by construction (it is its own bound); TorchOps, the
    project's CPU path, has to pass at the default margin like any implementation."""
    t = TorchOps()
    M, D = 37, 256
    x, r, gamma, beta, dy, G0 = _ln_inputs(M, D)
    ref, tru = O.REF.ln_fwd(x, r, gamma, beta), O.TRUTH.ln_fwd(x, r, gamma, beta)
    got = t.ln_fwd(x, r, gamma, beta)
    for k, name in enumerate(("xin", "y", "mean", "rstd")):
        a, b, c = (z[k].reshape(M, -1) for z in (got, ref, tru))
        O.assert_rows_close(b, b, c, margin=1)
        O.assert_rows_close(a, b, c, what="torchops ln " + name)
    xin, _, mean, rstd = ref
    rb, tb = (arm.ln_bwd(dy, xin, mean, rstd, gamma, G0) for arm in (O.REF, O.TRUTH))
    G, dr = G0.clone(), torch.empty(M, D, dtype=BF16)
    dg, db, dbias = (torch.empty(D, dtype=BF16) for _ in range(3))
    t.ln_bwd(dy, xin, mean, rstd, gamma, G, dr, dg, db, dbias=dbias)
    for name, a in (("G", G), ("dr", dr), ("dgamma", dg), ("dbeta", db), ("dbias", dbias)):
        row = D if a.dim() == 2 else 64
        O.assert_rows_close(rb[name], rb[name], tb[name], margin=1, row=row)
        O.assert_rows_close(a, rb[name], tb[name], row=row, what="torchops ln_bwd " + name)

    c = _attn_case(2, 256, 2)
    B, T, H = 2, 256, 2
    o, lse = t.attn_fwd(c["qkv"], B, T, H)
    O.assert_rows_close(O.head_rows(c["o"][0], B, T, H), O.head_rows(c["o"][0], B, T, H), O.head_rows(c["o"][1], B, T, H),
                        margin=1)
    O.assert_rows_close(O.head_rows(o, B, T, H), O.head_rows(c["o"][0], B, T, H), O.head_rows(c["o"][1], B, T, H),
                        what="torchops attn o")
    O.assert_rows_close(lse.reshape(-1, 1), c["lse"][0].reshape(-1, 1), c["lse"][1].reshape(-1, 1),
                        what="torchops attn lse")
    d = t.attn_bwd(c["qkv"], o, c["do"], lse, B, T, H)  # autograd: it never reads o
    for part in range(3):
        b, tt = (O.head_rows(z, B, T, H, part) for z in c["d"])
        O.assert_rows_close(b, b, tt, margin=1)
        a, b, tt = (O.head_rows(z, B, T, H, part) for z in (d, c["auto"][0], c["auto"][1]))
        O.assert_rows_close(a, b, tt, what="torchops attn d%s" % "qkv"[part])

    g = _gen(5)
    u = (torch.rand(4096, generator=g) * 24 - 12).to(BF16)
    dyu = torch.randn(4096, generator=g).to(BF16)
    O.assert_rows_close(t.gelu_fwd(u), O.REF.gelu_fwd(u), O.TRUTH.gelu_fwd(u), what="torchops gelu_fwd")
    O.assert_rows_close(t.gelu_bwd(u, dyu), O.REF.gelu_bwd(u, dyu), O.TRUTH.gelu_bwd(u, dyu), what="torchops gelu_bwd")

    N, V, Vp = 9, 1000, 1024
    logits = (torch.randn(N, Vp, generator=g) * 3).to(BF16)
    tgt = torch.randint(0, V, (N,), generator=g)
    loss, lse = t.xent_fwd(logits, tgt, V)
    (lr, sr), (lt, st) = O.REF.xent_fwd(logits, tgt, V), O.TRUTH.xent_fwd(logits, tgt, V)
    O.assert_rows_close(loss.reshape(-1, 1), lr.reshape(-1, 1), lt.reshape(-1, 1), what="torchops xent loss")
    O.assert_rows_close(lse.reshape(-1, 1), sr.reshape(-1, 1), st.reshape(-1, 1), what="torchops xent lse")
    gs = torch.full((1,), 0.7)
    O.assert_rows_close(t.xent_bwd(logits.clone(), tgt, lse, gs, V), O.REF.xent_bwd(logits, tgt, 0.7, V),
                        O.TRUTH.xent_bwd(logits, tgt, 0.7, V), what="torchops xent grad")

    n = 1000
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g).to(BF16) for _ in range(3)]
    p, m, v, w16 = p0.clone(), torch.zeros(n), torch.zeros(n), torch.empty(n, dtype=BF16)
    lr_t, step, ss = torch.full((1,), 1e-2), torch.zeros(1), torch.zeros(1)
    for gr in grads:
        step += 1
        t.adamw(p, gr, m, v, w16, lr_t, step, 0.9, 0.95, 1e-8, 0.1, 1.0, ss)
    rr, tt = _adamw_run(O.REF, p0, grads), _adamw_run(O.TRUTH, p0, grads)
    for k, (name, a) in enumerate((("p", p), ("m", m), ("v", v))):
        O.assert_rows_close(rr[k], rr[k], tt[k], margin=1)
        O.assert_rows_close(a, rr[k], tt[k], what="torchops adamw " + name)


def test_checker_floor_and_report():
    """A row whose truth is exactly zero (row 0 of dQ: one key, dS = 0) is judged against one ulp of
    the tensor's maximum instead of dividing by zero, and a failure names the worst row."""
    truth = torch.zeros(4, 64, dtype=F64)
    truth[1:] = torch.randn(3, 64, generator=_gen(), dtype=F64)
    ref = truth.to(BF16)
    assert float(O.row_err(ref, truth, O.ULP[BF16])[0]) == 0.0
    O.assert_rows_close(ref, ref, truth, margin=1)
    bad = ref.clone()
    bad[0, 5] = 0.25
    rep = O.rejects(bad, ref, truth)
    assert rep is not None and rep["row"] == 0 and rep["failing"] == 1
    with pytest.raises(AssertionError, match="worst row 0"):
        O.assert_rows_close(bad, ref, truth)
    with pytest.raises(AssertionError, match="non-finite"):
        O.assert_rows_close(torch.full_like(ref, float("nan")), ref, truth)


# ------------------------------------------------------------------------------ the checker can fail
@pytest.mark.parametrize("B,T,H", [(1, 128, 1), (2, 256, 2), (1, 384, 3)])
def test_mutant_causal_mask_off_by_one(B, T, H):
    c = _attn_case(B, T, H)
    bad = O.REF.attn_fwd(c["qkv"], B, T, H, diag=2)[0]  # key q + 1 visible
    # the metric this replaces: _rel(bad, truth) = 1.31 / 0.54 / 0.76 at these shapes (caught there
    # too: the per-row checker must not lose what the old one saw)
    print("old _rel %.3g" % _old_rel(bad, c["o"][1]))
    rep = O.rejects(*(O.head_rows(z, B, T, H) for z in (bad, c["o"][0], c["o"][1])))
    assert rep is not None and rep["failing"] > 0.5 * rep["rows"], rep


@pytest.mark.parametrize("B,T,H", [(1, 128, 1), (2, 256, 2), (1, 384, 3), (1, 512, 2)])
def test_mutant_late_query_rows_scaled(B, T, H):
    c = _attn_case(B, T, H)
    bad = c["o"][0].clone().view(B, T, H * 64)
    bad[:, T - 32:] = (bad[:, T - 32:].float() * 1.05).to(BF16)
    # the metric this replaces: _rel(bad, truth) = 0.0109 / 0.0066 / 0.0052 / 0.0068 at these shapes,
    # all under its 2e-2 bound - late rows average many values and are small beside row 0
    old = _old_rel(bad.view(B * T, H * 64), c["o"][1])
    print("old _rel %.3g" % old)
    assert old < 2e-2
    rep = O.rejects(*(O.head_rows(z, B, T, H) for z in (bad.view(B * T, H * 64), c["o"][0], c["o"][1])))
    assert rep is not None and rep["err"] > 0.04 and rep["bound"] < 0.03, rep


@pytest.mark.parametrize("part", [0, 1])
@pytest.mark.parametrize("B,T,H", [(1, 128, 1), (2, 256, 2), (3, 256, 2), (1, 384, 3), (1, 512, 2)])
def test_mutant_late_rows_of_dq_dk_scaled(B, T, H, part):
    """The last 32 rows of dQ (dK) times 1.05, and that the bound that rejects it stays where the
    reference arm's rounding puts it: about 2^-6 of each row's own maximum."""
    c = _attn_case(B, T, H)
    bad = c["d"][0].clone()
    v = bad.view(B, T, 3, H, 64)
    v[:, T - 32:, part] = (v[:, T - 32:, part].float() * 1.05).to(BF16)
    rep = O.rejects(*(O.head_rows(z, B, T, H, part) for z in (bad, c["d"][0], c["d"][1])))
    assert rep is not None and rep["failing"] >= 16 * B * H and rep["bound"] < 0.04, rep


def test_mutant_dv_of_the_last_keys_zeroed():
    B, T, H = 1, 512, 2
    c = _attn_case(B, T, H)
    bad = c["d"][0].clone()
    bad.view(B, T, 3, H, 64)[:, T - 64:, 2] = 0
    assert _old_rel(O.head_rows(bad, B, T, H, 2), O.head_rows(c["d"][1], B, T, H, 2)) < 3e-2  # the old bound
    rep = O.rejects(*(O.head_rows(z, B, T, H, 2) for z in (bad, c["d"][0], c["d"][1])))
    assert rep is not None and rep["failing"] >= 64 * H - 2, rep
    for part in (0, 1):  # dQ and dK are untouched and pass
        O.assert_rows_close(*(O.head_rows(z, B, T, H, part) for z in (bad, c["d"][0], c["d"][1])))


def test_mutant_one_pass_variance():
    M, D = 16, 256
    x, _, gamma, beta, _, _ = _ln_inputs(M, D, big_mean=True)
    ref, tru = O.REF.ln_fwd(x, None, gamma, beta), O.TRUTH.ln_fwd(x, None, gamma, beta)
    mu = x.mean(-1)
    rstd = torch.rsqrt(((x * x).mean(-1) - mu * mu).clamp_min(0) + 1e-5)  # E[x^2] - mu^2 in fp32
    y = ((x - mu[:, None]) * rstd[:, None] * gamma.float() + beta.float()).to(BF16)
    O.assert_rows_close(ref[1], ref[1], tru[1], margin=1)
    assert O.rejects(y, ref[1], tru[1]) is not None
    assert O.rejects(rstd.reshape(-1, 1), ref[3].reshape(-1, 1), tru[3].reshape(-1, 1)) is not None


def _xent_case():
    g = _gen(7)
    N, V, Vp = 5, 1000, 1024
    logits = (torch.randn(N, Vp, generator=g) * 3).to(BF16)
    logits[:, V:] = 0.0  # a pad value a forgotten mask would not shout about
    tgt = torch.randint(0, V, (N,), generator=g)
    tgt[4] = V - 1
    return N, V, Vp, logits, tgt


def test_mutant_xent_target_in_the_last_column():
    N, V, Vp, logits, tgt = _xent_case()
    ref, tru = O.REF.xent_bwd(logits, tgt, 0.7, V), O.TRUTH.xent_bwd(logits, tgt, 0.7, V)
    bad = ref.clone()
    bad[4, V - 1] = (bad[4, V - 1].float() + O.r32(0.7) / N).to(BF16)  # the -1 at the target dropped
    rep = O.rejects(bad, ref, tru)
    assert rep is not None and rep["row"] == 4 and rep["failing"] == 1


def test_mutant_xent_pad_column_in_lse():
    N, V, Vp, logits, tgt = _xent_case()
    (lr, sr), (lt, st) = O.REF.xent_fwd(logits, tgt, V), O.TRUTH.xent_fwd(logits, tgt, V)
    lb, sb = O.REF.xent_fwd(logits, tgt, V + 1)  # one pad column counted
    assert O.rejects(sb.reshape(-1, 1), sr.reshape(-1, 1), st.reshape(-1, 1)) is not None
    assert O.rejects(lb.reshape(-1, 1), lr.reshape(-1, 1), lt.reshape(-1, 1)) is not None


@pytest.mark.parametrize("mutant", ["bias_correction", "clip", "decay_first"])
def test_mutant_adamw(mutant):
    g = _gen()
    n = 2048
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g).to(BF16) for _ in range(3)]  # norm ~45: the clip is active
    ref, tru = _adamw_run(O.REF, p0, grads), _adamw_run(O.TRUTH, p0, grads)
    bad = _adamw_run(O.REF, p0, grads, **{mutant: False})
    O.assert_rows_close(ref[0], ref[0], tru[0], margin=1)
    assert O.rejects(bad[0], ref[0], tru[0]) is not None, mutant


def test_mutant_argmax_tie_to_the_higher_index():
    N, V, Vp, logits, tgt = _xent_case()
    logits = logits.clone()
    logits[:, 561] = logits[:, 700] = 40.0
    tgt = tgt.clone()
    tgt[:3], tgt[3:] = 561, 700
    (_, hr), (_, ht) = O.REF.xent_eval(logits, tgt, V), O.TRUTH.xent_eval(logits, tgt, V)
    assert hr.tolist() == [1.0, 1.0, 1.0, 0.0, 0.0] and torch.equal(hr.double(), ht)
    bad = O.REF.xent_eval(logits, tgt, V, lowest=False)[1]
    rep = O.rejects(bad.reshape(-1, 1), hr.reshape(-1, 1), ht.reshape(-1, 1))
    assert rep is not None and rep["failing"] == N


def test_mutant_dbias_from_the_fp32_gradient():
    """dbias is the column sum of the bf16 tensor dr (what a colsum pass over dr would give). In a
    column where +1.00366 (bf16: 1.0) and -1.0 alternate, that sum is 0 and the sum of the fp32 G is
    0.00366 M / 2; beside a column of sum 100 that is far over a bf16 ulp."""
    M, D = 2048, 256
    G0 = torch.zeros(M, D)
    G0[0::2, 1:] = 1.00366
    G0[1::2, 1:] = -1.0
    G0[:100, 0] = 1.0
    G0[:, 64:] = G0[:, :64].repeat(1, 3)
    x, _, gamma, _, _, _ = _ln_inputs(M, D)
    dy = torch.zeros(M, D, dtype=BF16)  # dx = 0: G' = G0 exactly in every arm
    _, _, mean, rstd = O.REF.ln_fwd(x, None, gamma, gamma)
    ref, tru = (arm.ln_bwd(dy, x, mean, rstd, gamma, G0) for arm in (O.REF, O.TRUTH))
    assert float(tru["dbias"][0]) == 100.0 and float(tru["dbias"][1:64].abs().max()) == 0.0
    O.assert_rows_close(ref["dbias"], ref["dbias"], tru["dbias"], margin=1, row=64)
    bad = O.REF.ln_bwd(dy, x, mean, rstd, gamma, G0, dbias_from_g=True)["dbias"]
    rep = O.rejects(bad, ref["dbias"], tru["dbias"], row=64)
    assert rep is not None and rep["failing"] == D // 64, rep


def test_mutant_ln_bwd_rows_from_1024_unwritten():
    M, D = 1029, 256
    x, r, gamma, beta, dy, G0 = _ln_inputs(M, D)
    xin, _, mean, rstd = O.REF.ln_fwd(x, r, gamma, beta)
    ref, tru = (arm.ln_bwd(dy, xin, mean, rstd, gamma, G0) for arm in (O.REF, O.TRUTH))
    for name, stale in (("G", G0), ("dr", torch.full((M, D), 7.0, dtype=BF16))):
        bad = ref[name].clone()
        bad[1024:] = stale[1024:]
        rep = O.rejects(bad, ref[name], tru[name], row=D)
        assert rep is not None and rep["failing"] == 5 and rep["row"] >= 1024, (name, rep)
    # and their contribution missing from the parameter gradients
    bad = (dy[:1024].float() * ((xin[:1024] - mean[:1024, None]) * rstd[:1024, None])).sum(0).to(BF16)
    assert O.rejects(bad, ref["dgamma"], tru["dgamma"], row=64) is not None
