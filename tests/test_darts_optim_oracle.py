"""The oracles of tests/darts_optim_oracle.py, validated without a GPU: the exact-order fp32
oracle (a) against the fp64 mathematics (b) to fp32 rounding, and against the torch branches of
DartsSearch (K is None) run on CPU tensors, which the project's parity tests already trust."""
import pytest
import torch

import darts_optim_oracle as O

F32, F64 = torch.float32, torch.float64
MU, WD, CLIP, LR = 0.9, 3e-4, 5.0, 0.025
PRIMS = ["separable_convolution_3x3", "dilated_convolution_3x3", "avg_pooling_3x3", "max_pooling_3x3",
         "skip_connection"]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _r(x):
    return float(O.s32(x))


# ------------------------------------------------------------------ (a) against (b)
@pytest.mark.parametrize("n", [1, 257, 100003])
def test_virtual_step_matches_fp64(n):
    """Three roundings in v (each <= ulp(v) / 2, scaled by lr), the product and the final add:
    inside 2 ulp of max |w'|."""
    g = _gen(n)
    w, mom, gr = torch.randn(n, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g)
    got = O.virtual_step(w, mom, gr, LR, MU, WD)
    want = O.virtual_step64(w, mom, gr, _r(LR), _r(MU), _r(WD))
    assert got.dtype == F32 and O.ulp_err(got, want) <= 2.0
    # the one-op rule matters: the FMA form differs from the oracle somewhere at this size
    if n == 100003:
        fused = (mom * O.s32(MU) + gr).add(w, alpha=_r(WD)).mul(-O.s32(LR)).add(w)
        assert int((fused != got).sum()) > 0


@pytest.mark.parametrize("scale", [10.0, 0.1, 0.0], ids=["clipped", "unclipped", "zero"])
@pytest.mark.parametrize("n", [1, 2049, 100003])
def test_sgd_clip_matches_fp64(n, scale):
    """Against clip_grad_norm_ + torch.optim.SGD in fp64: the norm, the divide, the product with
    coef and four more roundings, inside 4 ulp of each output's max magnitude."""
    g = _gen(n + 1)
    w, mom, gr = torch.randn(n, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g)
    gr = gr * (scale * CLIP / max(float(gr.norm()), 1e-30))
    coef = float(O.clip_coef(gr, CLIP))
    assert (coef < 0.11) if scale == 10.0 else (coef == 1.0)
    got = O.sgd_clip(w, gr, mom, LR, CLIP, MU, WD)
    want = O.sgd_clip64(w, gr, mom, _r(LR), _r(CLIP), _r(MU), _r(WD))
    for a, b, name in zip(got, want, ("w", "g", "mom")):
        assert a.dtype == F32 and O.ulp_err(a, b) <= 4.0, (name, O.ulp_err(a, b))


@pytest.mark.parametrize("n,na", [(1, 1), (2049, 112), (100003, 257)])
def test_hessian_matches_architect_closed_forms(n, na):
    g = _gen(n + 2)
    w, d = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.3
    gap, ga, gav = (torch.randn(na, generator=g) for _ in range(3))
    ga = gap + 1e-3 * ga  # finite differences: d+ and d- nearly cancel
    eps = O.eps_of(d)
    eps64, wp64, wm64, ag64 = O.architect64(w, d, gap, ga, gav, _r(LR))
    assert abs(float(eps) / float(eps64) - 1.0) <= 2 * O.ULP  # fp32 norm, 0.01f, divide
    w0 = O.hessian_step(0, w, d, eps)
    w1 = O.hessian_step(1, w0, d, eps)
    w2 = O.hessian_step(2, w1, d, eps)
    wp, wm = O.hessian_split(w, d, eps)
    assert torch.equal(wp, w0) and torch.equal(wm, w1)  # the concurrent form keeps the sequential rounding
    assert O.ulp_err(w0, wp64) <= 2.0 and O.ulp_err(w1, wm64) <= 3.0 and O.ulp_err(w2, w.to(F64)) <= 3.0
    # gap - ga is exact up to one rounding of the difference; relative to max |alpha_grad|
    got = O.hessian_alpha_grad(gap, ga, gav, eps, LR)
    exact = gav.to(F64) - _r(LR) * ((gap - ga).to(F64) / (2.0 * float(eps)))  # same eps, same difference
    assert O.ulp_err(got, exact) <= 3.0
    rel = float((got.to(F64) - ag64).abs().max() / ag64.abs().max())
    assert rel <= 8 * O.ULP * max(1.0, float((gap.abs().max() / (gap - ga).abs().max())))  # the cancellation


def test_bn_merge_matches_fp64():
    g = _gen(5)
    bn, bp, bz = (torch.randn(300, generator=g) for _ in range(3))
    want = (1.0 - _r(0.1)) * bp.to(F64) + bn.to(F64) - (1.0 - _r(0.1)) * bz.to(F64)
    assert O.ulp_err(O.bn_merge(bn, bp, bz, 0.1), want) <= 4.0


@pytest.mark.parametrize("K", [1, 7, 8, 16])
def test_fp32_softmax_stays_inside_the_derived_bound(K):
    for kind, x in O.softmax_inputs(600, K, seed=K).items():
        want = O.softmax64(x)
        got = torch.softmax(x, dim=-1)
        rel = float(((got.to(F64) - want).abs() / want).max())
        print("K %d %s: fp32 torch.softmax rel err %.3g, bound %.3g" % (K, kind, rel, O.softmax_tol(K)))
        assert rel <= O.softmax_tol(K), (kind, rel)
        assert float((got.to(F64).sum(-1) - 1.0).abs().max()) <= O.softmax_tol(K)


@pytest.mark.parametrize("K", [1, 7, 16])
def test_alpha_grad_formula_is_the_softmax_jacobian(K):
    """alpha_grad64 against autograd through torch.softmax in fp64: entries sharing a row add."""
    g, rep, rows = _gen(K), 4, 3
    a = torch.randn(rows, K, generator=g, dtype=F64, requires_grad=True)
    w = torch.softmax(a, dim=-1)
    entries, loss = [], 0.0
    for e in range(7):
        r = e % rows
        gr = torch.randn(rep * (K + 3), generator=g, dtype=F64)
        entries.append((gr, K + 3, w[r].detach(), r))
        loss = loss + (w[r] * sum(gr[q * (K + 3):q * (K + 3) + K] for q in range(rep))).sum()
    loss.backward()
    got = O.alpha_grad64(entries, rep, K)
    for r in range(rows):
        assert torch.allclose(got[r].to(F64), a.grad[r], rtol=0, atol=4 * O.ULP * float(a.grad.abs().max()))


def test_alpha_grad_dyadic_inputs_are_exact_in_fp64():
    """w multiples of 2^-8 in [0, 1], replicas multiples of 2^-10 below 2^10, 32 replicas, K = 16,
    128 entries on one row: the fp64 formula equals integer arithmetic, so no fp64 operation rounds
    and the device's order cannot matter."""
    g, rep, K, ne = _gen(9), 32, 16, 128
    wi = torch.randint(0, 257, (ne, K), generator=g)
    gi = torch.randint(-(2 ** 20) + 1, 2 ** 20, (ne, rep, K), generator=g)
    gs = gi.sum(1)  # < 2^25
    exact = (wi * (gs * 256 - (wi * gs).sum(1, keepdim=True))).sum(0)  # scaled by 2^8 * 2^8 * 2^10
    assert int(exact.abs().max()) < 2 ** 62
    entries = [((gi[e].to(F64) / 1024.0).reshape(-1), K, (wi[e].to(F64) / 256.0).to(F32), 0) for e in range(ne)]
    got = O.alpha_grad64(entries, rep, K)[0]
    assert torch.equal(got, (exact.to(F64) / 2.0 ** 26).to(F32))
    assert bool((exact.abs() < 2 ** 53).all())  # ... and the exact value fits an fp64


def test_dyadic_sum_of_squares_is_exact_in_any_order():
    n = 600000
    x = O.dyadic(n, _gen(1))
    exact = int((torch.round(x.to(F64) * 64).to(torch.int64) ** 2).sum())
    assert float(O.sumsq_total(x)) * 4096.0 == float(exact) and exact < 2 ** 53
    perm = torch.randperm(n, generator=_gen(2))
    parts = x[perm].to(F64).square().view(-1, 64).sum(1).flip(0)
    assert float(parts.sum()) == float(O.sumsq_total(x))


def test_partial_counts_and_the_norm_precondition():
    assert [O.sumsq_nparts(n) for n in (1, 2048, 2049, 262144 + 257, 524288, 524288 + 4099, 2 ** 30)] == \
        [1, 1, 2, 129, 256, 256, 256]
    bad = 0
    for s in range(400):
        bad += not O.norm_is_stable(torch.randn(2049, generator=_gen(s)))
    assert bad <= 40  # a few percent of random totals sit near an fp32 rounding boundary
    x, s = O.first_stable(lambda g: torch.randn(2049, generator=g), 0)
    assert O.norm_is_stable(x)


@pytest.mark.parametrize("t0", [0, 1000])
def test_adam_fp32_branch_against_fp64_adam(t0):
    """The fp32 arithmetic of the torch branch against torch.optim.Adam in fp64 (hyperparameters
    rounded to fp32 first), from the same fp32 state at every step. Where the branch may differ:
    * it rounds the double 1 - 0.999 to fp32 where the reference (and the kernel) take
      1 - float32(0.999): a relative ``kb2`` = 1.3e-5 on the new term of v, half of it after the root;
    * b2^t carries up to half an ulp of 1 (2^-24), which bc2 = 1 - b2^t magnifies by 1 / bc2;
    * about 16 roundings of half an ulp on the way to the update, and the stored alpha's own
      rounding, ulp(a) against the update's magnitude."""
    g = _gen(t0 + 3)
    n, lr, wd = 257, 3e-4, 1e-3
    a, m, v = 1e-3 * torch.randn(n, generator=g), torch.zeros(n), torch.zeros(n)
    if t0:
        m, v = 1e-2 * torch.randn(n, generator=g), 1e-4 * torch.rand(n, generator=g)
    kb2 = abs(_r(1 - 0.999) / (1.0 - _r(0.999)) - 1.0)
    assert 1e-5 < kb2 < 2e-5
    t = O.s32(t0)
    for k in range(5):
        grad = 1e-2 * torch.randn(n, generator=g)
        a64, m64, v64 = O.Adam64(a, m, v, float(t), lr, wd).step(grad)
        a2, m, v, t = O.adam_torch_branch(a, grad, m, v, t, lr, wd)
        upd, upd64 = (a.to(F64) - a2.to(F64)), a.to(F64) - a64
        bc2 = 1.0 - _r(0.999) ** float(t)
        bar = kb2 / 2 + 2.0 ** -24 / bc2 + 8 * O.ULP + float(a.abs().max()) * O.ULP / float(upd64.abs().max())
        err = float((upd - upd64).abs().max() / upd64.abs().max())
        print("t %d: fp32 branch update err %.3g (bar %.3g)" % (int(t), err, bar))
        assert err <= bar
        assert O.ulp_err(m, m64) <= 2.0
        assert float((v.to(F64) - v64).abs().max() / v64.abs().max()) <= kb2 + 2 * O.ULP
        a = a2
    assert float(t) == t0 + 5


# ------------------------------------------------------------------ (a) against DartsSearch's torch branches
@pytest.fixture(scope="module")
def search():
    from katib_amd.models.darts import DartsLayout
    from katib_amd.models.darts_search import DartsSearch

    layout = DartsLayout(PRIMS, init_channels=4, num_layers=2, num_nodes=2, stem_multiplier=1)
    s = DartsSearch(layout, "cpu", seed=3)
    assert s.K is None
    return s


def _stub_loss(s):
    """Replaces the network: a linear loss with fresh random coefficients per call, so every pass
    leaves known, different gradients; records W as each pass sees it."""
    seen = []

    def loss(x, y, P, an, ar, bn):
        g = _gen(100 + len(seen))
        seen.append(s.W.detach().clone())
        total = torch.zeros(())
        for v in list(P.values()) + [an] + ([ar] if isinstance(ar, torch.Tensor) else []):
            if v.requires_grad:
                total = total + (v * torch.randn(v.shape, generator=g)).sum()
        return total, None

    s._loss = loss
    return seen


def _fill(t, src):
    with torch.no_grad():
        t.copy_(src)


def test_oracle_matches_seg_unrolled(search):
    """The torch branch's last addition is add_(W, alpha=wd), an FMA on the CPU: one rounding fewer
    than the kernel's order, scaled by lr - inside 1 ulp of max |w'|, most elements identical."""
    s = search
    g = _gen(21)
    n = s.W.numel()
    w, mom, gr = torch.randn(n, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g)
    _fill(s.W, w), _fill(s.mom, mom), _fill(s.gW, gr)
    _stub_loss(s)
    s._seg_unrolled(None, None)
    want = O.virtual_step(w, mom, gr, s.lr, s.s["w_momentum"], s.s["w_weight_decay"])
    same = int((s.Wv == want).sum())
    print("virtual step: %d of %d elements identical to the torch branch" % (same, n))
    assert O.ulp_err(s.Wv.detach(), want.to(F64)) <= 1.0 and same >= 0.9 * n
    assert torch.equal(s.Av, s.A)


def _pow2_norm_vector(n, g):
    """Dyadic entries whose squares sum to 4 exactly (64 of 1/8, 256 of 1/16, 2 of 1, random signs
    and places): the norm is 2 in any order and precision, and 0.01 / 2 has one rounding however it
    is computed."""
    d = torch.zeros(n)
    pos = torch.randperm(n, generator=g)[:322]
    vals = torch.cat([torch.full((64,), 0.125), torch.full((256,), 0.0625), torch.ones(2)])
    d[pos] = vals * (torch.randint(0, 2, (322,), generator=g) * 2 - 1)
    return d


@pytest.mark.parametrize("exact", [True, False], ids=["pow2-norm", "randn"])
def test_oracle_matches_seg_hessian(search, exact):
    """With a power-of-two norm the branch's eps (0.01 * reciprocal of an fp32 norm) is the
    oracle's, and every later operation is the same single op: bit-exact. With random d the two
    eps differ by their norm and divide roundings (<= 2 ulp), and the rest follows to that."""
    s = search
    g = _gen(22)
    n, na = s.W.numel(), s.A.numel()
    assert n > 322
    w = torch.randn(n, generator=g)
    d = _pow2_norm_vector(n, g) if exact else 0.3 * torch.randn(n, generator=g)
    gav = torch.randn(na, generator=g)
    _fill(s.W, w), _fill(s.gWv, d), _fill(s.gAv, gav)
    seen = _stub_loss(s)
    s._seg_hessian(None, None)
    eps = O.eps_of(d)
    w0 = O.hessian_step(0, w, d, eps)
    w1 = O.hessian_step(1, w0, d, eps)
    w2 = O.hessian_step(2, w1, d, eps)
    gap, ga = s.gAp.detach().clone(), s.gA.detach().clone()
    assert len(seen) == 2 and not torch.equal(gap, ga) and float(gap.abs().max()) > 0
    ag = O.hessian_alpha_grad(gap, ga, gav, eps, s.lr)
    if exact:
        assert float(O.norm32(d)) == 2.0 and float(s.eps) == float(eps)
        assert torch.equal(seen[0], w0) and torch.equal(seen[1], w1) and torch.equal(s.W.detach(), w2)
        assert torch.equal(s.alpha_grad, ag)
    else:
        assert abs(float(s.eps) / float(eps) - 1.0) <= 2 * O.ULP
        for got, want in ((seen[0], w0), (seen[1], w1), (s.W.detach(), w2)):
            assert O.ulp_err(got, want.to(F64)) <= 1.0
        assert O.ulp_err(s.alpha_grad, ag.to(F64)) <= 4.0


def test_adam_branch_copy_is_seg_alpha_step(search):
    s = search
    g = _gen(23)
    na = s.A.numel()
    a, m, v, t = s.A.detach().clone(), torch.zeros(na), torch.zeros(na), O.s32(0.0)
    _fill(s.adam_m, m), _fill(s.adam_v, v), s.adam_t.zero_()
    for k in range(5):
        grad = 1e-2 * torch.randn(na, generator=g)
        _fill(s.alpha_grad, grad)
        s._seg_alpha_step()
        a, m, v, t = O.adam_torch_branch(a, grad, m, v, t, s.s["alpha_lr"], s.s["alpha_weight_decay"])
        assert torch.equal(s.A.detach(), a) and torch.equal(s.adam_m, m) and torch.equal(s.adam_v, v)
        assert float(s.adam_t) == float(t) == k + 1


@pytest.mark.parametrize("scale", [10.0, 0.1], ids=["clipped", "unclipped"])
def test_oracle_matches_seg_weight_update(search, scale):
    """The branch takes an fp32 norm, multiplies the clip by a reciprocal and fuses g + wd w: each
    differs from the kernel's order by at most a rounding - inside 2 ulp of each output's max."""
    s = search
    g = _gen(24)
    n = s.W.numel()
    w, mom, gr = torch.randn(n, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g)
    gr = gr * (scale * s.s["w_grad_clip"] / float(gr.norm()))
    _fill(s.W, w), _fill(s.mom, mom), _fill(s.gW, gr)
    s._seg_weight_update()
    w2, gc, m2 = O.sgd_clip(w, gr, mom, s.lr, s.s["w_grad_clip"], s.s["w_momentum"], s.s["w_weight_decay"])
    for got, want, name in ((s.W.detach(), w2, "w"), (s.gW, gc, "g"), (s.mom, m2, "mom")):
        print("%s: %d of %d identical" % (name, int((got == want).sum()), n))
        assert O.ulp_err(got, want.to(F64)) <= 2.0, name
    if scale == 0.1:
        assert torch.equal(s.gW, gr)  # coef is exactly 1
