"""The DARTS optimizer kernels (csrc/hip/darts_optim.hip: sumsq, virtual step, Hessian phases,
Adam, clipped SGD, alpha softmax, alpha gradient) and the replica folds (csrc/hip/darts_ops.hip:
fold_rows, fold_f64), each called directly and compared with tests/darts_optim_oracle.py:

* bit for bit (torch.equal) against the exact-order fp32 oracle wherever the kernel spells its
  rounding out with _rn intrinsics, and wherever dyadic inputs make every operation exact;
* Adam against fp64 torch.optim.Adam with a bar computed from the project's fp32 torch branch, the
  alpha softmax within (K + 6) 2^-23 of fp64, sumsq within 2 n 2^-53.

Every output and in-place tensor is a slice out of the middle of a sentinel-filled buffer (also
at a 4-byte but not 16-byte aligned start); the bands must stay untouched and read-only tensors
bit-identical. The sizes cross every cap and stride loop of the launches: one element, less than
a wave, workgroup boundaries, two sumsq partials, past grid_for's 1024 workgroups, past the 256
partials and fold_rows' 2048 workgroups."""
import math

import pytest
import torch

import darts_optim_oracle as O

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
SENT, PAD = -1234.5, 64
ELEM_N = [1, 63, 255, 256, 257, 2049, 262144 + 257, 524288 + 4099]
NA = [1, 112, 257, 2 * 14 * 8]
MU, WD, CLIP, LR = 0.9, 3e-4, 5.0, 0.025
NAN = float("nan")


def _dev():
    return torch.device("cuda", 0)


def _k():
    from katib_amd import _hipload

    return _hipload.hipkern()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


class Band:
    """``data`` on the device as a slice ``t`` from the middle of a sentinel-filled buffer; ``off``
    shifts the start off 16-byte alignment (elements)."""

    def __init__(self, data, off=0):
        self.orig = data.detach().clone().reshape(-1)
        self.n, self.lo = self.orig.numel(), PAD + off
        buf = torch.full((self.lo + self.n + PAD,), SENT, dtype=data.dtype)
        buf[self.lo:self.lo + self.n] = self.orig
        self.buf = buf.to(_dev())
        self.t = self.buf[self.lo:self.lo + self.n]
        assert self.n == 0 or self.t.data_ptr() % 16 == (off * data.element_size()) % 16

    def cpu(self):
        return self.t.cpu()

    def put(self, data):
        self.t.copy_(data.reshape(-1))

    def bands_ok(self):
        b = self.buf.cpu()
        return bool((b[:self.lo] == SENT).all()) and bool((b[self.lo + self.n:] == SENT).all())

    def unchanged(self):
        return self.bands_ok() and torch.equal(self.cpu(), self.orig)


def _parts():
    """The 256-slot partials buffer, every slot NaN (stale partials of another vector)."""
    return Band(torch.full((O.MAX_PARTS,), NAN, dtype=F64))


def _sumsq_stale(k, x, parts):
    """sumsq, then every slot past the partial count NaN again: consumers must not read them."""
    P = k.optim_sumsq(x, parts.t)
    parts.t[P:] = NAN
    return P


def _all_bands(*bs):
    return all(b.bands_ok() for b in bs)


def _scalar(v):
    return torch.full((), v, device=_dev())


# ---------------------------------------------------------------------------- sumsq
@pytest.mark.parametrize("n", ELEM_N + [600000])
def test_sumsq_dyadic_is_exact(n):
    k = _k()
    want_parts = max(1, min(math.ceil(n / 2048), 256))
    for off in (0, 1):
        x = Band(O.dyadic(n, _gen(n + off)), off)
        parts = _parts()
        P = k.optim_sumsq(x.t, parts.t)
        assert P == want_parts == O.sumsq_nparts(n)
        p = parts.cpu()
        assert float(p[:P].sum()) == float(O.sumsq_total(x.orig)), (n, off)
        assert bool(torch.isnan(p[P:]).all()) and parts.bands_ok() and x.unchanged()


@pytest.mark.parametrize("n", ELEM_N)
def test_sumsq_randn_within_summation_bound(n):
    k = _k()
    x = Band(torch.randn(n, generator=_gen(n)), 1)
    parts = _parts()
    P = k.optim_sumsq(x.t, parts.t)
    want = float(O.sumsq_total(x.orig))
    got = float(parts.cpu()[:P].sum())
    rel = abs(got - want) / want
    print("sumsq n %d: rel err %.3g, bound %.3g" % (n, rel, 2 * n * 2.0 ** -53))
    assert rel <= 2 * n * 2.0 ** -53
    assert x.unchanged() and parts.bands_ok()


# ---------------------------------------------------------------------------- sgd_clip
def _scaled_grad(n, scale, seed, clip=CLIP):
    """A gradient of norm scale * clip whose fp32 norm no summation order can move."""
    if scale == 0.0:
        return torch.zeros(n)

    def make(g):
        x = torch.randn(n, generator=g)
        return x * (scale * clip / float(x.to(F64).norm()))

    return O.first_stable(make, seed)[0]


# (norm / clip, clip). At clip 5 the clipped norm is 50, where 1e-6 is below half an ulp and the
# "+ 1e-6" of the coefficient cannot show; at clip 0.05 the norm is 0.5 and it moves the sum by 17 ulp.
SGD_CASES = {"clipped": (10.0, CLIP), "unclipped": (0.1, CLIP), "zero": (0.0, CLIP), "clipped-small-norm": (10.0, 0.05)}


@pytest.mark.parametrize("case", list(SGD_CASES))
@pytest.mark.parametrize("n", ELEM_N)
def test_sgd_clip_bit_exact(n, case):
    k = _k()
    scale, clip = SGD_CASES[case]
    g = _gen(7 * n + int(scale * 10))
    w0, m0 = torch.randn(n, generator=g), torch.randn(n, generator=g)
    g0 = _scaled_grad(n, scale, 1000 + n, clip)
    assert O.norm_is_stable(g0)  # the precondition of bit-exactness: a property of the input
    coef = float(O.clip_coef(g0, clip))
    assert (coef < 0.11) if scale == 10.0 else (coef == 1.0)
    if case == "clipped-small-norm":
        assert float(O.norm32(g0) + O.s32(1e-6)) != float(O.norm32(g0))
    w2, gc, m2 = O.sgd_clip(w0, g0, m0, LR, clip, MU, WD)
    lr = _scalar(LR)
    assert float(lr) != LR  # not representable: the kernel must read the device's fp32 value
    for zero_g, off in ((True, 0), (False, 1)):
        w, gr, mom, parts = Band(w0, off), Band(g0, off), Band(m0, 1 - off), _parts()
        P = _sumsq_stale(k, gr.t, parts)
        k.optim_sgd_clip(w.t, gr.t, mom.t, lr, parts.t, P, clip, MU, WD, zero_g)
        assert torch.equal(w.cpu(), w2), (n, case, zero_g, int((w.cpu() != w2).sum()))
        assert torch.equal(mom.cpu(), m2), (n, case, zero_g)
        assert torch.equal(gr.cpu(), torch.zeros(n) if zero_g else gc), (n, case, zero_g)
        assert _all_bands(w, gr, mom, parts) and float(lr) == float(O.s32(LR))
    if scale == 10.0 and n > 1:
        assert not torch.equal(gc, g0) and not torch.equal(w2, O.sgd_clip(w0, g0, m0, LR, 1e9, MU, WD)[0])


# ---------------------------------------------------------------------------- virtual step
@pytest.mark.parametrize("n,na", list(zip(ELEM_N, NA + NA)))
def test_virtual_step_bit_exact(n, na):
    k = _k()
    g = _gen(3 * n)
    w0, m0, g0 = torch.randn(n, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g)
    a0 = 1e-3 * torch.randn(na, generator=g)
    want = O.virtual_step(w0, m0, g0, LR, MU, WD)
    assert not torch.equal(want, O.virtual_step(w0, torch.zeros(n), g0, LR, MU, WD))  # momentum counts
    lr = _scalar(LR)
    junk = lambda m: torch.randn(m, generator=g) + 3.0
    for nz, zero_g, off in ((n // 2, True, 0), (n + 300, False, 1), (n, True, 1)):
        w, mom, gr, wv = Band(w0, off), Band(m0, off), Band(g0, 1 - off), Band(junk(n), off)
        a, av, zw, za = Band(a0, off), Band(junk(na), 1 - off), Band(junk(nz), off), Band(junk(na), off)
        k.optim_virtual_step(wv.t, w.t, mom.t, gr.t, lr, MU, WD, av.t, a.t, zw.t, za.t, zero_g)
        assert torch.equal(wv.cpu(), want), (n, nz, zero_g, int((wv.cpu() != want).sum()))
        assert w.unchanged() and mom.unchanged() and a.unchanged()
        assert (torch.equal(gr.cpu(), torch.zeros(n)) and gr.bands_ok()) if zero_g else gr.unchanged()
        assert torch.equal(av.cpu(), a0) and torch.equal(za.cpu(), torch.zeros(na))
        assert torch.equal(zw.cpu(), torch.zeros(nz))
        assert _all_bands(wv, av, zw, za)


# ---------------------------------------------------------------------------- Hessian phases
def _stable_d(n, seed):
    return O.first_stable(lambda g: 0.3 * torch.randn(n, generator=g), seed)[0]


@pytest.mark.parametrize("n,na", list(zip(ELEM_N, NA + NA)))
def test_hessian_sequential_chain_bit_exact(n, na):
    """Phases 0 -> 1 -> 2 with the alpha accumulator written between phases, as the passes would."""
    k = _k()
    g = _gen(5 * n)
    w0, d0 = torch.randn(n, generator=g), _stable_d(n, 2000 + n)
    assert O.norm_is_stable(d0)
    gav0, A1 = torch.randn(na, generator=g), torch.randn(na, generator=g)
    A2 = A1 + 1e-3 * torch.randn(na, generator=g)
    junk = lambda m: torch.randn(m, generator=g) + 3.0
    eps_w = O.eps_of(d0)
    w_0 = O.hessian_step(0, w0, d0, eps_w)
    w_1 = O.hessian_step(1, w_0, d0, eps_w)
    w_2 = O.hessian_step(2, w_1, d0, eps_w)
    ag_w = O.hessian_alpha_grad(A1, A2, gav0, eps_w, LR)
    for off in (0, 1):
        w, d, parts = Band(w0, off), Band(d0, 1 - off), _parts()
        ga, gap, gav, ag = Band(junk(na), off), Band(junk(na), 1 - off), Band(gav0, off), Band(junk(na), off)
        eps, lr = Band(torch.zeros(1), off), _scalar(LR)
        P = _sumsq_stale(k, d.t, parts)
        args = (w.t, d.t, eps.t.view(()), parts.t, P, ga.t, gap.t, gav.t, ag.t, lr)
        k.optim_hessian(0, *args)
        assert float(eps.cpu()) == float(eps_w), (float(eps.cpu()), float(eps_w))
        assert torch.equal(w.cpu(), w_0) and torch.equal(ga.cpu(), torch.zeros(na))
        assert gap.unchanged() and ag.unchanged()
        ga.put(A1.to(_dev()))
        parts.t.fill_(NAN)  # phases 1 and 2 take eps from the device scalar, never the partials
        k.optim_hessian(1, *args)
        assert torch.equal(w.cpu(), w_1) and torch.equal(gap.cpu(), A1) and torch.equal(ga.cpu(), torch.zeros(na))
        assert ag.unchanged()
        ga.put(A2.to(_dev()))
        k.optim_hessian(2, *args)
        assert torch.equal(w.cpu(), w_2), int((w.cpu() != w_2).sum())
        assert torch.equal(ag.cpu(), ag_w), int((ag.cpu() != ag_w).sum())
        assert torch.equal(ga.cpu(), A2) and torch.equal(gap.cpu(), A1) and float(eps.cpu()) == float(eps_w)
        assert d.unchanged() and gav.unchanged() and _all_bands(w, ga, gap, ag, eps, parts)


@pytest.mark.parametrize("n,nbn,na", [(1, 300, 1), (257, 0, 112), (2049, 1, 257), (63, 262144 + 5, 224),
                                      (262144 + 257, 300, 112), (524288 + 4099, 262144 + 5, 257)])
def test_hessian_split_and_merge_bit_exact(n, nbn, na):
    """Phase 3 (both perturbed vectors, snapshots) and the merging phase 2 that leaves w alone."""
    k = _k()
    g = _gen(11 * n + nbn)
    w0, d0 = torch.randn(n, generator=g), _stable_d(n, 3000 + n)
    assert O.norm_is_stable(d0)
    gav0, A1 = torch.randn(na, generator=g), torch.randn(na, generator=g)
    A2 = A1 + 1e-3 * torch.randn(na, generator=g)
    bn0 = torch.rand(nbn, generator=g) + 0.5
    junk = lambda m: torch.randn(m, generator=g) + 3.0
    eps_w = O.eps_of(d0)
    wp_w, wm_w = O.hessian_split(w0, d0, eps_w)
    momentum = 0.1
    for off in (0, 1):
        w, d, parts = Band(w0, off), Band(d0, 1 - off), _parts()
        ga, gap, gav, ag = Band(junk(na), off), Band(junk(na), 1 - off), Band(gav0, off), Band(junk(na), off)
        wp, wm = Band(junk(n), off), Band(junk(n), 1 - off)
        bn, bnp, bnz = Band(bn0, off), Band(junk(nbn), 1 - off), Band(junk(nbn), off)
        eps, lr = Band(torch.zeros(1), off), _scalar(LR)
        P = _sumsq_stale(k, d.t, parts)
        args = (w.t, d.t, eps.t.view(()), parts.t, P, ga.t, gap.t, gav.t, ag.t, lr, wp.t, wm.t, bn.t, bnp.t, bnz.t,
                momentum)
        k.optim_hessian_split(3, *args)
        assert float(eps.cpu()) == float(eps_w)
        assert torch.equal(wp.cpu(), wp_w) and torch.equal(wm.cpu(), wm_w), (n, off)
        assert torch.equal(ga.cpu(), torch.zeros(na)) and torch.equal(gap.cpu(), torch.zeros(na))
        assert torch.equal(bnp.cpu(), bn0) and torch.equal(bnz.cpu(), bn0)
        assert w.unchanged() and d.unchanged() and bn.unchanged() and ag.unchanged() and gav.unchanged()
        # the passes: alpha accumulators and each branch's running statistics move
        ga.put(A2.to(_dev())), gap.put(A1.to(_dev()))
        bp1, bz1, b1 = (bn0 + 0.1 * torch.randn(nbn, generator=g) for _ in range(3))
        bnp.put(bp1.to(_dev())), bn.put(b1.to(_dev()))
        bnz_now = bnz.cpu()
        parts.t.fill_(NAN)
        k.optim_hessian_split(2, *args)
        assert torch.equal(bn.cpu(), O.bn_merge(b1, bp1, bnz_now, momentum)), (n, nbn, off)
        assert torch.equal(ag.cpu(), O.hessian_alpha_grad(A1, A2, gav0, eps_w, LR))
        assert w.unchanged() and d.unchanged() and torch.equal(bnp.cpu(), bp1) and torch.equal(bnz.cpu(), bnz_now)
        assert torch.equal(wp.cpu(), wp_w) and torch.equal(wm.cpu(), wm_w)
        assert _all_bands(wp, wm, bn, bnp, bnz, ga, gap, ag, eps, parts)
        # cross-form: the concurrent form promises the sequential rounding
        ws = Band(w0, off)
        sargs = (ws.t, d.t, eps.t.view(()), parts.t, P, ga.t, gap.t, gav.t, ag.t, lr)
        _sumsq_stale(k, d.t, parts)
        k.optim_hessian(0, *sargs)
        assert torch.equal(ws.cpu(), wp.cpu())
        k.optim_hessian(1, *sargs)
        assert torch.equal(ws.cpu(), wm.cpu()) and ws.bands_ok()


# ---------------------------------------------------------------------------- Adam
@pytest.mark.parametrize("t0", [0, 1000])
@pytest.mark.parametrize("n", [1, 112, 257, 1000])
def test_adam_against_fp64_adam(n, t0):
    """Five launches; each step's update a_old - a_new against fp64 torch.optim.Adam from the same
    fp32 state, relative to the update's max magnitude. The bar is four times the error of the
    project's fp32 torch branch (DartsSearch._seg_alpha_step's arithmetic on the CPU) against the
    same reference at the same step: powf and the operation order differ from it by a few ulp
    through the cancellation in 1 - b2^t. m carries at most three roundings of half an ulp and v six
    (g twice in its square), so 1.5 ulp of max(|m|, |g|) and 3 ulp of max |v|.
    Measured on an MI355X over all 80 steps: kernel 2.7e-9 .. 4.8e-6, torch branch 2.7e-9 .. 9.5e-6,
    the kernel at most 0.91 of the bar (n = 1, t = 3: 3.1e-6 against 4 x 8.5e-7)."""
    k = _k()
    g = _gen(13 * n + t0)
    lr, wd = 3e-4, 1e-3
    a0, m0, v0 = 1e-3 * torch.randn(n, generator=g), torch.zeros(n), torch.zeros(n)
    if t0:
        m0, v0 = 1e-2 * torch.randn(n, generator=g), 1e-4 * torch.rand(n, generator=g)
    for nzero, off in ((0, 0), (n + 37, 1)):
        a, m, v, grad = Band(a0, off), Band(m0, 1 - off), Band(v0, off), Band(torch.zeros(n), off)
        t, zero = Band(torch.full((1,), float(t0)), off), Band(torch.randn(nzero, generator=g) + 3.0, 1 - off)
        a_c, m_c, v_c = a0, m0, v0
        for step in range(5):
            gr = 1e-2 * torch.randn(n, generator=g)
            grad.put(gr.to(_dev()))
            zero.t.fill_(7.0)
            k.optim_adam(a.t, grad.t, m.t, v.t, t.t.view(()), lr, 0.5, 0.999, wd, 1e-8, zero.t)
            assert float(t.cpu()) == t0 + step + 1  # the counter advances by exactly one
            a64, m64, v64 = O.Adam64(a_c, m_c, v_c, t0 + step, lr, wd).step(gr)
            a_b = O.adam_torch_branch(a_c, gr, m_c, v_c, float(t0 + step), lr, wd)[0]
            upd64 = a_c.to(F64) - a64
            scale = float(upd64.abs().max())
            err_b = float(((a_c.to(F64) - a_b.to(F64)) - upd64).abs().max()) / scale
            err_k = float(((a_c.to(F64) - a.cpu().to(F64)) - upd64).abs().max()) / scale
            print("adam n %d t %d: kernel update err %.3g, fp32 torch branch %.3g, bar %.3g"
                  % (n, t0 + step + 1, err_k, err_b, 4 * err_b))
            assert err_k <= 4 * err_b, (n, t0 + step + 1, err_k, err_b)
            # m = b1 m + (1 - b1) g can cancel: its roundings scale with the larger of |m| and |g|
            g_max = float((gr.to(F64) + float(O.s32(wd)) * a_c.to(F64)).abs().max())
            assert O.ulp_err(m.cpu(), m64, max(g_max, float(m64.abs().max()))) <= 1.5
            assert O.ulp_err(v.cpu(), v64) <= 3.0
            assert torch.equal(zero.cpu(), torch.zeros(nzero)) and torch.equal(grad.cpu(), gr) and grad.bands_ok()
            a_c, m_c, v_c = a.cpu(), m.cpu(), v.cpu()
        assert _all_bands(a, m, v, t, zero)


# ---------------------------------------------------------------------------- alpha softmax
@pytest.mark.parametrize("kind", ["production", "spread", "equal"])
@pytest.mark.parametrize("K", [1, 7, 8, 16])
def test_alpha_softmax_within_bound_of_fp64(K, kind):
    k = _k()
    tol = O.softmax_tol(K)
    worst = 0.0
    for i, rows in enumerate([(1,), (14,), (257,), (600,), (14, 257), (600, 1)]):
        xs = [O.softmax_inputs(r, K, seed=100 * K + 10 * i + j)[kind] for j, r in enumerate(rows)]
        ins = [Band(x, (i + j) % 2) for j, x in enumerate(xs)]
        outs = [Band(torch.full((x.numel(),), 9.0), (i + j + 1) % 2) for j, x in enumerate(xs)]
        k.alpha_softmax([b.t.view(r, K) for b, r in zip(ins, rows)], [b.t.view(r, K) for b, r in zip(outs, rows)])
        for x, bi, bo, r in zip(xs, ins, outs, rows):
            want = O.softmax64(x)
            got = bo.cpu().view(r, K).to(F64)
            rel = float(((got - want).abs() / want).max())
            worst = max(worst, rel)
            assert rel <= tol, (K, kind, rows, rel, tol)
            assert float((got.sum(-1) - 1.0).abs().max()) <= tol
            assert bi.unchanged() and bo.bands_ok()
            if kind == "equal":
                assert torch.equal(bo.cpu(), torch.full((r * K,), 1.0 / K))
    print("alpha_softmax K %d %s: worst rel err %.3g, bound %.3g" % (K, kind, worst, tol))


@pytest.mark.parametrize("nzero", [None, 1, 257, 262144 + 3])
def test_alpha_softmax_zeroes_the_f64_buffer(nzero):
    k = _k()
    K, rows = 8, (14, 14)
    xs = [O.softmax_inputs(r, K, seed=j)["production"] for j, r in enumerate(rows)]
    ins = [Band(x) for x in xs]
    outs = [Band(torch.full((x.numel(),), 9.0)) for x in xs]
    zero = Band(torch.full((nzero,), NAN, dtype=F64), 1) if nzero is not None else None
    k.alpha_softmax([b.t.view(r, K) for b, r in zip(ins, rows)], [b.t.view(r, K) for b, r in zip(outs, rows)],
                    zero.t if zero is not None else None)
    if zero is not None:
        assert torch.equal(zero.cpu(), torch.zeros(nzero, dtype=F64)) and zero.bands_ok()
    for x, bo, r in zip(xs, outs, rows):
        rel = float(((bo.cpu().view(r, K).to(F64) - O.softmax64(x)).abs() / O.softmax64(x)).max())
        assert rel <= O.softmax_tol(K) and bo.bands_ok()


# ---------------------------------------------------------------------------- alpha gradient
class AlphaCase:
    """Dyadic alpha_grad inputs: w multiples of 2^-8 in [0, 1], replicas multiples of 2^-10 below
    2^10 (every fp64 product and sum exact), the gaps between replicas poisoned; destination rows
    adjacent in one sentinel-banded buffer with one more row that no entry names."""

    def __init__(self, k, counts, K, rs, seed, order="interleaved"):
        g = _gen(seed)
        self.rep, self.K, self.nrows = int(k.REP), K, len(counts)
        ne, glen = sum(counts), (int(k.REP) - 1) * rs + K
        w = (torch.randint(0, 257, (ne, K), generator=g).to(F64) / 256.0).to(F32)
        gbuf = torch.full((ne, int(k.REP), rs), 3.0e7, dtype=F64)
        gbuf[:, :, :K] = torch.randint(-(2 ** 20) + 1, 2 ** 20, (ne, int(k.REP), K), generator=g).to(F64) / 1024.0
        gbuf = gbuf.reshape(ne, -1)
        self.dst0 = O.dyadic((self.nrows + 1, K), g, kmax=2 ** 14, denom=1024.0)
        self.dst = Band(self.dst0)
        self.gdev, self.wdev = gbuf.to(_dev()), w.to(_dev())
        rows = [r for r, c in enumerate(counts) for _ in range(c)]
        perm = torch.randperm(ne, generator=g).tolist() if order == "interleaved" else list(range(ne))
        drows = self.dst.t.view(self.nrows + 1, K)
        self.cpu_entries = [(gbuf[e, :glen], rs, w[e], rows[e]) for e in perm]
        self.entries = [(self.gdev[e, :glen], rs, self.wdev[e], drows[rows[e]]) for e in perm]

    def check(self, accumulate):
        want = O.alpha_grad64(self.cpu_entries, self.rep, self.K, self.dst0 if accumulate else None)
        got = self.dst.cpu().view(self.nrows + 1, self.K)
        for r in range(self.nrows):
            assert torch.equal(got[r], want[r]), (r, got[r], want[r])
        assert torch.equal(got[self.nrows], self.dst0[self.nrows]) and self.dst.bands_ok()
        assert float(torch.stack([want[r] for r in range(self.nrows)]).abs().max()) > 0


@pytest.mark.parametrize("K", [1, 7, 8, 16])
def test_alpha_grad_bit_exact(K):
    k = _k()
    assert int(k.REP) >= 2
    for counts in ([1, 15, 16, 17, 33], [128], [16, 1, 17]):
        for rs in (K, K + 5):
            for accumulate in (True, False):
                c = AlphaCase(k, counts, K, rs, seed=K * 100 + rs + len(counts))
                k.alpha_grad(c.entries, accumulate)
                c.check(accumulate)


def test_alpha_grad_through_the_python_chunking():
    """hip_darts._alpha_grad packs rows into launches of at most 64 entries: five rows of 15 cross
    that boundary; a first row of 70 entries goes out as one launch; more than the kernel's 128
    entries on one row is a clear Python error."""
    from katib_amd.ops import hip_darts

    k = _k()
    for counts in ([15] * 5, [70, 15, 15], [70], [128, 3]):
        c = AlphaCase(k, counts, 8, 8, seed=len(counts) + counts[0], order="grouped")
        hip_darts._alpha_grad(c.entries)
        c.check(True)
    c = AlphaCase(k, [129], 8, 8, seed=5, order="grouped")
    with pytest.raises(ValueError, match="129 entries"):
        hip_darts._alpha_grad(c.entries)
    assert c.dst.unchanged()


# ---------------------------------------------------------------------------- folds
@pytest.mark.parametrize("n", ELEM_N)
def test_fold_rows_exact(n):
    k = _k()
    for i, rows in enumerate([1, 2, 16, 17, int(k.REP)]):
        buf0 = O.dyadic((rows, n), _gen(n + rows))
        buf = Band(buf0, i % 2)
        k.fold_rows(buf.t.view(rows, n))
        assert torch.equal(buf.cpu().view(rows, n), O.fold_rows_ref(buf0)), (rows, n)
        assert buf.bands_ok()


@pytest.mark.parametrize("nseg", [1, 3, 128])
def test_fold_f64_exact(nseg):
    """Segments of unequal length (up to 5000 at 128 segments: the per-segment grid of 1024 / nseg
    workgroups strides), replica strides equal to and larger than n with the padding poisoned."""
    k = _k()
    rep, g = int(k.REP), _gen(nseg)
    ns = [1 + (i * 397) % 5000 for i in range(nseg)]
    ns[-1] = 5000
    segs, bands = [], []
    for i, n in enumerate(ns):
        rs = n + (i % 3) * 5
        data = torch.full((rep, rs), SENT, dtype=F64)
        data[:, :n] = O.dyadic((rep, n), g, kmax=2 ** 20, denom=1024.0, dtype=F64)
        b = Band(data.reshape(-1)[:(rep - 1) * rs + n], i % 2)
        bands.append((b, data, n, rs))
        segs.append((b.t, n, rs))
    k.fold_f64(segs)
    for b, data, n, rs in bands:
        want = data.clone()
        want[0, :n] = data[:, :n].sum(0)
        want[1:, :n] = 0.0
        assert torch.equal(b.cpu(), want.reshape(-1)[:(rep - 1) * rs + n]), (n, rs)
        assert b.bands_ok()


# ---------------------------------------------------------------------------- graph replay
def _capture(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph


def test_graph_replay_of_the_weight_update_reads_device_scalars():
    """sumsq + sgd_clip captured once: a replay after lr.fill_() and new gradient contents is the
    oracle for the new values (a linear chain, no parallel branches)."""
    k = _k()
    n = 2049 + 300
    g = _gen(31)
    w, gr, mom, parts, lr = Band(torch.zeros(n)), Band(torch.zeros(n), 1), Band(torch.zeros(n)), _parts(), _scalar(LR)
    graph = _capture(lambda: k.optim_sgd_clip(w.t, gr.t, mom.t, lr, parts.t, k.optim_sumsq(gr.t, parts.t), CLIP, MU, WD,
                                              False))
    for new_lr, scale, seed in ((0.01, 10.0, 41), (0.003, 0.1, 42), (LR, 10.0, 43)):
        w0, m0 = torch.randn(n, generator=g), torch.randn(n, generator=g)
        g0 = _scaled_grad(n, scale, seed)
        assert O.norm_is_stable(g0)
        w.put(w0.to(_dev())), mom.put(m0.to(_dev())), gr.put(g0.to(_dev()))
        lr.fill_(new_lr)
        parts.t[O.sumsq_nparts(n):] = NAN
        graph.replay()
        w2, gc, m2 = O.sgd_clip(w0, g0, m0, new_lr, CLIP, MU, WD)
        assert torch.equal(w.cpu(), w2) and torch.equal(gr.cpu(), gc) and torch.equal(mom.cpu(), m2), new_lr
    assert _all_bands(w, gr, mom, parts)


def test_graph_replay_of_adam_advances_the_device_counter():
    k = _k()
    n = 224
    g = _gen(32)
    a0, grad0 = 1e-3 * torch.randn(n, generator=g), 1e-2 * torch.randn(n, generator=g)

    def state():
        return [Band(a0), Band(torch.zeros(n)), Band(torch.zeros(n)), Band(torch.zeros(1)), Band(grad0),
                Band(torch.ones(n))]

    def launch(s):
        k.optim_adam(s[0].t, s[4].t, s[1].t, s[2].t, s[3].t.view(()), 3e-4, 0.5, 0.999, 1e-3, 1e-8, s[5].t)

    eager = state()
    for _ in range(3):
        launch(eager)
    cap = state()
    graph = _capture(lambda: launch(cap))
    for b, fresh in zip(cap, state()):  # the warm-up and the capture ran on it: back to the start
        b.put(fresh.t)
    for _ in range(3):
        graph.replay()
    assert float(cap[3].cpu()) == 3.0 == float(eager[3].cpu())
    for b, e in zip(cap, eager):
        assert torch.equal(b.cpu(), e.cpu()) and b.bands_ok()
    assert not torch.equal(cap[0].cpu(), a0)
