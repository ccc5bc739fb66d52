"""References for the GPT-2 trial kernels (csrc/hip/transformer.hip) in plain
torch, on any device, and the per-row checker the kernel tests judge them with.

Two arms of every contract of ``katib_amd.ops.transformer`` on the same bf16-rounded inputs, each
written from the mathematics (nothing here calls ``TorchOps``):

``TRUTH``  fp64, outputs left in fp64. The only roundings are those that are part of a contract:
           ``dbias`` is the column sum of the bf16 tensor ``dr``, ``w16`` is the bf16 of ``p``, and
           the attention backward takes the bf16 forward output ``o`` as the input it is.
``REF``    the same functions in fp32 with the final rounding of each output's type and the
           intermediate roundings the kernels document: the probabilities P and the score gradient
           dS are bf16 before the second product of the flash kernels, ``dr`` is bf16 before it is
           column-summed into ``dbias``. What a sound fp32 implementation of the contract gives.

``assert_rows_close(got, ref_arm, truth)`` holds a kernel to ``margin`` (4, ARCHITECTURE.md section 7)
times the reference arm's own worst row error against the truth, row by row, each row scaled by its
own maximum. A plain helper module of the tests: tests/test_gpt2_kernel_oracle.py validates it
without a GPU, tests/test_gpu_gpt2_kernels.py compares the kernels with it.
"""
import math

import torch

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
LOG2E = 1.4426950408889634
ULP = {BF16: 2.0 ** -8, F32: 2.0 ** -23}
ROW = 256  # a flat tensor is cut into rows of this many elements
GELU_K0, GELU_K1 = math.sqrt(2.0 / math.pi), 0.044715

# name of a check -> margin above the default. An entry is twice the ratio err(HIP) / max(err(REF), ulp)
# measured on MI355X against TRUTH, with the derivation of the excess beside it (ARCHITECTURE.md
# section 7). Empty: every kernel output is inside the default margin at every tested shape.
MARGINS = {}
DEFAULT_MARGIN = 4


def margin_for(name):
    return MARGINS.get(name, DEFAULT_MARGIN)


def r32(x):
    """A scalar as the bindings pass it: rounded to fp32 (Python float)."""
    if isinstance(x, torch.Tensor):
        return float(x.detach().reshape(()).to(F32))
    return float(torch.tensor(float(x), dtype=F32))


# ------------------------------------------------------------------------------ the checker
def as_rows(x, row=ROW):
    """[R, C] stays; anything else is flattened and cut into rows of ``row`` (zero padded: a zero
    adds neither error nor scale)."""
    if x.dim() == 2:
        return x
    x = x.reshape(-1)
    pad = -x.numel() % row
    if pad:
        x = torch.cat([x, x.new_zeros(pad)])
    return x.view(-1, row)


def row_err(a, truth, ulp, row=ROW):
    """err_i = max_j |a_ij - truth_ij| / max(max_j |truth_ij|, ulp * max |truth|), fp64 [R]."""
    a, t = as_rows(a, row).to(F64), as_rows(truth, row).to(F64)
    assert a.shape == t.shape, (a.shape, t.shape)
    scale = t.abs().amax(1).clamp_min(ulp * float(t.abs().max())).clamp_min(1e-300)
    return (a - t).abs().amax(1) / scale


def rows_report(got, ref_arm, truth, margin=DEFAULT_MARGIN, row=ROW):
    """-> dict(ok, worst row, its errors, the bound, ratio = worst err(got) / max(max err(ref), ulp),
    failing = number of rows over the bound, rows)."""
    ulp = ULP[got.dtype]
    assert torch.isfinite(as_rows(got, row).to(F64)).all(), "non-finite output"
    eg, er = row_err(got, truth, ulp, row), row_err(ref_arm, truth, ulp, row)
    base = max(float(er.max()), ulp)
    i = int(eg.argmax())
    over = eg > margin * base
    return {"ok": not bool(over.any()), "row": i, "err": float(eg[i]), "ref_err": float(er[i]), "base": base,
            "bound": margin * base, "ratio": float(eg[i]) / base, "failing": int(over.sum()), "rows": eg.numel()}


def assert_rows_close(got, ref_arm, truth, margin=DEFAULT_MARGIN, row=ROW, what=""):
    """Every row of ``got`` is within ``margin`` times the reference arm's worst row error (at least
    one ulp of the output type) of the truth; on failure names the worst row and both errors."""
    rep = rows_report(got, ref_arm, truth, margin, row)
    if what:  # the measured ratio, for whoever reads the captured output of a run
        print("%-28s ratio %7.3f  (worst row %d: err %.3e, ref arm %.3e there, %.3e at worst)"
              % (what, rep["ratio"], rep["row"], rep["err"], rep["ref_err"], rep["base"]))
    assert rep["ok"], ("%s: %d of %d rows over the bound %.3e = %g x %.3e; worst row %d: err %.3e, reference arm "
                       "%.3e there" % (what or "rows", rep["failing"], rep["rows"], rep["bound"], margin, rep["base"],
                                       rep["row"], rep["err"], rep["ref_err"]))
    return rep


def rejects(got, ref_arm, truth, margin=DEFAULT_MARGIN, row=ROW):
    """The report when the checker turns ``got`` down, else None."""
    rep = rows_report(got, ref_arm, truth, margin, row)
    return None if rep["ok"] else rep


def head_rows(x, B, T, H, part=None):
    """One token's 64-wide head slice per row: ``o`` [B*T, H*64] or part 0/1/2 (q/k/v) of ``dqkv``."""
    if part is None:
        return x.reshape(B * T * H, 64)
    return x.view(B, T, 3, H, 64)[:, :, part].reshape(B * T * H, 64)


# ------------------------------------------------------------------------------ the two arms
class Arm:
    def __init__(self, dt, rounded):
        self.dt, self.rounded = dt, rounded

    def out(self, x, dtype):
        """The final rounding of an output's type (reference arm only)."""
        return x.to(dtype) if self.rounded else x

    def rb(self, x):
        """An intermediate bf16 rounding a kernel documents (reference arm only)."""
        return x.to(BF16).to(self.dt) if self.rounded else x

    # ---------------------------------------------------------------- LayerNorm
    def ln_fwd(self, x32, r, gamma, beta, eps=1e-5, keep=None, scale=1.0):
        """-> (xin, y, mean, rstd); ``keep`` / ``scale``: the dropout mask of the branch r and its
        fp32 scale 1 / (1 - p)."""
        dt = self.dt
        x = x32.to(dt)
        if r is not None:
            rr = r.to(dt)
            if keep is not None:
                rr = torch.where(keep, rr * r32(scale), torch.zeros_like(rr))
            x = x + rr
        D = x.shape[-1]
        mean = x.sum(-1) / D
        xc = x - mean[:, None]
        rstd = 1.0 / torch.sqrt((xc * xc).sum(-1) / D + r32(eps))
        y = xc * rstd[:, None] * gamma.to(dt) + beta.to(dt)
        return self.out(x, F32), self.out(y, BF16), self.out(mean, F32), self.out(rstd, F32)

    def ln_bwd(self, dy, xin, mean, rstd, gamma, G, accumulate=True, keep=None, scale=1.0, dbias_from_g=False):
        """-> dict(G, dr, dgamma, dbeta, dbias). ``G`` is the fp32 residual-stream gradient before the
        call (ignored when ``accumulate`` is off), ``dr`` the (masked, scaled) new G in bf16, ``dbias``
        the column sums of that bf16 tensor. ``dbias_from_g``: a mutant for the checker's own test."""
        dt = self.dt
        D = xin.shape[-1]
        g, rs = dy.to(dt), rstd.to(dt)[:, None]
        xh = (xin.to(dt) - mean.to(dt)[:, None]) * rs
        dxh = g * gamma.to(dt)
        dx = rs * (dxh - dxh.sum(-1, keepdim=True) / D - xh * ((dxh * xh).sum(-1, keepdim=True) / D))
        Gn = G.to(dt) + dx if accumulate else dx
        Gn = self.out(Gn, F32)
        dr = Gn.to(dt)
        if keep is not None:
            dr = torch.where(keep, dr * r32(scale), torch.zeros_like(dr))
        summed = dr if dbias_from_g else dr.to(BF16).to(dt)  # the contract: dbias = colsum of the bf16 dr
        return {"G": Gn, "dr": self.out(dr, BF16), "dgamma": self.out((g * xh).sum(0), BF16),
                "dbeta": self.out(g.sum(0), BF16), "dbias": self.out(summed.sum(0), BF16)}

    def ln_reduce(self, part):
        """bf16 column sums of fp32 partial rows [nblk, D]."""
        return self.out(part.to(self.dt).sum(0), BF16)

    # ---------------------------------------------------------------- GELU (tanh form)
    def gelu_fwd(self, u):
        x = u.to(self.dt)
        return self.out(0.5 * x * (1.0 + torch.tanh(GELU_K0 * (x + GELU_K1 * x * x * x))), BF16)

    def gelu_bwd(self, u, dy):
        x = u.to(self.dt)
        t = torch.tanh(GELU_K0 * (x + GELU_K1 * x * x * x))
        d = 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * GELU_K0 * (1.0 + 3.0 * GELU_K1 * x * x)
        return self.out(dy.to(self.dt) * d, BF16)

    # ---------------------------------------------------------------- cross-entropy
    def _lse(self, x):
        m = x.amax(-1, keepdim=True)
        return (m + torch.log(torch.exp(x - m).sum(-1, keepdim=True)))[:, 0]

    def xent_fwd(self, logits, tgt, V):
        """-> (loss per row, lse per row) over the first V columns."""
        x = logits[:, :V].to(self.dt)
        lse = self._lse(x)
        return self.out(lse - x.gather(1, tgt[:, None])[:, 0], F32), self.out(lse, F32)

    def xent_bwd(self, logits, tgt, gscale, V, minus_one=True):
        """-> (softmax - onehot) * gscale / N over the real columns, 0 over the pad columns."""
        N, Vp = logits.shape
        x = logits[:, :V].to(self.dt)
        p = torch.exp(x - self._lse(x)[:, None])
        if minus_one:
            p[torch.arange(N, device=logits.device), tgt] -= 1.0
        out = torch.zeros(N, Vp, dtype=self.dt, device=logits.device)
        out[:, :V] = p * (r32(gscale) / N)
        return self.out(out, BF16)

    def xent_eval(self, logits, tgt, V, lowest=True):
        """-> (loss per row, hit per row); a tied maximum is the lowest index's."""
        x = logits[:, :V].to(self.dt)
        idx = torch.arange(V, device=logits.device).expand_as(x)
        at_max = x == x.amax(-1, keepdim=True)
        am = torch.where(at_max, idx, V).amin(-1) if lowest else torch.where(at_max, idx, -1).amax(-1)
        return self.xent_fwd(logits, tgt, V)[0], self.out((am == tgt).to(self.dt), F32)

    # ---------------------------------------------------------------- causal attention, head dim 64
    def _qkv(self, x, B, T, H):
        return x.view(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)  # 3 x [B, H, T, 64]

    def _probs(self, q, k, T, diag):
        s = (q @ k.transpose(-1, -2)) / 8.0
        hidden = torch.ones(T, T, dtype=torch.bool, device=q.device).triu(diag)
        s = s.masked_fill(hidden, float("-inf"))
        m = s.amax(-1, keepdim=True)
        lse = m + torch.log(torch.exp(s - m).sum(-1, keepdim=True))
        return torch.exp(s - lse), lse[..., 0]

    def _dropped(self, p, keep, scale):
        return p if keep is None else torch.where(keep, p * r32(scale), torch.zeros_like(p))

    def attn_fwd(self, qkv, B, T, H, keep=None, scale=1.0, diag=1):
        """-> (o [B*T, H*64], lse [B, H, T] in log2 units, of the undropped softmax). ``keep``
        [B, H, T, T] / ``scale``: attention-probability dropout. ``diag`` = 2 shows key q + 1: a
        mutant for the checker's own test."""
        q, k, v = self._qkv(qkv.to(self.dt), B, T, H)
        p, lse = self._probs(q, k, T, diag)
        o = self.rb(self._dropped(p, keep, scale)) @ v
        return self.out(o.permute(0, 2, 1, 3).reshape(B * T, H * 64), BF16), self.out(lse * LOG2E, F32)

    def attn_bwd(self, qkv, o, dout, B, T, H, keep=None, scale=1.0):
        """-> dqkv [B*T, 3*H*64] from the inputs of the contract: qkv, dout and the bf16 forward output
        ``o``, by the flash backward's algebra - delta = rowsum(dO * o), dS = P (dP - delta),
        dV = P^T dO, dQ = dS K / 8, dK = dS^T Q / 8. ``o`` is an input, so both arms take delta from
        the same given tensor (with the exact output the algebra is the derivative:
        :meth:`attn_bwd_autograd`). REF rounds P and dS to bf16 before the second products."""
        dt = self.dt
        q, k, v = self._qkv(qkv.to(dt), B, T, H)
        do = dout.to(dt).view(B, T, H, 64).permute(0, 2, 1, 3)
        ob = o.to(dt).view(B, T, H, 64).permute(0, 2, 1, 3)
        p, _ = self._probs(q, k, T, 1)
        delta = (do * ob).sum(-1, keepdim=True)
        ds = self.rb(p * (self._dropped(do @ v.transpose(-1, -2), keep, scale) - delta))
        dv = self.rb(self._dropped(p, keep, scale)).transpose(-1, -2) @ do
        dq, dk = (ds @ k) / 8.0, (ds.transpose(-1, -2) @ q) / 8.0
        g = torch.stack([dq, dk, dv]).permute(1, 3, 0, 2, 4).reshape(B * T, 3 * H * 64)
        return self.out(g, BF16)

    def attn_bwd_autograd(self, qkv, dout, B, T, H, keep=None, scale=1.0):
        """The derivative of the forward by autograd in this arm's precision (no ``o``): what
        :meth:`attn_bwd` equals when it is given the exact output."""
        dt = self.dt
        with torch.enable_grad():
            x = qkv.detach().to(dt).requires_grad_(True)
            q, k, v = self._qkv(x, B, T, H)
            p, _ = self._probs(q, k, T, 1)
            out = (self._dropped(p, keep, scale) @ v).permute(0, 2, 1, 3).reshape(B * T, H * 64)
            (g,) = torch.autograd.grad(out, x, dout.to(dt))
        return self.out(g, BF16)

    # ---------------------------------------------------------------- AdamW with the global-norm clip
    def grad_sumsq(self, g):
        gf = g.to(self.dt)
        return (gf * gf).sum()

    def adamw(self, p, g, m, v, lr, step, b1, b2, eps, wd, max_norm, bias_correction=True, clip=True,
              decay_first=True):
        """One step from (p, m, v) with the bf16 gradient g at step count ``step`` (1 = first) ->
        (p', m', v', w16). Hyperparameters are rounded to fp32 first, as the binding rounds them. The
        three flags are mutants for the checker's own test."""
        dt = self.dt
        lr, b1, b2, eps, wd, max_norm, t = (r32(x) for x in (lr, b1, b2, eps, wd, max_norm, step))
        gf = g.to(dt)
        if max_norm > 0 and clip:
            gf = gf * torch.clamp(max_norm / (torch.sqrt(self.grad_sumsq(g)) + r32(1e-6)), max=1.0)
        m = b1 * m.to(dt) + (1.0 - b1) * gf
        v = b2 * v.to(dt) + (1.0 - b2) * gf * gf
        bc1, bc2 = (1.0 - b1 ** t, 1.0 - b2 ** t) if bias_correction else (1.0, 1.0)
        upd = (lr / bc1) * m / (torch.sqrt(v) / math.sqrt(bc2) + eps)
        p = p.to(dt)
        p = p * (1.0 - lr * wd) - upd if decay_first else (p - upd) * (1.0 - lr * wd)
        p, m, v = self.out(p, F32), self.out(m, F32), self.out(v, F32)
        return p, m, v, p.to(BF16)

    # ---------------------------------------------------------------- column sums
    def colsum(self, x):
        """bf16 column sums of [M, N]."""
        return self.out(x.to(self.dt).sum(0), BF16)

    def reduce_rows(self, part):
        """bf16 sum of fp32 partial rows [R, n]."""
        return self.out(part.to(self.dt).sum(0), BF16)


TRUTH = Arm(F64, False)
REF = Arm(F32, True)


class StepUpdate:
    """The update one optimizer step of a flat model makes, d = p32 after - p32 before, against AdamW
    on the gradient that model itself computed: construct it ahead of ``optimizer_step()``, call
    ``check()`` after it. d is cut into rows of 256 and held to the default margin with REF's update
    as the reference arm and TRUTH's as the truth, and must move some weight by more than lr / 2
    (Adam's first steps move a weight with a gradient by about lr): a step that does nothing, or
    skips a stretch of the buffer, fails both, whatever p32 itself is compared with."""

    def __init__(self, model):
        self.model = model
        self.p, self.g, self.m, self.v = (t.clone() for t in (model.p32, model.g16, model.m, model.v))

    def check(self, what):
        """The hyperparameters are the defaults of the model's own ``optimizer_step``."""
        import inspect

        mod = self.model
        hp = {k: prm.default for k, prm in inspect.signature(mod.optimizer_step).parameters.items()}
        lr, step = r32(mod.lr_t), r32(mod.step_t)
        d = mod.p32 - self.p
        assert float(d.abs().max()) > 0.5 * lr, (float(d.abs().max()), lr)
        ref, tru = (arm.adamw(self.p, self.g, self.m, self.v, lr, step, hp["beta1"], hp["beta2"], hp["eps"],
                              hp["weight_decay"], hp["max_norm"])[0] for arm in (REF, TRUTH))
        return assert_rows_close(d, ref - self.p, tru - self.p.to(F64), what=what)


def bf16_near(x):
    """The bf16 value nearest x (Python float)."""
    return float(torch.tensor(float(x), dtype=F32).to(BF16))
