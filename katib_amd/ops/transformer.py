"""Transformer ops for the GPT-2 trial: two interchangeable backends.

* :class:`HipOps`   - the hand-written gfx950 kernels of ``csrc/hip/transformer.hip``
  (fused residual-add LayerNorm, tanh GELU, vocabulary cross-entropy with the gradient
  written in place, flat AdamW with global-norm clipping that emits the bf16 shadow
  weights, causal flash attention forward/backward on MFMA). bf16 activations, fp32
  residual stream and statistics.
* :class:`TorchOps` - plain PyTorch implementations of exactly the same contracts
  (any dtype, any device); the numerical oracle for the HIP kernels and the CPU path.

Contracts (``M`` rows, ``D`` features, ``Vp`` padded vocabulary of which ``V`` are real):

``ln_fwd(x32, r, gamma, beta) -> (xin, y, mean, rstd)``
    ``xin = x32 + r`` (fp32; ``x32`` itself when ``r`` is None), ``y = LN(xin)``.
``ln_bwd(dy, xin, mean, rstd, gamma, G, dr, dgamma, dbeta)``
    ``G += LN'(dy)`` in place (``G`` fp32 residual-stream gradient; ``G`` is *set* when
    ``accumulate=False``), ``dr[:] = G`` cast to the activation dtype when ``dr`` is given,
    ``dgamma/dbeta`` written.
``ln_fwd(..., drop=Drop(p, site, seed, step))`` / ``ln_bwd(..., drop=...)`` / ``dropout_(x, drop)``
    dropout of the residual branch ``r`` (forward) and of its gradient ``dr`` (backward), and in place
    over an fp32 tensor; the mask comes from Philox4x32-10 (contract above :func:`philox4x32`), the
    same in both backends bit for bit. ``drop=None`` or ``p == 0``: the calls above, unchanged.
``attn_fwd(qkv, B, T, H) -> (o, lse)``
    causal softmax attention with head dim 64; ``qkv`` is ``[B*T, 3*H*64]`` (q | k | v, heads
    contiguous), ``o`` is ``[B*T, H*64]``, ``lse`` ``[B, H, T]`` = log2-sum-exp2 of the
    scaled scores (in log2 units).
``attn_fwd(..., drop=Drop(...))`` / ``attn_bwd(..., drop=...)``
    dropout of the attention probabilities: ``o = (keep * scale * softmax(s)) @ v`` with the 8-bit
    mask contract above :func:`attn_dropout_mask`; ``lse`` stays that of the undropped softmax.
    ``drop=None`` or a ``p`` below 1/512: the calls above, unchanged.
``xent_fwd(logits, tgt, V) -> (loss_rows, lse)``; ``xent_bwd(logits, tgt, lse, gscale, V)``
    writes ``(softmax - onehot) * gscale / N`` over ``logits`` in place.
"""

from __future__ import annotations

import importlib
import math
import os
from typing import NamedTuple

import torch

from .. import _hipload
import torch.nn.functional as F

LOG2E = 1.4426950408889634


def _kern():
    try:
        return _hipload.hipkern()
    except ImportError as e:
        raise ImportError("katib_amd._hipkern is not built (run __graft_entry__.build()): %s" % e)


# Kernel choices of the GPT-2 step are fixed by measurement, not switched by the environment:
# * one-pass training cross-entropy (xent_fused_k): 783k -> 793k tokens/s against xent_fwd + xent_bwd
#   (profiles/gpt2_xent_fused_ab_r05.log);
# * the fc2 input gradient with the GELU backward in its epilogue (gemm_lt gelu_u): +1.3 % tokens/s
#   against hipBLASLt dgrad + gelu_bwd (profiles/gpt2_gelu_dgrad_ab_r05.log);
# * measured and removed: hipBLASLt's BGRADB weight + bias gradient epilogue (782k -> 743k tokens/s,
#   profiles/lt_epilogue_r05.log) and the fc1 bias gradient from the dgrad epilogue (neutral,
#   profiles/gpt2_gelu_dgrad_bias_ab_r05.log).


# ---------------------------------------------------------------- dropout (Philox4x32-10)
# The dropout mask of the GPT-2 trial is never stored: the kernels of csrc/hip/transformer.hip and
# the torch oracle below recompute it, forward and backward, from the same counter-based generator.
# For a site applied to a row-major [M, D] tensor, element e = row * D + col:
#   q = e >> 2 (64-bit); counter = (q & 0xffffffff, q >> 32, site, step); key = (seed & 0xffffffff, seed >> 32);
#   the element takes output word e & 3 and is kept iff word >= thr = round(p * 2^32);
#   kept values are multiplied by scale = 1 / (1 - p), computed in fp32.
# step = the model's device step counter (completed optimizer steps) as uint32.
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
DROPOUT_MAX_P = 0.9
_M32 = 0xFFFFFFFF


class Drop(NamedTuple):
    """One dropout site: probability, site id, the trial's seed, the device step counter."""
    p: float
    site: int
    seed: int
    step: "torch.Tensor | int"


def check_dropout_p(p: float) -> float:
    p = float(p)
    if not 0.0 <= p <= DROPOUT_MAX_P:  # also rejects NaN
        raise ValueError("dropout must be in [0, %g], got %r" % (DROPOUT_MAX_P, p))
    return p


def dropout_threshold(p: float) -> int:
    return int(math.floor(check_dropout_p(p) * 4294967296.0 + 0.5))


def dropout_scale(p: float) -> float:
    one = torch.ones((), dtype=torch.float32)
    return float(one / (one - torch.tensor(check_dropout_p(p), dtype=torch.float32)))


def _mulhilo32(a: int, b):
    """(hi, lo) words of the 64-bit product of the constant ``a`` and the uint32 values ``b`` (int64
    tensor). A 32 x 32 product overflows int64, so it is assembled from 16-bit limbs."""
    ah, al = a >> 16, a & 0xFFFF
    bh, bl = b >> 16, b & 0xFFFF
    p0 = al * bl
    mid = al * bh + ah * bl + (p0 >> 16)  # < 3 * 2^32
    return ah * bh + (mid >> 16), ((mid & 0xFFFF) << 16) | (p0 & 0xFFFF)


def philox4x32(counter, key):
    """Philox4x32-10 on uint32 words carried in int64 tensors: ``counter`` = 4 and ``key`` = 2 words
    (Python ints or broadcastable tensors); returns the 4 output words as int64 tensors."""
    def word(v):
        v = v.to(torch.int64) if torch.is_tensor(v) else torch.tensor(int(v), dtype=torch.int64)
        return v & _M32

    c0, c1, c2, c3 = (word(v) for v in counter)
    k0, k1 = (word(v) for v in key)
    for _ in range(10):
        hi0, lo0 = _mulhilo32(PHILOX_M0, c0)
        hi1, lo1 = _mulhilo32(PHILOX_M1, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + PHILOX_W0) & _M32, (k1 + PHILOX_W1) & _M32
    return c0, c1, c2, c3


def dropout_mask(M: int, D: int, p: float, site: int, seed: int, step, device=None):
    """Keep mask (bool [M, D]) of one dropout site at one step; ``step`` is an int or the device
    step tensor (read as uint32, no host sync)."""
    if D % 4:
        raise ValueError("dropout_mask: D must be a multiple of 4")
    if torch.is_tensor(step):
        device = step.device if device is None else device
        step = step.reshape(()).to(device=device, dtype=torch.int64)
    q = torch.arange(M * D // 4, dtype=torch.int64, device=device)  # q = e >> 2 for e = row * D + col
    words = philox4x32((q & _M32, q >> 32, int(site), step), (int(seed) & _M32, (int(seed) >> 32) & _M32))
    return (torch.stack(words, -1) >= dropout_threshold(p)).view(M, D)  # word e & 3 = the last axis


def _active(drop) -> bool:
    return drop is not None and check_dropout_p(drop.p) > 0.0


# ---------------------------------------------------------------- attention-probability dropout
# The third dropout site of a GPT-2 block acts on the probabilities P [B*H, T, T] inside the flash
# attention kernels, which never store P. A 32-bit word per probability (the contract above) would
# cost one Philox call per 4 probabilities, several times the softmax's own arithmetic, so this site
# draws 8 bits per element on 4 x 4 tiles - one call serves 16 probabilities:
#   bh = b * H + h, query q, key k, T % 4 == 0;
#   blk = (bh * (T / 4) + (q >> 2)) * (T / 4) + (k >> 2) (64-bit);
#   w = Philox4x32-10(counter = (blk & 0xffffffff, blk >> 32, site, step), key as above);
#   byte = (w[q & 3] >> (8 * (k & 3))) & 0xff; the element is kept iff byte >= thr8 = floor(p * 256 + 0.5);
#   kept values are multiplied by scale = 256 / (256 - thr8), computed in fp32.
# The realised drop probability is thr8 / 256 (a 1/256 grid; the scale is unbiased for that, not for
# the p asked for), and a p below 1/512 rounds to thr8 = 0: the site is inactive and takes the p = 0
# path. The causal mask is applied separately; the draw of a masked position is never used.
def attn_dropout_threshold(p: float) -> int:
    return int(math.floor(check_dropout_p(p) * 256.0 + 0.5))


def attn_dropout_scale(p: float) -> float:
    t = torch.tensor(256.0, dtype=torch.float32)
    return float(t / (t - torch.tensor(float(attn_dropout_threshold(p)), dtype=torch.float32)))


def attn_dropout_mask(B: int, H: int, T: int, p: float, site: int, seed: int, step, device=None):
    """Keep mask (bool [B, H, T, T], causality not applied) of one attention dropout site at one
    step; ``step`` is an int or the device step tensor (read as uint32, no host sync)."""
    if T % 4:
        raise ValueError("attn_dropout_mask: T must be a multiple of 4")
    thr8 = attn_dropout_threshold(p)
    if torch.is_tensor(step):
        device = step.device if device is None else device
        step = step.reshape(()).to(device=device, dtype=torch.int64)
    T4 = T // 4
    blk = torch.arange(B * H * T4 * T4, dtype=torch.int64, device=device)  # (bh, q >> 2, k >> 2) row-major
    words = philox4x32((blk & _M32, blk >> 32, int(site), step), (int(seed) & _M32, (int(seed) >> 32) & _M32))
    w = torch.stack(words, -1).view(B * H, T4, T4, 4, 1)  # [bh, q >> 2, k >> 2, q & 3, .]
    shifts = torch.arange(0, 32, 8, dtype=torch.int64, device=device)  # 8 * (k & 3)
    keep = ((w >> shifts) & 0xFF) >= thr8  # [bh, q >> 2, k >> 2, q & 3, k & 3]
    return keep.permute(0, 1, 3, 2, 4).reshape(B, H, T, T)


def _attn_active(drop) -> bool:
    return drop is not None and attn_dropout_threshold(drop.p) > 0


class TorchOps:
    name = "torch"

    def __init__(self, eps: float = 1e-5):
        self.eps = eps

    # ---------------------------------------------------------------- dropout
    def dropout_mask(self, M, D, drop, device=None):
        return dropout_mask(M, D, drop.p, drop.site, drop.seed, drop.step, device)

    def _dropped(self, t, drop):
        """``keep ? scale * t : 0`` in fp32 for t [M, D]."""
        keep = self.dropout_mask(t.shape[0], t.shape[1], drop, t.device)
        t = t.float()
        return torch.where(keep, t * dropout_scale(drop.p), torch.zeros_like(t))

    def dropout_(self, x, drop):
        """``x = keep ? scale * x : 0`` in place (fp32 [M, D])."""
        if _active(drop):
            x.copy_(self._dropped(x, drop))
        return x

    # ---------------------------------------------------------------- LayerNorm
    def ln_fwd(self, x32, r, gamma, beta, drop=None):
        if _active(drop):
            if r is None:
                raise ValueError("ln_fwd: dropout applies to the residual branch r")
            xin = x32 + self._dropped(r, drop)
        else:
            xin = x32 if r is None else x32 + r.float()
        mean = xin.mean(-1)
        var = ((xin - mean[:, None]) ** 2).mean(-1)
        rstd = torch.rsqrt(var + self.eps)
        y = ((xin - mean[:, None]) * rstd[:, None] * gamma.float() + beta.float()).to(gamma.dtype)
        return xin, y, mean, rstd

    def ln_bwd(self, dy, xin, mean, rstd, gamma, G, dr, dgamma, dbeta, accumulate=True, dbias=None, drop=None):
        """``drop``: the dropout site of the branch whose output gradient ``dr`` is - ``dr`` (and so
        ``dbias``) takes the masked, scaled gradient; ``G`` is unchanged by it."""
        D = xin.shape[-1]
        g = dy.float()
        xh = (xin - mean[:, None]) * rstd[:, None]
        dxh = g * gamma.float()
        dx = rstd[:, None] * (dxh - dxh.sum(-1, keepdim=True) / D - xh * (dxh * xh).sum(-1, keepdim=True) / D)
        if accumulate:
            G.add_(dx)
        else:
            G.copy_(dx)
        if _active(drop):
            if dr is None:
                raise ValueError("ln_bwd: dropout applies to the branch gradient dr")
            dr.copy_(self._dropped(G, drop))
        elif dr is not None:
            dr.copy_(G)
        dgamma.copy_((g * xh).sum(0))
        dbeta.copy_(g.sum(0))
        if dbias is not None and dr is not None:
            dbias.copy_(dr.float().sum(0))

    # ---------------------------------------------------------------- GELU
    def gelu_fwd(self, u):
        return F.gelu(u.float(), approximate="tanh").to(u.dtype)

    def gelu_bwd(self, u, dy):
        x = u.float()
        k0, k1 = math.sqrt(2.0 / math.pi), 0.044715
        t = torch.tanh(k0 * (x + k1 * x ** 3))
        d = 0.5 * (1 + t) + 0.5 * x * (1 - t * t) * k0 * (1 + 3 * k1 * x * x)
        return (dy.float() * d).to(u.dtype)

    # ---------------------------------------------------------------- attention
    def _attn_dropped(self, p, B, T, H, drop):
        """``keep * scale * p`` for the probabilities p [B, H, T, T] (fp32)."""
        keep = attn_dropout_mask(B, H, T, drop.p, drop.site, drop.seed, drop.step, p.device)
        return torch.where(keep, p * attn_dropout_scale(drop.p), torch.zeros_like(p))

    def attn_fwd(self, qkv, B, T, H, hd=64, drop=None):
        q, k, v = qkv.float().view(B, T, 3, H, hd).permute(2, 0, 3, 1, 4)
        s = (q @ k.transpose(-1, -2)) / math.sqrt(hd)
        mask = torch.ones(T, T, dtype=torch.bool, device=qkv.device).triu(1)
        s = s.masked_fill(mask, float("-inf"))
        lse = torch.logsumexp(s, -1)
        p = torch.softmax(s, -1)
        if _attn_active(drop):
            p = self._attn_dropped(p, B, T, H, drop)
        o = p @ v
        return o.permute(0, 2, 1, 3).reshape(B * T, H * hd).to(qkv.dtype), lse * LOG2E

    def attn_bwd(self, qkv, o, dout, lse, B, T, H, hd=64, drop=None):
        with torch.enable_grad():
            x = qkv.detach().float().requires_grad_(True)
            q, k, v = x.view(B, T, 3, H, hd).permute(2, 0, 3, 1, 4)
            s = (q @ k.transpose(-1, -2)) / math.sqrt(hd)
            mask = torch.ones(T, T, dtype=torch.bool, device=qkv.device).triu(1)
            p = torch.softmax(s.masked_fill(mask, float("-inf")), -1)
            if _attn_active(drop):
                p = self._attn_dropped(p, B, T, H, drop)
            out = (p @ v).permute(0, 2, 1, 3).reshape(B * T, H * hd)
            (g,) = torch.autograd.grad(out, x, dout.float())
        return g.to(qkv.dtype)

    # ---------------------------------------------------------------- cross-entropy
    def xent_fwd(self, logits, tgt, V):
        x = logits[:, :V].float()
        lse = torch.logsumexp(x, -1)
        return lse - x.gather(1, tgt[:, None])[:, 0], lse

    def xent_bwd(self, logits, tgt, lse, gscale, V):
        N = logits.shape[0]
        p = torch.exp(logits[:, :V].float() - lse[:, None])
        p[torch.arange(N, device=logits.device), tgt] -= 1.0
        logits[:, :V] = (p * (gscale.float() / N)).to(logits.dtype)
        logits[:, V:] = 0
        return logits

    def xent_train(self, logits, tgt, gscale, V):
        loss, lse = self.xent_fwd(logits, tgt, V)
        return loss, lse, self.xent_bwd(logits, tgt, lse, gscale, V)

    def xent_eval(self, logits, tgt, V):
        """(summed loss, top-1 hits) over the rows: the validation metric (0-d fp32 tensors)."""
        x = logits[:, :V].float()
        return F.cross_entropy(x, tgt, reduction="sum"), (x.argmax(-1) == tgt).sum().float()

    # ---------------------------------------------------------------- GEMM helpers
    def linear(self, x, w, b):
        """x [M, K] . w[N, K]^T (+ b)."""
        return torch.addmm(b, x, w.t()) if b is not None else torch.mm(x, w.t())

    def linear_gelu(self, x, w, b):
        """(u, gelu_tanh(u)) with u = x . w^T + b."""
        u = self.linear(x, w, b)
        return u, self.gelu_fwd(u)

    def colsum(self, x, out):
        torch.sum(x, 0, out=out)

    def wgrad_bgrad(self, dy, x, dw, db):
        """dw = dy^T x; db = column sums of dy (a linear layer's weight + bias gradients)."""
        self.wgrad(dy, x, dw)
        self.colsum(dy, db)

    def dgrad_gelu(self, dy, w, u, db=None):
        """(dy @ w) * gelu_tanh'(u): the MLP's fc2 input gradient taken back through the GELU;
        ``db``: also its column sums (the fc1 bias gradient)."""
        du = self.gelu_bwd(u, self.dgrad(dy, w))
        if db is not None:
            self.colsum(du, db)
        return du

    def dgrad(self, dy, w):
        return torch.mm(dy, w)

    def wgrad(self, dy, x, out):
        torch.mm(dy.t(), x, out=out)

    # ---------------------------------------------------------------- optimizer
    def adamw(self, p, g, m, v, w16, lr, step, b1, b2, eps, wd, max_norm, sumsq):
        gf = g.float()
        sumsq.copy_((gf * gf).sum().reshape(1))
        if max_norm > 0:
            gf = gf * torch.clamp(max_norm / (sumsq.sqrt() + 1e-6), max=1.0)
        t = step.float()
        bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
        m.mul_(b1).add_(gf, alpha=1 - b1)
        v.mul_(b2).addcmul_(gf, gf, value=1 - b2)
        p.mul_(1 - lr * wd)
        p.sub_(lr / bc1 * m / (v.sqrt() / bc2.sqrt() + eps))
        w16.copy_(p)


class HipOps:
    """The gfx950 kernels. Raises at construction if the extension is missing."""

    name = "hip"

    def __init__(self, eps: float = 1e-5, gemm: str = "auto", gemm_bwd: str = "auto"):
        self.k = _kern()
        self.eps = eps
        self._bmm_f32 = True
        # forward projections on the hand-written MFMA GEMM (gemm_bf16.hip, bias / GELU fused into the
        # epilogue) for the shapes where it measured faster than hipBLASLt on MI355X, hipBLASLt
        # (torch.addmm) for the rest (profiles/gemm_bf16_r03.log: at M = 8192 the 128x128-tile kernel
        # wins the d x d projection 1.23-1.37x and loses qkv 0.87x, fc + GELU 0.96x, fc2 0.80x, the LM
        # head 0.61x). gemm="all": every supported shape (tests), "0": hipBLASLt only; gemm_bwd likewise
        # for the backward GEMMs.
        self.gemm = gemm
        self.gemm_bwd = gemm_bwd

    # (N, K) classes where gemm_bf16 beat hipBLASLt in the measured table
    GEMM_WINS = {(768, 768), (256, 256), (512, 512), (1024, 1024)}

    def _gemm_ok(self, x, w):
        if self.gemm in ("0", "off") or x.dtype != torch.bfloat16 or w.dtype != torch.bfloat16 or x.dim() != 2:
            return False
        if self.gemm != "all" and (w.shape[0], w.shape[1]) not in self.GEMM_WINS:
            return False
        return x.is_contiguous() and w.is_contiguous() and bool(self.k.gemm_nt_supported(x.shape[0], w.shape[0],
                                                                                        x.shape[1]))

    def linear(self, x, w, b):
        if not self._gemm_ok(x, w):
            return torch.addmm(b, x, w.t()) if b is not None else torch.mm(x, w.t())
        c = torch.empty((x.shape[0], w.shape[0]), device=x.device, dtype=torch.bfloat16)
        self.k.gemm_nt(x, w, b, c, None)
        return c

    def linear_gelu(self, x, w, b):
        if not self._gemm_ok(x, w):
            u = torch.addmm(b, x, w.t())
            return u, self.gelu_fwd(u)
        u = torch.empty((x.shape[0], w.shape[0]), device=x.device, dtype=torch.bfloat16)
        g = torch.empty_like(u)
        self.k.gemm_nt(x, w, b, u, g)
        return u, g

    # dropout (csrc/hip/transformer.hip): the mask is recomputed by every kernel from Philox4x32-10
    # keyed by (site, seed, device step counter) - see the contract at the top of this module
    def dropout_mask(self, M, D, drop, device=None):
        step = drop.step
        if not torch.is_tensor(step):
            step = torch.full((1,), float(step), device=device, dtype=torch.float32)
        out = torch.empty((M, D), device=step.device, dtype=torch.bool)
        self.k.dropout_mask(out, check_dropout_p(drop.p), drop.site, drop.seed, step)
        return out

    def dropout_(self, x, drop):
        """``x = keep ? scale * x : 0`` in place (fp32 [M, D], D % 4 == 0)."""
        if _active(drop):
            self.k.dropout_f32(x, drop.p, drop.site, drop.seed, drop.step)
        return x

    def ln_fwd(self, x32, r, gamma, beta, drop=None):
        M, D = x32.shape
        xin = x32 if r is None else torch.empty_like(x32)
        y = torch.empty((M, D), device=x32.device, dtype=torch.bfloat16)
        mean = torch.empty(M, device=x32.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        if _active(drop):
            if r is None:
                raise ValueError("ln_fwd: dropout applies to the residual branch r")
            self.k.ln_fwd_drop(x32, r, xin, gamma, beta, y, mean, rstd, self.eps, drop.p, drop.site, drop.seed,
                               drop.step)
            return xin, y, mean, rstd
        self.k.ln_fwd(x32, r, None if r is None else xin, gamma, beta, y, mean, rstd, self.eps)
        return xin, y, mean, rstd

    def ln_bwd(self, dy, xin, mean, rstd, gamma, G, dr, dgamma, dbeta, accumulate=True, dbias=None, drop=None):
        """``dbias``: also the bias gradient of the linear layer whose output gradient ``dr`` is
        (column sums of dr, accumulated by the same kernel instead of a colsum pass). ``drop``: the
        dropout site of that layer's output - ``dr`` and ``dbias`` take the masked, scaled gradient."""
        M, D = xin.shape
        nb = self.k.ln_bwd_blocks(M)
        want = dbias is not None and dr is not None
        part = torch.empty((3 if want else 2, nb, D), device=xin.device, dtype=torch.float32)
        if _active(drop):
            if dr is None:
                raise ValueError("ln_bwd: dropout applies to the branch gradient dr")
            self.k.ln_bwd_drop(dy, xin, mean, rstd, gamma, G if accumulate else None, G, dr, part[0], part[1],
                               part[2] if want else None, drop.p, drop.site, drop.seed, drop.step)
        else:
            self.k.ln_bwd(dy, xin, mean, rstd, gamma, G if accumulate else None, G, dr, part[0], part[1],
                          part[2] if want else None)
        self.k.ln_reduce(part[0], part[1], dgamma, dbeta, part[2] if want else None, dbias if want else None)

    def gelu_fwd(self, u):
        g = torch.empty_like(u)
        self.k.gelu_fwd(u, g)
        return g

    def gelu_bwd(self, u, dy):
        du = torch.empty_like(u)
        self.k.gelu_bwd(u, dy, du)
        return du

    def dgrad_gelu(self, dy, w, u, db=None):
        """(dy @ w) * gelu_tanh'(u) in one launch: the NN dgrad kernel (gemm_lt) with the GELU backward in
        its epilogue (reads u where it writes the gradient) - against hipBLASLt's dgrad + the gelu_bwd
        pass, which writes the gradient, then re-reads it with u and writes it again. ``db`` (the fc1
        bias gradient): one colsum pass over the result."""
        M, N = dy.shape
        K = w.shape[1]
        if (self._bwd_mode() != "0" and self._lt_ok(dy, w, u) and u.shape == (M, K)
                and M % 128 == 0 and K % 128 == 0 and N % 64 == 0):
            out = torch.empty((M, K), device=dy.device, dtype=torch.bfloat16)
            self.k.gemm_lt(dy, False, w, True, None, out, 1, u)
            if db is not None:
                self.colsum(out, db)
            return out
        du = self.gelu_bwd(u, self.dgrad(dy, w))
        if db is not None:
            self.colsum(du, db)
        return du

    def wgrad_bgrad(self, dy, x, dw, db):
        """dw = dy^T x and db = column sums of dy (a linear layer's weight + bias gradients)."""
        self.wgrad(dy, x, dw)
        self.colsum(dy, db)

    def attn_fwd(self, qkv, B, T, H, hd=64, drop=None):
        """``drop``: dropout of the attention probabilities, the mask recomputed inside the flash
        kernels (attn_fwd_k<true>; contract above :func:`attn_dropout_mask`)."""
        assert hd == 64
        o = torch.empty((B * T, H * hd), device=qkv.device, dtype=torch.bfloat16)
        lse = torch.empty((B, H, T), device=qkv.device, dtype=torch.float32)
        if _attn_active(drop):
            self.k.attn_fwd_drop(qkv, o, lse, B, T, H, 1.0 / math.sqrt(hd), drop.p, drop.site, drop.seed,
                                 drop.step)
            return o, lse
        self.k.attn_fwd(qkv, o, lse, B, T, H, 1.0 / math.sqrt(hd))
        return o, lse

    def attn_bwd(self, qkv, o, dout, lse, B, T, H, hd=64, drop=None):
        dqkv = torch.empty_like(qkv)
        delta = torch.empty_like(lse)
        if _attn_active(drop):
            self.k.attn_bwd_drop(qkv, o, dout, lse, delta, dqkv, B, T, H, 1.0 / math.sqrt(hd), drop.p, drop.site,
                                 drop.seed, drop.step)
            return dqkv
        self.k.attn_bwd(qkv, o, dout, lse, delta, dqkv, B, T, H, 1.0 / math.sqrt(hd))
        return dqkv

    def xent_fwd(self, logits, tgt, V):
        N = logits.shape[0]
        loss = torch.empty(N, device=logits.device, dtype=torch.float32)
        lse = torch.empty_like(loss)
        self.k.xent_fwd(logits, tgt, loss, lse, V)
        return loss, lse

    def xent_bwd(self, logits, tgt, lse, gscale, V):
        self.k.xent_bwd(logits, tgt, lse, gscale, 1.0 / logits.shape[0], V)
        return logits

    def xent_train(self, logits, tgt, gscale, V):
        """(loss_rows, lse, dlogits): forward + backward in one read of the logits (the gradient
        overwrites them); falls back to the two-pass kernels for rows wider than 53248."""
        N = logits.shape[0]
        loss = torch.empty(N, device=logits.device, dtype=torch.float32)
        lse = torch.empty_like(loss)
        if not self.k.xent_fused(logits, tgt, loss, lse, gscale, 1.0 / N, V):
            self.k.xent_fwd(logits, tgt, loss, lse, V)
            self.k.xent_bwd(logits, tgt, lse, gscale, 1.0 / N, V)
        return loss, lse, logits

    def xent_eval(self, logits, tgt, V):
        """(summed loss, top-1 hits) in one pass over the bf16 logits (xent_eval_k): no fp32 copy of the
        logits, no softmax / argmax framework kernels on the PBT member's validation path."""
        N = logits.shape[0]
        out = torch.empty((2, -(-N // 4) * 4), device=logits.device, dtype=torch.float32)  # 16-byte aligned rows
        self.k.xent_eval(logits, tgt, out[0, :N], out[1, :N], V)
        s = out[:, :N].sum(1)
        return s[0], s[1]

    def colsum(self, x, out):
        """Bias gradient: bf16 column sums of [M, N] (two-stage, fp32 partials)."""
        self.k.colsum(x, out)

    # Backward GEMMs on the layout-native kernel (gemm_lt: dgrad NN, wgrad TN, no transposed
    # copies; profiles/gemm_fwd_bwd_table_r05.log, MI355X, median of 5 interleaved rounds, 16k
    # tokens = the PBT member's batch). Against the best hipBLASLt form (split-K batched fp32 +
    # row sum for wgrad, the strided mm for dgrad) the 128^2 two-stage tile (~600-800 TF/s) wins
    # only the qkv wgrad (1.07x); hipBLASLt's 192x256 / 256x256 tiles reach ~1 PF/s on the rest.
    # The d x d dgrad wins at 8k tokens (1.19x). gemm_bwd="0": hipBLASLt for all, "all": gemm_lt
    # wherever supported (tests).
    WGRAD_SPLIT = {(2304, 768): 4}  # (out, in) -> split-K
    DGRAD_WINS = {(768, 768)}  # (out, in) classes of W where the NN kernel won (at <= 8k tokens)

    def _bwd_mode(self):
        return self.gemm_bwd

    def _lt_ok(self, *ts):
        return all(t.dtype == torch.bfloat16 and t.dim() == 2 and t.is_contiguous() for t in ts)

    def dgrad(self, dy, w):
        """``dy @ w`` ([M, K] from dy [M, N], w [N, K]): the NN GEMM where it wins, else hipBLASLt."""
        M, N = dy.shape
        K = w.shape[1]
        mode = self._bwd_mode()
        use = mode == "all" or (mode == "auto" and (N, K) in self.DGRAD_WINS and M <= 8192)
        if use and mode != "0" and self._lt_ok(dy, w) and M % 128 == 0 and K % 128 == 0 and N % 64 == 0:
            out = torch.empty((M, K), device=dy.device, dtype=torch.bfloat16)
            self.k.gemm_lt(dy, False, w, True, None, out)
            return out
        return torch.mm(dy, w)

    def wgrad(self, dy, x, out):
        """``out = dy^T x`` ([N, K] from [M, N], [M, K]). The reduction over M = B*T tokens is
        long and the output small (768 x 768 = 36 tiles of 128^2 for the attention
        projection), so it is split S ways: the layout-native TN kernel (gemm_lt) writes one fp32
        slab per K slice and one row-sum launch adds them into the bf16 gradient."""
        M, N = dy.shape
        K = x.shape[1]
        mode = self._bwd_mode()
        S = self.WGRAD_SPLIT.get((N, K)) if mode == "auto" else (8 if mode == "all" else None)
        if S is not None and self._lt_ok(dy, x) and out.is_contiguous() and N % 128 == 0 and K % 128 == 0:
            while S > 1 and M % (64 * S):
                S //= 2
            if M % 64 == 0:
                if S == 1:
                    self.k.gemm_lt(dy, True, x, True, None, out)
                    return
                part = torch.empty((S, N, K), device=dy.device, dtype=torch.float32)
                self.k.gemm_lt(dy, True, x, True, None, part, S)
                self.k.reduce_rows(part.view(S, N * K), out.view(-1))
                return
        tiles = -(-N // 128) * -(-K // 128)
        S = 1
        while tiles * S < 512 and M % (2 * S) == 0 and M // (2 * S) >= 1024:
            S *= 2
        if S == 1 or not self._bmm_f32:
            torch.mm(dy.t(), x, out=out)
            return
        try:
            part = torch.bmm(dy.view(S, M // S, N).transpose(1, 2), x.view(S, M // S, K), out_dtype=torch.float32)
        except (RuntimeError, TypeError, NotImplementedError):
            self._bmm_f32 = False  # this stack's bmm has no fp32-output bf16 path
            torch.mm(dy.t(), x, out=out)
            return
        self.k.reduce_rows(part.view(S, N * K), out.view(-1))

    def adamw(self, p, g, m, v, w16, lr, step, b1, b2, eps, wd, max_norm, sumsq):
        sumsq.zero_()
        self.k.grad_sumsq(g, sumsq)
        self.k.adamw(p, g, m, v, w16, lr, step, b1, b2, eps, wd, sumsq, max_norm)


def get_ops(name: str = "auto", device=None):
    """``hip`` (fails loudly without the extension), ``torch``, or ``auto`` (hip on a GPU)."""
    if name == "auto":
        name = "hip" if (device is not None and torch.device(device).type == "cuda") else "torch"
    if name == "hip":
        return HipOps()
    if name == "torch":
        return TorchOps()
    raise ValueError("unknown transformer ops backend %r" % name)
