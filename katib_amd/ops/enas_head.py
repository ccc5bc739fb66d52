"""Head of an ENAS child on the hand-written HIP kernels (``csrc/hip/enas_head.hip``): global average
pooling, ``Dropout``, the dense classifier and softmax cross-entropy with the accuracy bookkeeping
(reference ``examples/v1beta1/trial-images/enas-cnn-cifar10/ModelConstructor.py``), two launches
forward and one backward.

Contract. ``x`` is the last layer's activation ``[B, C, H, W]`` (on a GPU: the NCHW view of dense
channels-last bf16 memory), ``weight`` ``[K, C]`` and ``bias`` ``[K]`` the ``nn.Linear`` masters,
``y`` int64 labels in ``[0, K)``::

    pooled = x.sum((2, 3)) * (1 / HW)
    feat   = where(keep, pooled * scale, 0)      keep = dropout_mask(B, Cp, p, site, seed, step)[:, :C],
                                                 Cp = 4 ceil(C / 4), scale = 1 / (1 - p) in fp32;
                                                 p = 0 or evaluation: feat = pooled
    logits = feat @ weight.T + bias
    loss_b = logsumexp(logits) - logits[y];  hit_b = (lowest argmax == y);  loss = sum(loss_b) / B

``drop`` is a ``Drop(p, site, seed, step)`` of ``ops/transformer.py`` whose ``step`` is a device int32
tensor: the kernels read it, and a training forward adds 1 to it after the draw, so a replayed graph
draws a fresh mask each step. :func:`reference` is the contract as a torch composition in the dtype
of its inputs - the oracle of the tests, and what the entry points run on a CPU.
"""

from __future__ import annotations

from typing import NamedTuple, Optional

import torch
from torch.autograd.function import once_differentiable

from .conv import kernels
from .transformer import Drop, check_dropout_p, dropout_mask, dropout_scale, dropout_threshold

MAX_K = 64    # csrc/hip/enas_head.h: kMaxK
MAX_C = 4096  # csrc/hip/enas_head.h: kMaxC

NO_DROP = Drop(0.0, 0, 0, 0)


class Parts(NamedTuple):
    """What a forward leaves: ``loss`` (mean; the sum in evaluation), ``hits``, and per sample
    ``feat [B, C]``, ``keep [B, C]``, ``logits [B, K]``, ``dl [B, K]`` (None from :func:`reference`:
    autograd has it), ``loss_b [B]``, ``hit_b [B]``."""
    loss: torch.Tensor
    hits: torch.Tensor
    feat: torch.Tensor
    keep: torch.Tensor
    logits: torch.Tensor
    dl: Optional[torch.Tensor]
    loss_b: torch.Tensor
    hit_b: torch.Tensor


def limit(B: int, H: int, W: int, C: int, K: int) -> str:
    """The limit of the kernels that these sizes break, or ''."""
    if K > MAX_K:
        return "K = %d classes, the head kernels serve K <= %d" % (K, MAX_K)
    if C > MAX_C:
        return "C = %d channels, the head kernels serve C <= %d" % (C, MAX_C)
    if B * H * W * C >= 2 ** 31:
        return "B * H * W * C = %d, the head kernels index with 32 bits (< 2^31)" % (B * H * W * C)
    return ""


def supported(x: torch.Tensor, K: int) -> bool:
    return (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 4 and x.numel() > 0 and 1 <= K
            and x.permute(0, 2, 3, 1).is_contiguous() and not limit(*x.shape[:1], *x.shape[2:], x.shape[1], K))


def reference(x, weight, bias, y, drop: Drop = NO_DROP, train: bool = True) -> Parts:
    B, C, H, W = x.shape
    pooled = x.sum((2, 3)) * (1.0 / (H * W))
    p = check_dropout_p(drop.p) if train else 0.0
    if p > 0.0:
        keep = dropout_mask(B, (C + 3) // 4 * 4, p, drop.site, drop.seed, drop.step, x.device)[:, :C]
        feat = torch.where(keep, pooled * dropout_scale(p), torch.zeros_like(pooled))
    else:
        keep, feat = torch.ones(B, C, dtype=torch.bool, device=x.device), pooled
    logits = torch.nn.functional.linear(feat, weight.to(feat.dtype), bias.to(feat.dtype))
    loss_b = torch.logsumexp(logits, 1) - logits.gather(1, y[:, None])[:, 0]
    hit_b = (logits.argmax(1) == y).to(loss_b.dtype)
    loss = loss_b.sum() / B if train else loss_b.sum()
    return Parts(loss, hit_b.sum(), feat, keep, logits, None, loss_b, hit_b)


def _book(stats, drop, loss, hits, train):
    # the bookkeeping of the finishing kernel, for the CPU path
    if stats is not None:
        stats[0].add_(loss.detach().to(stats.dtype))
        stats[1].add_(hits.to(stats.dtype))
    if train and torch.is_tensor(drop.step):
        drop.step.add_(1)


def forward_parts(x, weight, bias, y, drop: Drop = NO_DROP, stats=None, train: bool = True) -> Parts:
    """The two forward launches on a GPU tensor; sizes the kernels do not serve raise from the binding."""
    xn = x.permute(0, 2, 3, 1).contiguous()  # [B, H, W, C]; a copy only where the channels-last memory is not dense
    p = check_dropout_p(drop.p) if train else 0.0
    step = drop.step if torch.is_tensor(drop.step) else None
    if p > 0.0 and step is None:
        raise ValueError("enas_head: dropout needs Drop.step as a device int32 tensor")
    seed = int(drop.seed)
    out, feat, keep, logits, dl, loss_b, hit_b = kernels().enas_head_fwd(
        xn, weight, bias, y, dropout_threshold(p), dropout_scale(p), int(drop.site), seed & 0xFFFFFFFF,
        (seed >> 32) & 0xFFFFFFFF, step if train else None, bool(train), stats)
    return Parts(out[0], out[1], feat, keep, logits, dl, loss_b, hit_b)


def backward_parts(parts: Parts, weight, g, H: int, W: int, p: float, need=(True, True, True), segs: int = 0):
    """(dx ``[B, C, H, W]`` view of NHWC bf16, dW, db) in one launch; None where ``need`` says so."""
    dx, dw, db = kernels().enas_head_bwd(g, parts.dl, weight, parts.feat, parts.keep, H, W, dropout_scale(p),
                                         bool(need[0]), bool(need[1]), bool(need[2]), int(segs))
    return (None if dx is None else dx.permute(0, 3, 1, 2)), dw, db


class _HeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, y, drop, stats):
        parts = forward_parts(x, weight, bias, y, drop, stats, True)
        ctx.save_for_backward(weight, parts.feat, parts.keep, parts.dl)
        ctx.hw, ctx.p = (x.shape[2], x.shape[3]), float(drop.p)
        return parts.loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        weight, feat, keep, dl = ctx.saved_tensors
        parts = Parts(None, None, feat, keep, None, dl, None, None)
        g = g.to(torch.float32).contiguous()
        dx, dw, db = backward_parts(parts, weight, g, ctx.hw[0], ctx.hw[1], ctx.p, ctx.needs_input_grad[:3])
        return dx, dw, db, None, None, None


def head_loss(x, weight, bias, y, drop: Drop = NO_DROP, stats=None) -> torch.Tensor:
    """Mean training loss of the head, differentiable in ``x``, ``weight`` and ``bias``. ``stats`` (2
    fp32: loss sum, correct) gets the loss and the hit count added; ``drop.step`` advances by 1."""
    if not x.is_cuda:
        r = reference(x, weight, bias, y, drop, True)
        _book(stats, drop, r.loss, r.hits, True)
        return r.loss
    return _HeadFn.apply(x, weight, bias, y, drop, stats)


@torch.no_grad()
def head_eval(x, weight, bias, y):
    """(loss sum, correct) of an evaluation batch: no dropout, the step counter untouched."""
    r = (forward_parts if x.is_cuda else reference)(x, weight, bias, y, NO_DROP, train=False)
    return r.loss, r.hits
