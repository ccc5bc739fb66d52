"""Input of an ENAS child layer on the hand-written HIP kernels (``csrc/hip/enas_concat.hip``).

Layer ``l`` of the child network (reference ``examples/v1beta1/trial-images/enas-cnn-cifar10/
ModelConstructor.py:24-81``) reads layer ``l - 1`` and every earlier layer its skip bits select:
smaller feature maps are zero-padded to the largest (``d // 2`` rows above and columns left, the
rest below and right), all are concatenated along the channels, and every op but ``reduction``
starts with a ReLU. :func:`reference` is that composition in PyTorch (a pad per source, a cat, a
ReLU; any device and dtype); :func:`relu_pad_concat` is one kernel per direction for channels-last
bf16 tensors on a GPU. The operation selects, fills zeros and tests a sign, so the two are equal
bit for bit, values and gradients.

``pad8=True`` rounds the channels of the result up to a multiple of 8 with zeros the kernel writes
itself - the input the implicit-GEMM convolutions want (``ops/conv.py``), so a 67-channel layer
input (the 3-channel image as a skip source) is neither padded by a copy afterwards nor built
element by element: one source of fewer than 8 channels among sources of multiples of 8 is served
by the shifted 16-byte kernels. The backward then takes a gradient over the padded channels and
never reads the pad into a source's gradient.
"""

from __future__ import annotations

from typing import List, Sequence

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from .conv import kernels

MAX_SRC = 16  # csrc/hip/enas_concat.h: kMaxSrc


def reference(xs: Sequence[torch.Tensor], relu: bool, pad8: bool = False) -> torch.Tensor:
    m = max(x.shape[2] for x in xs)
    out = []
    for x in xs:
        d = m - x.shape[2]
        if d:
            h = d // 2
            x = F.pad(x, (h, d - h, h, d - h))
        out.append(x)
    y = out[0] if len(out) == 1 else torch.cat(out, 1)
    y = F.relu(y) if relu else y
    return F.pad(y, (0, 0, 0, 0, 0, -y.shape[1] % 8)) if pad8 else y


def supported(xs: Sequence[torch.Tensor], pad8: bool = False) -> bool:
    """What the kernels serve; a caller with another path (``ChildNet``) keeps it for the rest."""
    if not (1 <= len(xs) <= MAX_SRC
            and all(x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 4 and x.shape[2] == x.shape[3]
                    and x.shape[0] == xs[0].shape[0] and x.numel() > 0 for x in xs)):
        return False
    # the kernels' 32-bit indices (the output with pad8, and a gradient either way, may come with its pixels
    # 8-padded, so the bound does not depend on pad8) and exact chunk arithmetic
    m, Ct = max(x.shape[2] for x in xs), sum(x.shape[1] for x in xs)
    return xs[0].shape[0] * m * m * ((Ct + 7) // 8 * 8) < 2 ** 31 and m * (Ct // 8 + 1) ** 2 < 2 ** 32


class _ConcatFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, relu, pad8, fans, *xs):
        fans = list(fans) if fans is not None else [None] * len(xs)
        if len(fans) != len(xs):
            raise ValueError("relu_pad_concat: one fan (or None) per source, got %d for %d" % (len(fans), len(xs)))
        need = ctx.needs_input_grad[3:]
        ctx.relu, ctx.pad8, ctx.fans = relu, pad8, fans
        ctx.geom = [[x.shape[2], x.shape[1]] for x in xs]
        if not xs[0].is_cuda:  # with fans on the CPU: the composition forward, slices of gout backward
            if relu:  # a source with a fan is not kept: the fan holds it
                ctx.save_for_backward(*[x if n and f is None else None for x, n, f in zip(xs, need, fans)])
            out = reference(xs, relu, pad8)
            return out.view_as(out) if out is xs[0] else out
        # [B, C, H, W] -> [B, H, W, C]; a copy only where the channels-last memory is not dense
        xn = [x.permute(0, 2, 3, 1).contiguous() for x in xs]
        B = xn[0].shape[0]
        m = max(x.shape[1] for x in xn)
        Ct = sum(x.shape[3] for x in xn)
        out = torch.empty((B, m, m, Ct + (-Ct % 8 if pad8 else 0)), device=xn[0].device, dtype=torch.bfloat16)
        kernels().enas_concat_fwd(xn, out, relu, pad8)
        if relu:  # the backward reads a source only where it writes a gradient
            ctx.save_for_backward(*[x if n and f is None else None for x, n, f in zip(xn, need, fans)])
        return out.permute(0, 3, 1, 2)  # NCHW view, channels_last memory

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        g = gout.permute(0, 2, 3, 1)
        B, m, _, Cs = g.shape
        gs = g.stride(2)
        # a slice [..., :Ct] of a wider NHWC buffer (the convolutions' input gradient) is read in place
        if g.is_cuda and not (g.dtype == torch.bfloat16 and g.stride(3) == 1 and gs >= Cs and g.stride(1) == m * gs
                              and g.stride(0) == m * m * gs):
            g = g.to(torch.bfloat16).contiguous()
        xs = list(ctx.saved_tensors) if ctx.relu else [None] * len(ctx.geom)
        need = list(ctx.needs_input_grad[3:])
        # a source with a fan hands its contribution over - gout in place, its channel offset, ReLU or not -
        # and gets no gradient from here; one the fan turns down takes its mask from the fan
        off = 0
        for i, ((H, C), fan) in enumerate(zip(ctx.geom, ctx.fans)):
            if need[i] and fan is not None:
                if fan.add(g, off, ctx.relu):
                    need[i] = False
                elif ctx.relu:
                    xs[i] = fan.nhwc() if g.is_cuda else fan.x
            off += C
        if not any(need):
            return (None,) * (3 + len(need))
        if not g.is_cuda:
            gxs, off = [], 0
            for (H, C), x, n in zip(ctx.geom, xs, need):
                t = (m - H) // 2
                gx = g[:, t:t + H, t:t + H, off:off + C].permute(0, 3, 1, 2) if n else None
                gxs.append(torch.where(x <= 0, torch.zeros((), dtype=gx.dtype), gx) if n and ctx.relu else gx)
                off += C
            return (None, None, None) + tuple(gxs)
        gxs: List = [torch.empty((B, H, H, C), device=g.device, dtype=torch.bfloat16) if n else None
                     for (H, C), n in zip(ctx.geom, need)]
        kernels().enas_concat_bwd(ctx.geom, B, xs, gxs, g, ctx.relu, ctx.pad8)
        return (None, None, None) + tuple(None if gx is None else gx.permute(0, 3, 1, 2) for gx in gxs)


def relu_pad_concat(xs: Sequence[torch.Tensor], relu: bool, pad8: bool = False, fans=None) -> torch.Tensor:
    """``relu(cat([zero-pad x to the largest map for x in xs], 1))`` (``relu=False``: no ReLU) for
    ``[B, C, H, W]`` tensors. On a GPU: channels-last bf16 in and out, one HIP kernel forward and one
    backward, whatever the number of sources; on the CPU: :func:`reference`. GPU tensors the kernels
    do not serve (see :func:`supported`) raise from the binding: no quiet change of path here.
    ``pad8``: the result has ``8 ceil(Ct / 8)`` channels, the ones past the channel sum ``Ct`` exactly
    zero, and the backward takes a gradient of that shape whose pad channels reach no source.
    ``fans``: per source its ``ops.enas_fanin.Fan`` (from ``share``) or None. The backward writes no
    gradient for a source with a fan: it records this reader's term in the fan, whose one launch sums
    the layer's gradient over all its readers. A term outside the fan-in's contract (a gradient whose
    pixel stride is no multiple of 8) keeps the path without a fan, and reaches the fan as part of the
    ordinary incoming gradient. ``None``: nothing is deferred."""
    if not xs[0].is_cuda and fans is None:
        return reference(xs, relu, pad8)
    return _ConcatFn.apply(bool(relu), bool(pad8), fans, *xs)
