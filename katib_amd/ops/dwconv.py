"""Depthwise convolution on the hand-written NHWC HIP kernels (``csrc/hip/dwconv.hip``).

The ENAS child networks' ``depthwise_convolution`` op and the depthwise half of
``separable_convolution`` (reference ``examples/v1beta1/trial-images/enas-cnn-cifar10/
op_library.py:22-155``: Keras ``DepthwiseConv2D`` / ``SeparableConv2D`` with
``padding='same'``) - kernel 3/5/7, stride 1/2, depth multiplier 1/2. Activations are bf16
channels-last like the rest of the child network, weights are the fp32 master parameters
(``[C*DM, 1, K, K]``, output channel ``o`` reads input channel ``o // DM`` as in Keras and
``groups=C`` in PyTorch), accumulation is fp32. The weight gradient is summed from
per-workgroup partials without atomics (deterministic). Channel counts that are not a
multiple of 8 (the 3-channel image input of a child whose first op is a (separable)
depthwise convolution) are zero-padded to 8 channels around the kernels, so no child op
falls back to MIOpen's grouped convolution (whose solvers, measured on MI355X, corrupt
the HIP-graph-captured train step: ``profiles/enas_child_capture_bisect_r02.log``).
"""

from __future__ import annotations

import torch

from .conv import kernels, same_geometry


def weight_supported(weight: torch.Tensor, groups: int, stride: int) -> bool:
    """The part of :func:`supported` the layer alone decides; ``ops.enas_optim.ChildAdam`` sorts by it."""
    K = weight.shape[-1]
    dm = weight.shape[0] // max(groups, 1)
    return (weight.shape[0] == groups * dm and dm in (1, 2) and K in (3, 5, 7) and weight.shape[-2] == K
            and stride in (1, 2))


def supported(x: torch.Tensor, weight: torch.Tensor, groups: int, stride: int) -> bool:
    return x.is_cuda and x.dim() == 4 and groups == x.shape[1] and weight_supported(weight, groups, stride)


def _image(w, prep):
    """The fp32 tap-major ``[K*K][Co]`` weights ``dw_fwd`` and ``dw_dgrad`` read, and what the forward saves of
    them for :func:`_kept_image`: the image the launch of ``ops.enas_optim.ChildAdam`` writes (``prep``, the
    record it attached to the layer) and nothing, or a copy of the master ``w``."""
    if prep is not None:
        return prep.img, ()
    img = w.detach().float().reshape(w.shape[0], -1).t().contiguous()
    return img, (img,)


def _kept_image(kept, prep):
    return prep.img if prep is not None else kept[0]


def _sink(prep, rows, Co, KK, device):
    """The fp32 ``[rows][Co][KK]`` per-workgroup partials ``dw_wgrad`` writes, and whether they are the
    Function's own to sum and return as the master's gradient: the optimizer's, which its launch sums (the
    master's ``.grad`` stays None), or a fresh buffer."""
    if prep is not None:
        return prep.partials(rows), False
    return torch.empty((rows, Co, KK), device=device, dtype=torch.float32), True


class _DwFn(torch.autograd.Function):
    """``prep``, the record of ``ops.enas_optim.ChildAdam``, is seen by :func:`_image`, :func:`_kept_image` and
    :func:`_sink`, and by the rule that the optimizer's sink is fed whether or not autograd asks: with it
    there is no weight copy and no ``sum(0)``, and ``w``, the master parameter, only anchors the node in
    autograd."""

    @staticmethod
    def forward(ctx, x, w, b, stride, prep=None):
        k = kernels()
        N, C, H, W = x.shape
        Co, _, K, _ = w.shape
        dm = Co // C
        pt, _, OH = same_geometry(H, K, stride)
        pl, _, OW = same_geometry(W, K, stride)
        geom = [N, H, W, C, dm, K, stride, pt, pl, OH, OW]
        xn = x.to(torch.bfloat16).permute(0, 2, 3, 1).contiguous()
        wt, kept = _image(w, prep)
        y = torch.empty((N, OH, OW, Co), device=x.device, dtype=torch.bfloat16)
        k.dw_fwd(xn, wt, b.detach().float().contiguous() if b is not None else None, y, geom)
        ctx.save_for_backward(xn, *kept)
        ctx.geom, ctx.wshape, ctx.wdtype, ctx.has_b, ctx.prep = geom, w.shape, w.dtype, b is not None, prep
        return y.permute(0, 3, 1, 2)  # NCHW view, channels_last memory

    @staticmethod
    def backward(ctx, gy):
        k = kernels()
        xn, *kept = ctx.saved_tensors
        N, H, W, C, dm, K, S, pt, pl, OH, OW = ctx.geom
        gyn = gy.to(torch.bfloat16).permute(0, 2, 3, 1).contiguous()
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty((N, H, W, C), device=gy.device, dtype=torch.bfloat16)
            k.dw_dgrad(gyn, _kept_image(kept, ctx.prep), dx, ctx.geom)
            gx = dx.permute(0, 3, 1, 2)
        if ctx.prep is not None or ctx.needs_input_grad[1]:  # the optimizer's partials are always fed
            part, own = _sink(ctx.prep, k.dw_wgrad_rows(ctx.geom), C * dm, K * K, gy.device)
            k.dw_wgrad(xn, gyn, part, ctx.geom)
            if own:
                gw = part.sum(0).view(ctx.wshape).to(ctx.wdtype)
        if ctx.has_b and ctx.needs_input_grad[2]:  # HIP channel sum: no PyTorch reduction under capture
            gb = torch.empty(C * dm, device=gy.device, dtype=torch.float32)
            k.channel_sum(gyn.view(-1, C * dm), gb)
        return gx, gw, gb, None, None


def depthwise_same(x: torch.Tensor, weight: torch.Tensor, bias, stride: int, prep=None) -> torch.Tensor:
    """Keras ``padding='same'`` depthwise convolution (bf16 NHWC in / out). ``prep``: the record
    ``ops.enas_optim.ChildAdam`` attached to the layer (``C % 8 == 0``)."""
    if x.dtype != torch.bfloat16:
        x = x.to(torch.bfloat16)
    C = x.shape[1]
    if prep is not None:
        return _DwFn.apply(x, weight, bias, int(stride), prep)
    if C % 8 == 0:
        return _DwFn.apply(x, weight, bias, int(stride))
    # zero channels C..C8-1: output channel o = c*DM + j, so the real outputs are the first C*DM
    c8, dm = (C + 7) // 8 * 8, weight.shape[0] // C
    xp = torch.nn.functional.pad(x, (0, 0, 0, 0, 0, c8 - C))
    wp = torch.nn.functional.pad(weight, (0, 0, 0, 0, 0, 0, 0, (c8 - C) * dm))
    bp = torch.nn.functional.pad(bias, (0, (c8 - C) * dm)) if bias is not None else None
    return _DwFn.apply(xp, wp, bp, int(stride))[:, :C * dm]
