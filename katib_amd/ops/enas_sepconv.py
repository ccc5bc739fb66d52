"""Separable convolution of the ENAS child in one HIP kernel per direction (``csrc/hip/enas_sepconv.hip``).

``separable_convolution`` (reference ``op_library.py:22-155``: Keras ``SeparableConv2D``, ``padding='same'``)
is a depthwise convolution followed by a 1x1 convolution with a bias. On the split path those are
``dw_fwd`` and the 1x1 implicit GEMM with the depthwise result ``d`` ``[N, OH, OW, C*dm]`` bf16 between them
in HBM, kept for the backward. :func:`separable_same` keeps ``d`` on the chip: the forward is one launch
(depthwise on the VALU into an LDS tile, pointwise on MFMA, bias on the accumulator), the backward one
launch that recomputes ``d`` with the forward's device function and forms ``gd = gy . wp`` and the
pointwise weight gradient, then the existing ``dw_dgrad`` / ``dw_wgrad`` on ``gd`` and ``channel_sum`` for the
bias. Only ``x`` is saved.

Rounding points: ``d = bf16(fp32 tap sum)``, ``y = bf16(fp32 sum + bias)``, ``gd = bf16(fp32 sum)``; the
pointwise weights are read as bf16, as the implicit GEMM reads them; the pointwise weight gradient is fp32
(atomic adds: not bit-reproducible), everything else is deterministic.

Served: K in {3, 5, 7}, stride in {1, 2}, dm in {1, 2}, ``C % 8 == 0``, ``F % 16 == 0`` and ``F <= 128``,
``N*H*W*max(C*dm, F) < 2^31``, and a map the kernels can cut into bands (at most 128 output columns, one
output row's input patch within the LDS: ``sep_plan``). Anything else stays on the split path.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F_

from . import conv as hconv, dwconv as hdw
from .conv import kernels, same_geometry


def _geom(x, dw_weight, pw_weight, stride):
    N, C, H, W = x.shape
    Cd, _, K, _ = dw_weight.shape
    pt, _, OH = same_geometry(H, K, stride)
    pl, _, OW = same_geometry(W, K, stride)
    return [N, H, W, C, Cd // C, K, int(stride), pt, pl, OH, OW, pw_weight.shape[0]]


def supported(x: torch.Tensor, dw_weight: torch.Tensor, pw_weight: torch.Tensor, stride: int) -> bool:
    if not (x.is_cuda and x.dim() == 4 and dw_weight.dim() == 4 and pw_weight.dim() == 4):
        return False
    N, C, H, W = x.shape
    Cd, one, K, K2 = dw_weight.shape
    Fo = pw_weight.shape[0]
    if not (C > 0 and C % 8 == 0 and Cd in (C, 2 * C) and one == 1 and K == K2 and K in (3, 5, 7)
            and stride in (1, 2) and tuple(pw_weight.shape[1:]) == (Cd, 1, 1) and Fo % 16 == 0 and 16 <= Fo <= 128
            and N * H * W * max(Cd, Fo) < 2 ** 31):
        return False
    return kernels().sep_plan(_geom(x, dw_weight, pw_weight, stride)) is not None


class _SepFn(torch.autograd.Function):
    """The weight images and the gradient sinks are those of ``_DwFn`` (depthwise) and of a 1x1 ``_ConvFn``
    (pointwise, ``[F][Cd]``), through their helpers: built here and returned as gradients without ``prep``
    records, the optimizer's buffers with them - the masters then only anchor the node and their ``.grad``
    stays None."""

    @staticmethod
    def forward(ctx, x, wd, wp, b, stride, prep_dw=None, prep_pw=None):
        k = kernels()
        geom = _geom(x, wd, wp, stride)
        N, H, W, C, dm, K, S, pt, pl, OH, OW, Fo = geom
        Cd = C * dm
        xn = x.to(torch.bfloat16).permute(0, 2, 3, 1).contiguous()
        img, kept_dw = hdw._image(wd, prep_dw)
        wk, kept_pw = hconv._image(wp.reshape(Fo, Cd), Cd, prep_pw)
        ctx.save_for_backward(xn, *kept_dw, *kept_pw)
        y = torch.empty((N, OH, OW, Fo), device=x.device, dtype=torch.bfloat16)
        k.sep_fwd(xn, img, wk, b.detach().float().contiguous() if b is not None else None, y, geom)
        ctx.geom, ctx.prep = geom, (prep_dw, prep_pw)
        ctx.meta = (wd.shape, wd.dtype, wp.shape, wp.dtype, b is not None)
        return y.permute(0, 3, 1, 2)  # NCHW view, channels_last memory

    @staticmethod
    def backward(ctx, gy):
        k = kernels()
        prep_dw, prep_pw = ctx.prep
        N, H, W, C, dm, K, S, pt, pl, OH, OW, Fo = ctx.geom
        Cd, dwgeom = C * dm, ctx.geom[:11]
        wd_shape, wd_dtype, wp_shape, wp_dtype, has_b = ctx.meta
        dev = gy.device
        gyn = gy.to(torch.bfloat16).permute(0, 2, 3, 1).contiguous()
        gx = gwd = gwp = gb = None
        xn, *kept = ctx.saved_tensors
        img = hdw._kept_image(kept[:1], prep_dw)
        wt = hconv._image_t(kept[1:], prep_pw)  # [Cd][F]
        acc, own_pw = hconv._sink(prep_pw, Fo, Cd, dev)
        gd = torch.empty((N, OH, OW, Cd), device=dev, dtype=torch.bfloat16)
        k.sep_bwd_pw(xn, img, wt, gyn, gd, acc, ctx.geom)
        if ctx.needs_input_grad[0]:
            dx = torch.empty((N, H, W, C), device=dev, dtype=torch.bfloat16)
            k.dw_dgrad(gd, img, dx, dwgeom)
            gx = dx.permute(0, 3, 1, 2)
        rows = k.dw_wgrad_rows(dwgeom)
        if prep_dw is not None or ctx.needs_input_grad[1]:  # the optimizer's partials are always fed
            part, own = hdw._sink(prep_dw, rows, Cd, K * K, dev)
            k.dw_wgrad(xn, gd, part, dwgeom)
            if own:
                gwd = part.sum(0).view(wd_shape).to(wd_dtype)
        if own_pw and ctx.needs_input_grad[2]:
            gwp = acc.view(wp_shape).to(wp_dtype)
        if has_b and ctx.needs_input_grad[3]:  # HIP channel sum: no PyTorch reduction under capture
            gb = torch.empty(Fo, device=dev, dtype=torch.float32)
            k.channel_sum(gyn.view(-1, Fo), gb)
        return gx, gwd, gwp, gb, None, None, None


def separable_same(x, dw_weight, pw_weight, pw_bias, stride, prep_dw=None, prep_pw=None):
    """Keras ``SeparableConv2D(padding='same')`` without its activation: bf16 channels-last in and out.
    ``dw_weight`` ``[C*dm, 1, K, K]`` and ``pw_weight`` ``[F, C*dm, 1, 1]`` are the fp32 masters, ``pw_bias``
    ``[F]`` or None; ``prep_dw`` / ``prep_pw``: the records ``ops.enas_optim.ChildAdam`` attached to the two
    layers (both or neither)."""
    if (prep_dw is None) != (prep_pw is None):
        raise ValueError("fused separable conv: both layers' ChildAdam records or neither")
    if not supported(x, dw_weight, pw_weight, stride):
        raise ValueError("fused separable conv: not served (see ops.enas_sepconv.supported): x %s, dw %s, pw %s, "
                         "stride %s" % (tuple(x.shape), tuple(dw_weight.shape), tuple(pw_weight.shape), stride))
    if x.dtype != torch.bfloat16:
        x = x.to(torch.bfloat16)
    return _SepFn.apply(x, dw_weight, pw_weight, pw_bias, int(stride), prep_dw, prep_pw)


class _RoundBf16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t):
        return t.to(torch.bfloat16).to(t.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


def round_bf16(t: torch.Tensor) -> torch.Tensor:
    """The rounding hook of :func:`reference`: the value to bf16 forward, its gradient to bf16 backward."""
    return _RoundBf16.apply(t)


def reference(x, wd, wp, b, stride, dm, rounding=None):
    """The same op in plain torch, in the dtype of its inputs: ``x`` ``[N, C, H, W]``, ``wd`` ``[C*dm, 1, K, K]``,
    ``wp`` ``[F, C*dm, 1, 1]``, ``b`` ``[F]`` or None. ``rounding`` (:func:`round_bf16`) is applied to ``d`` -
    whose gradient is ``gd`` - and to ``y``: the kernels' rounding points."""
    K = wd.shape[-1]
    pt, pb, _ = same_geometry(x.shape[2], K, stride)
    pl, pr, _ = same_geometry(x.shape[3], K, stride)
    assert wd.shape[0] == x.shape[1] * dm
    d = F_.conv2d(F_.pad(x, (pl, pr, pt, pb)), wd, None, stride, 0, 1, x.shape[1])
    if rounding is not None:
        d = rounding(d)
    y = F_.conv2d(d, wp, b)
    return rounding(y) if rounding is not None else y
