"""2-D convolution on the hand-written implicit-GEMM HIP kernels (``csrc/hip/conv_igemm.hip``).

Activations are bf16 NHWC (``torch.channels_last``), weights are the fp32 master
parameters ([K, C, R, S]); the forward casts them to a bf16 [K][R][S][C] matrix, the
backward returns an fp32 weight gradient (accumulated by the kernel in fp32) and a bf16
input gradient. Channel counts that are not a multiple of 8 (the 3-channel image stem)
are zero-padded to 8 on the fly; an input that already carries the weight's input channels
rounded up to a multiple of 8 (``enas_concat.relu_pad_concat(..., pad8=True)``) is taken as it is
and gets its gradient over all of its channels.

Used by the ResNet-18 trial (reference BASELINE config 3; the reference's own trial
images delegate convolutions to cuDNN, e.g. ``examples/v1beta1/trial-images/
pytorch-mnist/mnist.py:32-48``) and the ENAS child CNNs (reference
``examples/v1beta1/trial-images/enas-cnn-cifar10/op_library.py:22-155``).

:class:`Conv2d` is a drop-in ``nn.Conv2d``: on a GPU it runs the HIP kernels (inputs
cast to bf16 like autocast does), on CPU it is the stock module.
"""

from __future__ import annotations

import importlib

import torch

from .. import _hipload
import torch.nn as nn
import torch.nn.functional as F

_K = None


def kernels():
    global _K
    if _K is None:
        try:
            _K = _hipload.hipkern()
        except ImportError as e:
            raise ImportError("katib_amd._hipkern is not built (run __graft_entry__.build()): %s" % e)
    return _K


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def _nhwc(t: torch.Tensor) -> torch.Tensor:
    """[N, C, H, W] (any memory format) -> contiguous NHWC view/copy."""
    return t.permute(0, 2, 3, 1).contiguous()


def _pad_c(t: torch.Tensor, c8: int) -> torch.Tensor:
    return t if t.shape[-1] == c8 else F.pad(t, (0, c8 - t.shape[-1]))


def _image(w, C8, prep):
    """The bf16 ``[K][R][S][C8]`` weights ``conv_fwd`` reads, and what the forward saves of them for
    :func:`_image_t`: the image the launch of ``ops.enas_optim.ChildAdam`` writes (``prep``, the record it
    attached to the layer) and nothing, or a cast copy of the master ``w``. The fused separable convolution
    passes its 1x1 weights as ``[F][Cd]``, which is ``[F][1][1][Cd]``."""
    if prep is not None:
        return prep.wk, ()
    wk = _pad_c(w.detach().movedim(1, -1).to(torch.bfloat16), C8).contiguous()
    return wk, (wk,)


def _image_t(kept, prep):
    """The bf16 ``[C8][R][S][K]`` weights ``conv_dgrad`` reads: the optimizer's, or the transpose of the image
    the forward ``kept``."""
    if prep is None:
        return kept[0].transpose(0, -1).contiguous()
    if prep.wt is None:
        raise RuntimeError("prepared conv: the input wants a gradient, the optimizer holds no [C8][R][S][K] "
                           "image for this layer")
    return prep.wt


def _sink(prep, K, n, device):
    """The fp32 ``[K][n]`` accumulator ``conv_wgrad`` adds into, and whether it is the Function's own to return
    as the master's gradient: the one the optimizer reads and zeroes (the master's ``.grad`` stays None), or
    fresh zeros."""
    if prep is not None:
        return prep.g.view(K, -1), False
    return torch.zeros((K, n), device=device, dtype=torch.float32), True


class _ConvFn(torch.autograd.Function):
    """``prep``, the record of ``ops.enas_optim.ChildAdam``, is seen by :func:`_image`, :func:`_image_t` and
    :func:`_sink`, and by the rule that the optimizer's sink is fed whether or not autograd asks: with it
    neither pass copies a weight, fills an accumulator or permutes a gradient, and ``w``, the master parameter,
    only anchors the node in autograd (the backward runs when ``x`` wants no gradient, too)."""

    @staticmethod
    def forward(ctx, x, w, stride, padding, dilation, out_hw, prep=None):
        k = kernels()
        N, C, H, W = x.shape
        K, Cw, R, S = w.shape
        if C != Cw and C != (Cw + 7) // 8 * 8:
            raise ValueError("conv2d: input has %d channels, the weight %d (or that rounded up to 8)" % (C, Cw))
        sh, sw = stride
        ph, pw = padding
        dh, dw = dilation
        if out_hw is None:
            OH = (H + 2 * ph - dh * (R - 1) - 1) // sh + 1
            OW = (W + 2 * pw - dw * (S - 1) - 1) // sw + 1
        else:  # asymmetric ('same') padding: (ph, pw) top/left, the rest implied by the output size
            OH, OW = out_hw
        C8 = (C + 7) // 8 * 8
        xn = _pad_c(_nhwc(x.to(torch.bfloat16)), C8)
        wk, kept = _image(w, C8, prep)
        y = torch.empty((N, OH, OW, K), device=x.device, dtype=torch.bfloat16)
        geom = [N, H, W, C8, K, R, S, OH, OW, sh, sw, ph, pw, dh, dw]
        k.conv_fwd(xn, wk, y, geom)
        ctx.save_for_backward(xn, *kept)
        ctx.geom, ctx.C, ctx.Cw, ctx.wdtype, ctx.prep = geom, C, Cw, w.dtype, prep
        return y.permute(0, 3, 1, 2)  # NCHW view with channels_last memory

    @staticmethod
    def backward(ctx, gy):
        k = kernels()
        xn, *kept = ctx.saved_tensors
        N, H, W, C8, K, R, S, OH, OW = ctx.geom[:9]
        gyn = _nhwc(gy.to(torch.bfloat16))
        gx = gw = None
        if K % 8:
            raise ValueError("HIP conv backward needs K % 8 == 0")
        if ctx.needs_input_grad[0]:
            wt = _image_t(kept, ctx.prep)
            dx = torch.empty((N, H, W, C8), device=gy.device, dtype=torch.bfloat16)
            k.conv_dgrad(gyn, wt, dx, ctx.geom)
            gx = (dx if ctx.C == C8 else dx[..., :ctx.C]).permute(0, 3, 1, 2)
        if ctx.prep is not None or ctx.needs_input_grad[1]:  # the optimizer's accumulator is always fed
            dw32, own = _sink(ctx.prep, K, R * S * C8, gy.device)
            k.conv_wgrad(xn, gyn, dw32, ctx.geom)
            if own:
                gw = dw32.view(K, R, S, C8)[..., :ctx.Cw].permute(0, 3, 1, 2).to(ctx.wdtype)
        return gx, gw, None, None, None, None, None


def channel_sum_nhwc(g: torch.Tensor) -> torch.Tensor:
    """Sum of an [N, C, H, W] gradient over (N, H, W) -> fp32 [C] on the HIP channel-sum kernel
    (C % 8 == 0), never through PyTorch's cross-workgroup reduction: on this ROCm stack that
    reduction (global staging buffer + semaphores) reads its staging memory before writing it
    when replayed from a HIP graph, which turned the captured ENAS child step NaN
    (profiles/enas_child_capture_rootcause_r03.log)."""
    N, C, H, W = g.shape
    rows = g.to(torch.bfloat16).permute(0, 2, 3, 1).contiguous().view(-1, C)
    out = torch.empty(C, device=g.device, dtype=torch.float32)
    kernels().channel_sum(rows, out)
    return out


class _BiasAddFn(torch.autograd.Function):
    """y + bias[c]; the bias gradient is the HIP channel sum (see :func:`channel_sum_nhwc`)."""

    @staticmethod
    def forward(ctx, y, bias):
        ctx.bdtype = bias.dtype
        return y + bias.to(y.dtype).view(1, -1, 1, 1)

    @staticmethod
    def backward(ctx, gy):
        gb = channel_sum_nhwc(gy).to(ctx.bdtype) if ctx.needs_input_grad[1] else None
        return gy, gb


def bias_add(y: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    if y.is_cuda and y.shape[1] % 8 == 0:
        return _BiasAddFn.apply(y, bias)
    return y + bias.to(y.dtype).view(1, -1, 1, 1)


def conv2d(x: torch.Tensor, w: torch.Tensor, bias=None, stride=1, padding=0, dilation=1,
           out_hw=None, prep=None) -> torch.Tensor:
    """bf16 NHWC implicit-GEMM convolution (groups=1) with an fp32 weight master.
    ``out_hw`` overrides the output size for asymmetric padding (``padding`` = top/left). ``prep``: the
    record ``ops.enas_optim.ChildAdam`` attached to the layer (:class:`_ConvFn`)."""
    if x.dtype != torch.bfloat16:
        x = x.to(torch.bfloat16)  # like autocast; keeps the Function's input grad bf16
    y = _ConvFn.apply(x, w, _pair(stride), _pair(padding), _pair(dilation), out_hw, prep)
    if bias is not None:
        y = bias_add(y, bias)
    return y


def weight_supported(w: torch.Tensor, groups: int = 1) -> bool:
    """The part of :func:`supported` the layer alone decides; ``ops.enas_optim.ChildAdam`` sorts by it."""
    return groups == 1 and w.shape[0] % 8 == 0


def supported(x: torch.Tensor, w: torch.Tensor, groups: int = 1) -> bool:
    return x.is_cuda and weight_supported(w, groups) and x.dim() == 4


def _prep_guard(module: nn.Module, x: torch.Tensor) -> None:
    """Called where a layer is about to leave the HIP kernels: with a ``prep`` record that is an error, since
    autograd would fill the master's ``.grad`` while the optimizer reads its own, untouched accumulator."""
    if getattr(module, "prep", None) is not None:
        raise RuntimeError("%s: ChildAdam holds this layer's weight images and gradient buffers, but the HIP kernels "
                           "do not serve this call (input %s on %s); on the fallback the weight would stop training"
                           % (type(module).__name__, tuple(x.shape), x.device))


def same_geometry(size: int, k: int, s: int):
    """TF/Keras ``padding='same'`` along one axis -> (padding before, padding after, output size): bottom /
    right-heavy when the total padding is odd."""
    out = -(-size // s)
    total = max((out - 1) * s + k - size, 0)
    return total // 2, total - total // 2, out


def same_conv2d(x, w, bias, stride: int, prep=None):
    """TF/Keras ``padding='same'``; the kernel takes the top / left padding and the output size."""
    (pt, _, oh), (pl, _, ow) = (same_geometry(size, w.shape[2], stride) for size in x.shape[2:])
    return conv2d(x, w, bias, stride, (pt, pl), 1, (oh, ow), prep)


class Conv2d(nn.Conv2d):
    """``nn.Conv2d`` whose GPU path is the HIP implicit-GEMM kernels (bf16 compute)."""

    def forward(self, x):
        if (supported(x, self.weight, self.groups) and self.padding_mode == "zeros"
                and isinstance(self.padding, tuple)):
            return conv2d(x, self.weight, self.bias, self.stride, self.padding, self.dilation,
                          prep=getattr(self, "prep", None))
        _prep_guard(self, x)
        return super().forward(x)
