"""Device-side random crop + horizontal flip (+ normalisation) fused into the batch gather.

The reference's DARTS trial trains on ``RandomCrop(32, padding=4)`` + ``RandomHorizontalFlip`` +
per-channel normalisation; here the data set lives in HBM and a batch is an on-device gather, so
the augmentation is part of that gather: one kernel (``csrc/hip/augment.hip``) reads the sample,
crops, flips, normalises and writes the batch once.

The contract. One draw per (sample, stream, epoch), a pure function of the sample's DATA-SET index
(not of the batch size, the batch position or the world size)::

    i    = idx[b]                                   (int64 data-set index)
    w    = Philox4x32-10(counter = (i lo, i hi, stream, epoch), key = (seed lo, seed hi))
    k    = 2 * pad + 1
    dx   = (w[0] * k) >> 32                         (0 .. 2 pad)
    dy   = (w[1] * k) >> 32
    flip = flip_enabled and (w[2] >> 31)
    sy   = y + dy - pad
    sx   = (flip ? W - 1 - x : x) + dx - pad        (crop first, then flip the crop)
    out[b, c, y, x] = value(i, c, sy, sx) if 0 <= sy < H and 0 <= sx < W else fill[c]

Sources: ``u8`` packed ``[N, H, W, 4]`` uint8 (channels in bytes 0..C-1) with a table ``lut [C, 256]``
fp32, ``value = lut[c][byte]`` and ``fill[c] = lut[c][0]`` (the reference pads the raw image with 0
before it normalises); ``f32`` ``[N, C, H, W]`` and ``bf16`` ``[N, H, W, C]``, ``value`` a copy and
``fill`` 0. Destinations: ``[B, C, H, W]`` fp32, or ``[B, H, W, C8]`` bf16 with channels C..C8-1
zero (the fused ResNet step's ``x0``). An index outside ``[0, N)`` yields the fill image.
``pad = 0, flip = False`` is a plain (normalising) gather. A third destination, ``nhwc``, is the
unpadded channels-last ``[B, H, W, C]`` bf16 batch (exactly ``C`` channels): ``out.permute(0, 3, 1, 2)``
is the channels-last NCHW tensor the ENAS child feeds its first layer.

Translation mode (``AugSpec.translate > 0``, which needs ``pad == 0``): the ENAS reference child's
``RandomFlip('horizontal')`` + ``RandomTranslation(translate, translate)``. The same Philox call, so
the keying by data-set index (independence of batch size, batch position and world size, the device
epoch, graph replay) is that of crop mode::

    rx   = floor(translate * W * 256),  ry = floor(translate * H * 256)     (host-side ints)
    tx   = ((w[0] * (2 rx + 1)) >> 32) - rx          (translation in 1/256 pixel, -rx .. rx)
    ty   = ((w[1] * (2 ry + 1)) >> 32) - ry
    flip = flip_enabled and (w[2] >> 31)             (flip first, then translate: the reference's layer order)

    u = 256 x - tx,  x0 = u >> 8 (arithmetic),  fx = u & 255        (likewise v, y0, fy from y, ty)
    R_n(k)  = k < 0 ? -1 - k : (k >= n ? 2 n - 1 - k : k)           (Keras 'reflect': d c b a | a b c d | d c b a)
    col(k)  = flip ? W - 1 - R_W(k) : R_W(k)
    a = value(i, c, R_H(y0),     col(x0)),   b = value(i, c, R_H(y0),     col(x0 + 1))
    e = value(i, c, R_H(y0 + 1), col(x0)),   d = value(i, c, R_H(y0 + 1), col(x0 + 1))
    out[b, y, x, c] = ((f((256-fy)(256-fx)) * a + f((256-fy) fx) * b)
                     + (f(fy (256-fx)) * e      + f(fy fx) * d)) * 2^-16

``f()`` is the exact int -> fp32 conversion (the weights are at most 65536), and every ``*`` and
``+`` of the last line is one IEEE fp32 operation, rounded on its own, in the order written - no
step is fused into an FMA, in the kernel or here - which is what lets kernel and oracle agree bit
for bit. ``translate <= 0.5`` keeps every tap within one reflection (``-n/2 - 1 <= k <= n + n/2``).
A whole-pixel draw (``fx = fy = 0``) returns ``a`` exactly; an index outside ``[0, N)`` yields the
fill image. bf16 destinations round the interpolated fp32 value last, to nearest-even.

This is Keras' transformation in kind, not bit parity with TensorFlow: here the flip comes first,
the translation is uniform in +-factor * size, sampling is bilinear and the fill is reflect, but
TensorFlow reflects the continuous coordinate before it interpolates whereas here the integer taps
are reflected.

``augment_reference`` is the contract in integer torch arithmetic (the Philox is
``ops/transformer.py: philox4x32``, shared with the dropout kernels): the oracle of the tests and
the implementation on the CPU. ``augment_gather`` runs the HIP kernel on a GPU.
"""

from __future__ import annotations

import dataclasses
import math
from typing import Optional, Tuple, Union

import torch

from .transformer import philox4x32

_M32 = 0xFFFFFFFF
MAX_PAD = 16

# (source dtype, destination) pairs the kernel is instantiated for; the two "nhwc" forms are built
# in plain / crop mode and in translation mode, the other four in plain / crop mode only
_HIP_FORMS = {(torch.uint8, "nchw"), (torch.float32, "nchw"), (torch.uint8, "c8"), (torch.bfloat16, "c8"),
              (torch.uint8, "nhwc"), (torch.bfloat16, "nhwc")}
# the binding's destination argument: from out's dtype (fp32 NCHW / bf16 C8) | augment.h: kDstNHWC
DST_AUTO, DST_NHWC = -1, 2


@dataclasses.dataclass(frozen=True)
class AugSpec:
    """``seed`` is 64-bit, ``stream`` a 32-bit id separating passes that visit the same image in
    one epoch, ``epoch`` an int or a one-element int32 device tensor (the kernel reads it from
    device memory, so a captured graph replays with a new epoch after ``epoch_t.fill_(e)``).
    ``translate > 0`` selects translation mode (a fraction of the image size, at most 0.5, with
    ``pad == 0``)."""
    pad: int = 4
    flip: bool = True
    seed: int = 0
    stream: int = 0
    epoch: Union[int, torch.Tensor] = 0
    translate: float = 0.0

    def __post_init__(self):
        if not 0 <= int(self.pad) <= MAX_PAD:
            raise ValueError("AugSpec: pad must be in [0, %d], got %r" % (MAX_PAD, self.pad))
        if not 0.0 <= float(self.translate) <= 0.5:
            raise ValueError("AugSpec: translate must be in [0, 0.5], got %r" % (self.translate,))
        if self.translate > 0 and int(self.pad) != 0:
            raise ValueError("AugSpec: translate needs pad == 0, got pad = %r" % (self.pad,))
        if torch.is_tensor(self.epoch) and (self.epoch.numel() != 1 or self.epoch.dtype != torch.int32):
            raise ValueError("AugSpec: a tensor epoch must be a one-element int32 tensor")

    def replace(self, **kw) -> "AugSpec":
        return dataclasses.replace(self, **kw)


PLAIN = AugSpec(pad=0, flip=False)  # the plain (normalising) gather


def cifar_lut(mean, std) -> torch.Tensor:
    """``lut[c][v] = (v / 255 - mean[c]) / std[c]`` in fp32, built on the host once: the kernel and
    the oracle then read the same bits whatever a compiler does to the expression."""
    v = torch.arange(256, dtype=torch.float32) / 255.0
    mean = torch.as_tensor(mean, dtype=torch.float32).view(-1, 1)
    std = torch.as_tensor(std, dtype=torch.float32).view(-1, 1)
    return ((v.view(1, 256) - mean) / std).contiguous()


def _philox(idx: torch.Tensor, spec: AugSpec):
    i = idx.to(torch.int64)
    epoch = spec.epoch
    if torch.is_tensor(epoch):
        epoch = epoch.reshape(()).to(device=i.device, dtype=torch.int64)
    seed = int(spec.seed)
    return philox4x32((i & _M32, i >> 32, int(spec.stream), epoch), (seed & _M32, (seed >> 32) & _M32))


def draws(idx: torch.Tensor, spec: AugSpec) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dx, dy, flip) int64 tensors of the samples with data-set indices ``idx``."""
    w = _philox(idx, spec)
    k = 2 * int(spec.pad) + 1
    dx, dy = (w[0] * k) >> 32, (w[1] * k) >> 32
    flip = (w[2] >> 31) if spec.flip else torch.zeros_like(dx)
    return dx, dy, flip


def translate_range(spec: AugSpec, H: int, W: int) -> Tuple[int, int]:
    """(rx, ry): the largest translation in 1/256 pixel, ``floor(translate * size * 256)``."""
    t = float(spec.translate)
    return int(math.floor(t * W * 256)), int(math.floor(t * H * 256))


def draws_translate(idx: torch.Tensor, spec: AugSpec, H: int = 32,
                    W: int = 32) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(tx, ty, flip) int64 tensors of translation mode: ``tx`` in ``-rx .. rx`` and ``ty`` in
    ``-ry .. ry``, in 1/256 pixel of an ``H x W`` image (CIFAR's 32 x 32 unless given)."""
    w = _philox(idx, spec)
    rx, ry = translate_range(spec, H, W)
    tx, ty = ((w[0] * (2 * rx + 1)) >> 32) - rx, ((w[1] * (2 * ry + 1)) >> 32) - ry
    flip = (w[2] >> 31) if spec.flip else torch.zeros_like(tx)
    return tx, ty, flip


def _source_geometry(src: torch.Tensor, lut: Optional[torch.Tensor]):
    if src.dim() != 4:
        raise ValueError("augment: the source must be 4-D, got %s" % (tuple(src.shape),))
    if src.dtype == torch.uint8:
        if lut is None or lut.dim() != 2 or lut.shape[1] != 256 or not 1 <= lut.shape[0] <= 4:
            raise ValueError("augment: a u8 source needs lut [C <= 4, 256]")
        if src.shape[3] != 4:
            raise ValueError("augment: a u8 source is packed [N, H, W, 4]")
        return src.shape[0], lut.shape[0], src.shape[1], src.shape[2]
    if src.dtype == torch.float32:
        return src.shape[0], src.shape[1], src.shape[2], src.shape[3]
    if src.dtype == torch.bfloat16:
        return src.shape[0], src.shape[3], src.shape[1], src.shape[2]
    raise ValueError("augment: source dtype %s (u8 [N,H,W,4], f32 [N,C,H,W] or bf16 [N,H,W,C])" % src.dtype)


def _values(src: torch.Tensor, lut: Optional[torch.Tensor], ic: torch.Tensor, rows: torch.Tensor,
            cols: torch.Tensor, C: int) -> torch.Tensor:
    """``value(ic[b], c, rows[b, y], cols[b, x])`` as ``[B, C, H, W]`` fp32 (coordinates in range)."""
    B, H, W = ic.numel(), rows.shape[1], cols.shape[1]
    if src.dtype == torch.float32:
        return src[ic.view(B, 1, 1, 1), torch.arange(C, device=src.device).view(1, C, 1, 1), rows.view(B, 1, H, 1),
                   cols.view(B, 1, 1, W)]
    pix = src[ic.view(B, 1, 1), rows.view(B, H, 1), cols.view(B, 1, W)]  # [B, H, W, C or 4]
    if src.dtype == torch.uint8:
        return torch.stack([lut[c][pix[..., c].long()] for c in range(C)], 1)
    return pix.permute(0, 3, 1, 2).float()


def _reflect(k: torch.Tensor, n: int) -> torch.Tensor:
    return torch.where(k < 0, -1 - k, torch.where(k >= n, 2 * n - 1 - k, k))


def augment_reference(src: torch.Tensor, idx: torch.Tensor, spec: AugSpec, lut: Optional[torch.Tensor] = None,
                      c8: Optional[int] = None, nhwc: bool = False) -> torch.Tensor:
    """The contract, vectorised. Returns ``[B, C, H, W]`` fp32, ``[B, H, W, c8]`` bf16 when ``c8``
    is given, or ``[B, H, W, C]`` bf16 with ``nhwc``."""
    if nhwc and c8 is not None:
        raise ValueError("augment: nhwc and c8 are mutually exclusive")
    N, C, H, W = _source_geometry(src, lut)
    if c8 is not None and (c8 % 8 or c8 < C):
        raise ValueError("augment: c8 must be a multiple of 8 and >= C, got %d" % c8)
    dev = src.device
    i = idx.to(device=dev, dtype=torch.int64)
    B = i.numel()
    ok = (i >= 0) & (i < N)
    ic = i.clamp(0, max(N - 1, 0))
    ys = torch.arange(H, device=dev).view(1, H)
    xs = torch.arange(W, device=dev).view(1, W)
    if src.dtype == torch.uint8:
        lut = lut.to(device=dev, dtype=torch.float32)
        fill = lut[:, 0]
    else:
        fill = torch.zeros(C, device=dev)
    if spec.translate > 0:
        tx, ty, flip = draws_translate(i, spec, H, W)
        u, v = 256 * xs - tx.view(B, 1), 256 * ys - ty.view(B, 1)  # [B, W], [B, H]
        x0, fx, y0, fy = u >> 8, u & 255, v >> 8, v & 255
        fl = flip.view(B, 1) != 0
        c0, c1 = _reflect(x0, W), _reflect(x0 + 1, W)
        c0, c1 = torch.where(fl, W - 1 - c0, c0), torch.where(fl, W - 1 - c1, c1)
        r0, r1 = _reflect(y0, H), _reflect(y0 + 1, H)
        a, b = _values(src, lut, ic, r0, c0, C), _values(src, lut, ic, r0, c1, C)
        e, d = _values(src, lut, ic, r1, c0, C), _values(src, lut, ic, r1, c1, C)
        fy, fx = fy.view(B, 1, H, 1), fx.view(B, 1, 1, W)
        waa, wab = ((256 - fy) * (256 - fx)).float(), ((256 - fy) * fx).float()  # exact: at most 65536
        wae, wad = (fy * (256 - fx)).float(), (fy * fx).float()
        # one torch op per multiply and per add, in the order of the contract: each is a single fp32
        # operation rounded on its own (nothing here fuses into an FMA), as in the kernel
        top = waa * a
        top = top + wab * b
        bot = wae * e
        bot = bot + wad * d
        val = (top + bot) * (2.0 ** -16)
        valid = ok.view(B, 1, 1, 1).expand(B, 1, H, W)
    else:
        pad = int(spec.pad)
        dx, dy, flip = draws(i, spec)
        sy = ys + dy.view(B, 1) - pad  # [B, H]
        sx = torch.where(flip.view(B, 1) != 0, W - 1 - xs, xs) + dx.view(B, 1) - pad  # [B, W]
        valid = (ok.view(B, 1, 1) & ((sy >= 0) & (sy < H)).view(B, H, 1)
                 & ((sx >= 0) & (sx < W)).view(B, 1, W)).view(B, 1, H, W)
        val = _values(src, lut, ic, sy.clamp(0, H - 1), sx.clamp(0, W - 1), C)
    out = torch.where(valid, val, fill.view(1, C, 1, 1).expand(B, C, H, W)).contiguous()
    if nhwc:
        return out.permute(0, 2, 3, 1).to(torch.bfloat16).contiguous()
    if c8 is None:
        return out
    o = torch.zeros(B, H, W, c8, dtype=torch.bfloat16, device=dev)
    o[..., :C] = out.permute(0, 2, 3, 1).to(torch.bfloat16)
    return o


def hip_supported(src: torch.Tensor, c8: Optional[int], nhwc: bool = False, spec: Optional[AugSpec] = None) -> bool:
    """Whether ``augment_gather`` runs the HIP kernel for this form; translation mode is built for
    the ``nhwc`` destination only."""
    if spec is not None and spec.translate > 0 and not nhwc:
        return False
    dst = "nhwc" if nhwc else ("nchw" if c8 is None else "c8")
    return src.is_cuda and (src.dtype, dst) in _HIP_FORMS


def augment_gather(src: torch.Tensor, idx: torch.Tensor, spec: AugSpec, lut: Optional[torch.Tensor] = None,
                   c8: Optional[int] = None, out: Optional[torch.Tensor] = None, nhwc: bool = False) -> torch.Tensor:
    """The augmented batch of ``src`` at ``idx``: the HIP kernel on a GPU for the forms it is built
    for, ``augment_reference`` otherwise (CPU tensors, the f32 -> C8 / NHWC and bf16 -> NCHW forms,
    and translation into NCHW or C8). ``out`` (the static buffer of a captured step) is written in
    place when given."""
    if nhwc and c8 is not None:
        raise ValueError("augment: nhwc and c8 are mutually exclusive")
    if not hip_supported(src, c8, nhwc, spec):
        ref = augment_reference(src, idx, spec, lut, c8, nhwc)
        if out is None:
            return ref
        out.copy_(ref)
        return out
    from .. import _hipload

    k = _hipload.hipkern()  # a missing build raises: no quiet fall-back on a GPU
    N, C, H, W = _source_geometry(src, lut)
    B = idx.numel()
    if out is None:
        out = (torch.empty(B, H, W, C, device=src.device, dtype=torch.bfloat16) if nhwc else
               torch.empty(B, C, H, W, device=src.device) if c8 is None else
               torch.empty(B, H, W, c8, device=src.device, dtype=torch.bfloat16))
    seed = int(spec.seed) & 0xFFFFFFFFFFFFFFFF
    epoch_t = spec.epoch if torch.is_tensor(spec.epoch) else None
    epoch_i = 0 if epoch_t is not None else int(spec.epoch) & _M32
    rx, ry = translate_range(spec, H, W)
    k.augment_gather(src, lut, idx, out, int(spec.pad), bool(spec.flip), seed & _M32, seed >> 32,
                     int(spec.stream) & _M32, epoch_i, epoch_t, rx, ry, DST_NHWC if nhwc else DST_AUTO)
    return out


