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
``pad = 0, flip = False`` is a plain (normalising) gather.

``augment_reference`` is the contract in integer torch arithmetic (the Philox is
``ops/transformer.py: philox4x32``, shared with the dropout kernels): the oracle of the tests and
the implementation on the CPU. ``augment_gather`` runs the HIP kernel on a GPU.
"""

from __future__ import annotations

import dataclasses
from typing import Optional, Tuple, Union

import torch

from .transformer import philox4x32

_M32 = 0xFFFFFFFF
MAX_PAD = 16

# (source dtype, destination is C8 bf16) pairs the kernel is instantiated for
_HIP_FORMS = {(torch.uint8, False), (torch.float32, False), (torch.uint8, True), (torch.bfloat16, True)}


@dataclasses.dataclass(frozen=True)
class AugSpec:
    """``seed`` is 64-bit, ``stream`` a 32-bit id separating passes that visit the same image in
    one epoch, ``epoch`` an int or a one-element int32 device tensor (the kernel reads it from
    device memory, so a captured graph replays with a new epoch after ``epoch_t.fill_(e)``)."""
    pad: int = 4
    flip: bool = True
    seed: int = 0
    stream: int = 0
    epoch: Union[int, torch.Tensor] = 0

    def __post_init__(self):
        if not 0 <= int(self.pad) <= MAX_PAD:
            raise ValueError("AugSpec: pad must be in [0, %d], got %r" % (MAX_PAD, self.pad))
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


def draws(idx: torch.Tensor, spec: AugSpec) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dx, dy, flip) int64 tensors of the samples with data-set indices ``idx``."""
    i = idx.to(torch.int64)
    epoch = spec.epoch
    if torch.is_tensor(epoch):
        epoch = epoch.reshape(()).to(device=i.device, dtype=torch.int64)
    seed = int(spec.seed)
    w = philox4x32((i & _M32, i >> 32, int(spec.stream), epoch), (seed & _M32, (seed >> 32) & _M32))
    k = 2 * int(spec.pad) + 1
    dx, dy = (w[0] * k) >> 32, (w[1] * k) >> 32
    flip = (w[2] >> 31) if spec.flip else torch.zeros_like(dx)
    return dx, dy, flip


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


def augment_reference(src: torch.Tensor, idx: torch.Tensor, spec: AugSpec, lut: Optional[torch.Tensor] = None,
                      c8: Optional[int] = None) -> torch.Tensor:
    """The contract, vectorised. Returns ``[B, C, H, W]`` fp32, or ``[B, H, W, c8]`` bf16 when
    ``c8`` is given."""
    N, C, H, W = _source_geometry(src, lut)
    dev = src.device
    i = idx.to(device=dev, dtype=torch.int64)
    B = i.numel()
    pad = int(spec.pad)
    dx, dy, flip = draws(i, spec)
    ok = (i >= 0) & (i < N)
    ic = i.clamp(0, max(N - 1, 0))
    ys = torch.arange(H, device=dev).view(1, H)
    xs = torch.arange(W, device=dev).view(1, W)
    sy = ys + dy.view(B, 1) - pad  # [B, H]
    sx = torch.where(flip.view(B, 1) != 0, W - 1 - xs, xs) + dx.view(B, 1) - pad  # [B, W]
    valid = (ok.view(B, 1, 1) & ((sy >= 0) & (sy < H)).view(B, H, 1) & ((sx >= 0) & (sx < W)).view(B, 1, W))
    syc, sxc = sy.clamp(0, H - 1), sx.clamp(0, W - 1)
    if src.dtype == torch.float32:
        val = src[ic.view(B, 1, 1, 1), torch.arange(C, device=dev).view(1, C, 1, 1), syc.view(B, 1, H, 1),
                  sxc.view(B, 1, 1, W)]
        fill = torch.zeros(C, device=dev)
    else:
        pix = src[ic.view(B, 1, 1), syc.view(B, H, 1), sxc.view(B, 1, W)]  # [B, H, W, C or 4]
        if src.dtype == torch.uint8:
            lut = lut.to(device=dev, dtype=torch.float32)
            val = torch.stack([lut[c][pix[..., c].long()] for c in range(C)], 1)
            fill = lut[:, 0]
        else:
            val = pix.permute(0, 3, 1, 2).float()
            fill = torch.zeros(C, device=dev)
    out = torch.where(valid.view(B, 1, H, W), val, fill.view(1, C, 1, 1).expand(B, C, H, W)).contiguous()
    if c8 is None:
        return out
    if c8 % 8 or c8 < C:
        raise ValueError("augment: c8 must be a multiple of 8 and >= C, got %d" % c8)
    o = torch.zeros(B, H, W, c8, dtype=torch.bfloat16, device=dev)
    o[..., :C] = out.permute(0, 2, 3, 1).to(torch.bfloat16)
    return o


def hip_supported(src: torch.Tensor, c8: Optional[int]) -> bool:
    return src.is_cuda and (src.dtype, c8 is not None) in _HIP_FORMS


def augment_gather(src: torch.Tensor, idx: torch.Tensor, spec: AugSpec, lut: Optional[torch.Tensor] = None,
                   c8: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The augmented batch of ``src`` at ``idx``: the HIP kernel on a GPU for the forms it is built
    for, ``augment_reference`` otherwise (CPU tensors, and the f32 -> C8 / bf16 -> NCHW forms).
    ``out`` (the static buffer of a captured step) is written in place when given."""
    if not hip_supported(src, c8):
        ref = augment_reference(src, idx, spec, lut, c8)
        if out is None:
            return ref
        out.copy_(ref)
        return out
    from .. import _hipload

    k = _hipload.hipkern()  # a missing build raises: no quiet fall-back on a GPU
    N, C, H, W = _source_geometry(src, lut)
    B = idx.numel()
    if out is None:
        out = (torch.empty(B, C, H, W, device=src.device) if c8 is None else
               torch.empty(B, H, W, c8, device=src.device, dtype=torch.bfloat16))
    seed = int(spec.seed) & 0xFFFFFFFFFFFFFFFF
    epoch_t = spec.epoch if torch.is_tensor(spec.epoch) else None
    epoch_i = 0 if epoch_t is not None else int(spec.epoch) & _M32
    k.augment_gather(src, lut, idx, out, int(spec.pad), bool(spec.flip), seed & _M32, seed >> 32,
                     int(spec.stream) & _M32, epoch_i, epoch_t)
    return out
