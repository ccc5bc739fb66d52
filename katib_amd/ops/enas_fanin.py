"""Gradient fan-in of an ENAS child layer (``csrc/hip/enas_fanin.hip``).

Layer ``i`` of the child is read by layer ``i + 1`` and by every later layer whose skip bit selects
it, each through its own :func:`~katib_amd.ops.enas_concat.relu_pad_concat`. Left to autograd, every
reader writes a full-size gradient of the layer (reading the layer again for its ReLU mask) and the
engine folds them with one bf16 add per extra reader. Here the readers only *record* their
contribution - their output gradient, read in place, the channel offset and pad of the layer inside
it, ReLU or not - in the layer's :class:`Fan`, and one kernel forms the sum: ``n`` gradient reads, one
mask read, one write, one rounding from an fp32 sum.

``x, fan = share(x)`` marks a layer output; ``relu_pad_concat(xs, relu, pad8, fans=[...])`` takes the
fans of its sources. :func:`share`'s backward runs after every reader's (the engine orders it so even
when all of them return ``None``), launches the kernel over the ledger followed by the ordinary incoming
gradient, if there is one, and spends the fan: a second backward over the same graph raises.
On the CPU the same sum is formed in torch ops.
"""

from __future__ import annotations

from typing import List, Optional, Tuple

import torch
from torch.autograd.function import once_differentiable

from .conv import kernels

MAX_TERMS = 16  # csrc/hip/enas_fanin.h: kMaxTerms


def pixel_stride(g: torch.Tensor) -> int:
    """Of an NHWC view: from the first dimension that has one (a dimension of size 1 has no say)."""
    B, m, _, Cg = g.shape
    return g.stride(2) if m > 1 else (g.stride(0) if B > 1 else (Cg + 7) // 8 * 8)


def readable(g: torch.Tensor) -> bool:
    """``g`` [B, m, m, Cg] can be a term as it lies: bf16, channels adjacent, dense up to a pixel stride
    that is a multiple of 8, 16-byte base, 32-bit indices."""
    B, m, _, Cg = g.shape
    gs = pixel_stride(g)
    return (g.dtype == torch.bfloat16 and (Cg == 1 or g.stride(3) == 1) and gs >= Cg and gs % 8 == 0
            and (m == 1 or g.stride(1) == m * gs) and (B == 1 or g.stride(0) == m * m * gs)
            and g.data_ptr() % 16 == 0 and B * m * m * gs < 2 ** 31)


class Fan:
    """The ledger of one layer output ``x`` ([B, C, H, H]) for one forward: ``(g, off, relu)`` per reader
    that deferred its contribution, in the order the readers' backwards ran."""

    def __init__(self, x: torch.Tensor):
        self.x: Optional[torch.Tensor] = x
        self.terms: List[Tuple[torch.Tensor, int, bool]] = []
        self.shift = 0  # the one non-zero off % 8 a launch serves
        self.spent = False

    def _live(self):
        if self.spent:
            raise RuntimeError("enas_fanin: this graph's gradient fans are spent by an earlier backward; a second "
                               "backward needs a new forward")

    def nhwc(self) -> torch.Tensor:
        """The producer as a dense [B, H, H, C] tensor: the ReLU mask of a reader that does not defer."""
        self._live()
        return self.x.permute(0, 2, 3, 1).contiguous()

    def add(self, g: torch.Tensor, off: int, relu: bool) -> bool:
        """Record a reader's output gradient ``g`` ([B, m, m, Cg], this layer at channels ``off ..``) if it
        fits the kernel's contract; ``False`` leaves the reader on its own path."""
        self._live()
        if g.is_cuda:
            sh = off % 8
            if (len(self.terms) >= MAX_TERMS - 1 or not readable(g) or g.shape[1] < self.x.shape[2]
                    or (sh and self.shift not in (0, sh))):
                return False
            self.shift = sh or self.shift
        self.terms.append((g, int(off), bool(relu)))
        return True

    def collect(self, g: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        """The layer's gradient from the ledger and the incoming gradient ``g`` ([B, C, H, H] or None)."""
        self._live()
        x, terms = self.x, self.terms
        self.x, self.terms, self.spent = None, [], True
        if g is not None:
            gn = g.permute(0, 2, 3, 1)
            if x.is_cuda and not readable(gn):
                gn = gn.to(torch.bfloat16).clone(memory_format=torch.contiguous_format)
            terms = terms + [(gn, 0, False)]
        if not terms:
            return None
        B, C, H, _ = x.shape
        if x.is_cuda:
            gx = torch.empty((B, H, H, C), device=x.device, dtype=torch.bfloat16)
            xn = x.permute(0, 2, 3, 1).contiguous() if any(r for _, _, r in terms) else None
            kernels().enas_fanin(xn, terms, gx)
            return gx.permute(0, 3, 1, 2)
        acc = torch.float64 if x.dtype == torch.float64 else torch.float32
        masked = torch.zeros((B, H, H, C), dtype=acc)
        plain = torch.zeros((B, H, H, C), dtype=acc)
        for gk, off, relu in terms:
            t = (gk.shape[1] - H) // 2
            (masked if relu else plain).add_(gk[:, t:t + H, t:t + H, off:off + C].to(acc))
        keep = ~(x.permute(0, 2, 3, 1) <= 0)  # as the kernels: x <= 0 drops, a NaN does not
        return (torch.where(keep, masked, torch.zeros((), dtype=acc)) + plain).to(x.dtype).permute(0, 3, 1, 2)


class _ShareFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, fan):
        ctx.set_materialize_grads(False)  # no reader outside the fans: None, not a tensor of zeros
        ctx.fan = fan
        return x.view_as(x)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return ctx.fan.collect(g), None


def servable(x: torch.Tensor) -> bool:
    """Layer outputs the fan-in serves: anything on the CPU; on a GPU, bf16 with ``C % 8 == 0``."""
    return x.dim() == 4 and x.shape[2] == x.shape[3] and x.numel() > 0 and (
        not x.is_cuda or (x.dtype == torch.bfloat16 and x.shape[1] % 8 == 0 and x.numel() < 2 ** 31))


def share(x: torch.Tensor) -> Tuple[torch.Tensor, Fan]:
    """``(x_view, fan)``: hand ``x_view`` to every reader of ``x`` and ``fan`` to the ``relu_pad_concat``
    calls among them. Raises for an ``x`` the fan-in does not serve (see :func:`servable`)."""
    if not servable(x):
        raise ValueError("enas_fanin.share: [B, C, H, H] with C % 8 == 0 in bf16 on a GPU, got %s %s"
                         % (tuple(x.shape), x.dtype))
    fan = Fan(x)
    return _ShareFn.apply(x, fan), fan
