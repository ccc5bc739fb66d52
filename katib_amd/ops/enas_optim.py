"""Adam of an ENAS child in one HIP launch (``csrc/hip/enas_optim.hip``): the update of every parameter,
the zeroing of the gradient buffers, the sum of the depthwise partial gradients, the weight images the
convolution kernels read and the step counter.

:class:`ChildAdam` is ``torch.optim.Adam`` with default flags over a ``ChildNet``. It sorts the
parameters into three kinds of segment (``enas_optim.h``):

* conv - the weight of a groups-1 ``_SameConv`` / ``ops.conv.Conv2d`` the implicit-GEMM kernels serve.
  The optimizer owns the fp32 master in ``[K][RS][C]`` memory order (the parameter's ``.data`` becomes a
  view of it; name, shape and values are unchanged), the fp32 accumulator ``[K][RS][C8]`` ``conv_wgrad``
  adds into, and the bf16 images ``[K][RS][C8]`` and ``[C8][RS][K]`` (the latter only where the layer's
  input wants a gradient);
* depthwise - the weight of a depthwise ``_SameConv`` with ``C % 8 == 0``: master ``[Co][KK]``, the
  partials ``[rows][Co][KK]`` ``dw_wgrad`` writes (allocated by the first backward, which knows the
  geometry) and the fp32 tap-major image ``[KK][Co]``;
* flat - everything else, fed from the parameter's ``.grad``, which the launch zeroes.

The layers find their buffers through the ``prep`` record attached to the module and hand it to
``ops.conv._ConvFn`` / ``ops.dwconv._DwFn`` / ``ops.enas_sepconv._SepFn``, which then take their weight images
from it and leave their weight gradients in it; the ``.grad`` of such a weight stays None. Which layers get a
record is decided by the ``weight_supported`` of ``ops.conv`` / ``ops.dwconv``, the layer's half of the test
their forward makes; a layer with a record raises where its forward would leave the HIP kernels.
"""

from __future__ import annotations

import torch
import torch.nn as nn

from . import conv as hconv, dwconv as hdw
from .conv import kernels

FLAT, CONV, DEPTHWISE = 0, 1, 2


class _Seg:
    """One parameter: its buffers, and for a conv / depthwise weight the ``prep`` record of its layer."""

    def __init__(self, opt, name, param, kind, dgrad=True):
        dev = param.device
        self.opt, self.name, self.param, self.kind = opt, name, param, kind
        self.shape = tuple(param.shape)
        w = param.detach()
        self.wk = self.wt = self.img = self.g = None
        self.rows = 0
        if kind == CONV:
            K, C, R, S = self.shape
            self.K, self.C, self.RS, self.C8 = K, C, R * S, (C + 7) // 8 * 8
            self.p = w.permute(0, 2, 3, 1).contiguous().clone()  # [K][R][S][C]
            param.data = self.p.permute(0, 3, 1, 2)
            self.g = torch.zeros(K * self.RS * self.C8, device=dev)
            self.wk = torch.empty(K * self.RS * self.C8, device=dev, dtype=torch.bfloat16)
            self.wt = torch.empty_like(self.wk) if dgrad else None
        elif kind == DEPTHWISE:
            Co, _, K, _ = self.shape
            self.K, self.C, self.RS = Co, 0, K * K
            self.p = w.reshape(Co, K * K).clone()
            param.data = self.p.view(self.shape)
            self.img = torch.empty(K * K, Co, device=dev)
        else:
            self.K = self.C = self.RS = 0
            self.p = w.reshape(-1).clone()
            param.data = self.p.view(self.shape)
            param.grad = torch.zeros(self.shape, device=dev)
            self.g = param.grad
        self.m, self.v = torch.zeros_like(self.p), torch.zeros_like(self.p)

    def partials(self, rows: int) -> torch.Tensor:
        """The ``[rows][Co][KK]`` buffer of a depthwise layer's backward; a new ``rows`` makes a new buffer
        and the optimizer rebuild its table before the next launch."""
        if self.g is None or self.rows != rows:
            self.g = torch.empty(rows, self.K, self.RS, device=self.p.device)
            self.rows = rows
            self.opt._table = None
        return self.g

    def torch_view(self, t: torch.Tensor) -> torch.Tensor:
        """A master-layout tensor (p, m, v) in the parameter's torch shape."""
        if self.kind == CONV:
            K, C, R, S = self.shape
            return t.view(K, R, S, C).permute(0, 3, 1, 2)
        return t.view(self.shape)

    def grad(self) -> torch.Tensor:
        if self.kind == CONV:
            K, C, R, S = self.shape
            return self.g.view(K, R, S, self.C8)[..., :C].permute(0, 3, 1, 2).clone()
        if self.kind == DEPTHWISE:
            if self.g is None:
                raise RuntimeError("ChildAdam: %s has seen no backward yet" % self.name)
            return self.g.double().sum(0).float().view(self.shape)
        return self.g.clone()

    def entry(self, update: bool):
        if update and self.g is None:
            raise RuntimeError("ChildAdam.step(): %s has seen no backward yet" % self.name)
        img = self.wk if self.kind == CONV else self.img
        g = self.g if self.g is not None else self.p
        return (self.kind, self.p, g, self.m, self.v, img, self.wt, self.K, self.C, self.RS, max(self.rows, 1))


class ChildAdam:
    def __init__(self, model: nn.Module, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8):
        params = dict(model.named_parameters())
        if not params or not all(p.is_cuda and p.dtype == torch.float32 for p in params.values()):
            raise ValueError("ChildAdam: the HIP optimizer needs a model with fp32 parameters on a GPU")
        self.k = kernels()
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        # a layer fed by the image alone: the first convolution of its body has nothing to send a gradient to
        no_dgrad = {id(op.body[0]) for op, ins in zip(getattr(model, "ops", []), getattr(model, "inputs", []))
                    if ins == [0] and hasattr(op, "body")}
        kinds = {}
        for mname, mod in model.named_modules():
            c = mod if isinstance(mod, hconv.Conv2d) else getattr(mod, "conv", None)
            if not isinstance(c, nn.Conv2d) or not (mod is c or hasattr(mod, "s")):
                continue
            wname = (mname + "." if mname else "") + ("weight" if mod is c else "conv.weight")
            # the layer's side of what its forward asks (``supported`` there adds the input's side, and raises
            # on a fallback once ``prep`` is attached); the depthwise kernels run unpadded only: C % 8 == 0
            if hconv.weight_supported(c.weight, c.groups):
                if mod is not c or (c.padding_mode == "zeros" and isinstance(c.padding, tuple)):
                    kinds[wname] = (CONV, mod)
            elif (mod is not c and c.groups == c.in_channels and c.in_channels % 8 == 0
                  and hdw.weight_supported(c.weight, c.groups, mod.s)):
                kinds[wname] = (DEPTHWISE, mod)
        self.segs = []
        for name, p in params.items():
            kind, mod = kinds.get(name, (FLAT, None))
            seg = _Seg(self, name, p, kind, dgrad=id(mod) not in no_dgrad)
            if mod is not None:
                mod.prep = seg
            self.segs.append(seg)
        self.counters = torch.zeros(2, dtype=torch.int32, device=self.segs[0].p.device)  # t, ticket
        self._table = None
        self.refresh()

    @property
    def t(self) -> torch.Tensor:
        """The device count of completed updates (int32, one element)."""
        return self.counters[:1]

    def _launch(self, update: bool):
        # two tables: the image launch runs before any backward has sized the depthwise partials, which it
        # never reads (their place is held by the master), and skips the flat segments
        if self._table is None:
            self._table = {}
        if update not in self._table:
            segs = self.segs if update else [s for s in self.segs if s.kind != FLAT]
            self._table[update] = self.k.enas_adam_table([s.entry(update) for s in segs])
        table, nseg, tiles = self._table[update]
        self.k.enas_adam(table, nseg, tiles, self.counters, self.lr, self.betas[0], self.betas[1], self.eps, update)

    def refresh(self):
        """Write the images from the masters (initialisation, ``load_state_dict``); nothing else changes."""
        if any(s.kind != FLAT for s in self.segs):
            self._launch(False)

    def step(self):
        self._launch(True)

    def grads(self):
        """Parameter name -> the gradient the next ``step()`` would consume, in the parameter's torch shape
        (accumulators sliced, partials summed in fp64). For tests and debugging."""
        return {s.name: s.grad() for s in self.segs}

    def state_dict(self):
        sd = {"step": int(self.counters[0])}
        for s in self.segs:
            sd["exp_avg." + s.name] = s.torch_view(s.m).clone()
            sd["exp_avg_sq." + s.name] = s.torch_view(s.v).clone()
        return sd

    def load_state_dict(self, sd):
        for s in self.segs:
            s.torch_view(s.m).copy_(sd["exp_avg." + s.name])
            s.torch_view(s.v).copy_(sd["exp_avg_sq." + s.name])
        self.counters.copy_(torch.tensor([int(sd["step"]), 0], dtype=torch.int32))
        self.refresh()
