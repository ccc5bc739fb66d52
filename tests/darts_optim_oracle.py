"""References for the DARTS optimizer kernels (csrc/hip/darts_optim.hip) and the replica folds
(csrc/hip/darts_ops.hip), in torch on the CPU. Two per kernel:

(a) an exact-order fp32 oracle: one torch op per arithmetic operation in the order the kernel
    header documents, scalars cast to fp32 first as the bindings do. ``x.add(y, alpha=c)`` is
    never used (on the CPU it contracts into an FMA); every product is materialised before it is
    added. Norms are ``float32(sqrt_fp64(fp64 sum of squares))``.
(b) an fp64 reference of the mathematics, from torch's own optimizers where one exists.

A plain helper module of the tests (tests/test_darts_optim_oracle.py validates it without a GPU,
tests/test_gpu_darts_optim.py compares the kernels with it).
"""
import torch

F32, F64 = torch.float32, torch.float64
THREADS = 256
MAX_PARTS = 256
ALPHA_GRAD_MAX = 128
ULP = 2.0 ** -23


def s32(x):
    """A scalar as the bindings pass it: rounded to fp32 (0-dim tensor)."""
    if isinstance(x, torch.Tensor):
        return x.detach().to("cpu", F32).reshape(())
    return torch.tensor(float(x), dtype=F32)


# ------------------------------------------------------------------------------ norms
def sumsq_total(x):
    """fp64 sum of squares (0-dim fp64)."""
    return x.to(F64).square().sum()


def sumsq_nparts(n):
    """Partials sumsq writes for n elements: one per workgroup of 8 * 256 elements, capped."""
    return max(1, min(-(-n // (THREADS * 8)), MAX_PARTS))


def norm32(x):
    return sumsq_total(x).sqrt().to(F32)


def norm_is_stable(x, rel=1e-9):
    """True when a relative error of ``rel`` in the fp64 norm cannot move its fp32 rounding: the
    device sums the squares in another order (error <= n 2^-53) and takes its own fp64 sqrt, both
    far inside 1e-9, so for such inputs the fp32 norm is the oracle's bit for bit."""
    s = sumsq_total(x).sqrt()
    return bool((s * (1.0 - rel)).to(F32) == (s * (1.0 + rel)).to(F32))


def eps_of(d):
    """eps = float32(0.01) / float32(||d||)."""
    return s32(0.01) / norm32(d)


def clip_coef(g, clip):
    """coef = min(clip / (norm + float32(1e-6)), 1)."""
    return torch.minimum(s32(clip) / (norm32(g) + s32(1e-6)), s32(1.0))


# ------------------------------------------------------------------------------ (a) fp32, exact order
def virtual_step(w, mom, g, lr, mu, wd):
    """w' = w + (-lr) * ((mu * mom + g) + wd * w)."""
    lr, mu, wd = s32(lr), s32(mu), s32(wd)
    v = (mom * mu + g) + w * wd
    return v * (-lr) + w


def hessian_step(phase, w, d, eps):
    """Sequential phases: 0 and 2 add d * eps, 1 adds d * -(2 eps)."""
    eps = s32(eps)
    scale = -(s32(2.0) * eps) if phase == 1 else eps
    return w + d * scale


def hessian_alpha_grad(gap, ga, gav, eps, lr):
    """alpha_grad = gav - ((gap - ga) / (2 eps)) * lr."""
    h = (gap - ga) / (s32(2.0) * s32(eps))
    return gav - h * s32(lr)


def hessian_split(w, d, eps):
    """Phase 3: wp = w + d * eps; wm = wp + d * -(2 eps)."""
    eps = s32(eps)
    wp = w + d * eps
    return wp, wp + d * (-(s32(2.0) * eps))


def bn_merge(bn, bn_plus, bn_zero, momentum):
    """(k * bn_plus + bn) - k * bn_zero with k = 1.0f - float32(momentum)."""
    k = s32(1.0) - s32(momentum)
    return (bn_plus * k + bn) - bn_zero * k


def sgd_clip(w, g, mom, lr, clip, mu, wd):
    """-> (w', clipped g, mom'): g' = g * coef; m = mu * mom + (g' + wd * w); w' = w - m * lr."""
    lr, mu, wd = s32(lr), s32(mu), s32(wd)
    gc = g * clip_coef(g, clip)
    m = mom * mu + (gc + w * wd)
    return w - m * lr, gc, m


def adam_torch_branch(a, grad, m, v, t, lr, wd, b1=0.5, b2=0.999, eps=1e-8):
    """The arithmetic of DartsSearch._seg_alpha_step's torch branch, op for op, on copies:
    -> (a', m', v', t')."""
    a, m, v, t = a.clone(), m.clone(), v.clone(), s32(t).clone()
    g = grad + wd * a
    t.add_(1.0)
    m.mul_(b1).add_(g, alpha=1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    bc1 = 1 - torch.pow(b1, t)
    bc2 = 1 - torch.pow(b2, t)
    denom = (v.sqrt() / bc2.sqrt()).add_(eps)
    a.sub_(m / denom * (lr / bc1))
    return a, m, v, t


# ------------------------------------------------------------------------------ (b) fp64 mathematics
def virtual_step64(w, mom, g, lr, mu, wd):
    w, mom, g = w.to(F64), mom.to(F64), g.to(F64)
    return w - float(lr) * (float(mu) * mom + g + float(wd) * w)


def architect64(w, d, gap, ga, gav, lr):
    """The architect's closed forms -> (eps, w + eps d, w - eps d, alpha_grad)."""
    w, d = w.to(F64), d.to(F64)
    eps = 0.01 / d.norm()
    h = (gap.to(F64) - ga.to(F64)) / (2.0 * eps)
    return eps, w + eps * d, w - eps * d, gav.to(F64) - float(lr) * h


def sgd_clip64(w, g, mom, lr, clip, mu, wd):
    """clip_grad_norm_ + torch.optim.SGD(momentum, weight_decay) -> (w', clipped g, mom')."""
    p = torch.nn.Parameter(w.to(F64).clone())
    p.grad = g.to(F64).clone()
    opt = torch.optim.SGD([p], lr=float(lr), momentum=float(mu), weight_decay=float(wd))
    opt.state[p]["momentum_buffer"] = mom.to(F64).clone()
    torch.nn.utils.clip_grad_norm_([p], float(clip))
    gc = p.grad.clone()
    opt.step()
    return p.detach(), gc, opt.state[p]["momentum_buffer"]


class Adam64:
    """torch.optim.Adam(betas, weight_decay) in fp64 with the hyperparameters first rounded to
    fp32 as the binding rounds them, started from given moments and step count."""

    def __init__(self, a, m, v, t, lr, wd, b1=0.5, b2=0.999, eps=1e-8):
        r = lambda x: float(s32(x))
        self.p = torch.nn.Parameter(a.to(F64).clone())
        self.opt = torch.optim.Adam([self.p], lr=r(lr), betas=(r(b1), r(b2)), eps=r(eps), weight_decay=r(wd))
        self.opt.state[self.p] = {"step": torch.tensor(float(t)), "exp_avg": m.to(F64).clone(),
                                  "exp_avg_sq": v.to(F64).clone()}

    def step(self, grad):
        """-> (a', m', v') after one step with this gradient."""
        self.p.grad = grad.to(F64).clone()
        self.opt.step()
        st = self.opt.state[self.p]
        return self.p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()


def softmax64(x):
    return torch.softmax(x.to(F64), dim=-1)


def softmax_tol(K):
    """Relative bound of the fp32 softmax against fp64: K - 1 additions, the exps (argument
    subtraction and exp itself), and the divide."""
    return (K + 6) * ULP


def alpha_grad64(entries, rep, K, dst=None):
    """entries: (g [f64, rep replicas rstride apart], rstride, w [K], row index). Per destination
    row the sum over its entries of w_k (g_k - sum_j w_j g_j) in fp64, rounded to fp32 and, with
    ``dst`` ([rows][K] fp32), added to it in fp32. -> {row index: [K] fp32}."""
    acc = {}
    for g, rs, w, r in entries:
        gs = torch.stack([g[q * rs:q * rs + K] for q in range(rep)]).to(F64).sum(0)
        w = w.to(F64)
        acc[r] = acc.get(r, torch.zeros(K, dtype=F64)) + w * (gs - (w * gs).sum())
    return {r: (dst[r] + v.to(F32)) if dst is not None else v.to(F32) for r, v in acc.items()}


def fold_rows_ref(buf):
    """Row 0 = the rows summed in row order (fp32), rows 1.. zero."""
    out = torch.zeros_like(buf)
    acc = buf[0].clone()
    for r in range(1, buf.shape[0]):
        acc = acc + buf[r]
    out[0] = acc
    return out


# ------------------------------------------------------------------------------ inputs
def dyadic(shape, g, kmax=1024, denom=64.0, dtype=F32):
    """k / denom with integer |k| <= kmax: squares, products with dyadic weights and fp64 sums of
    them are exact in any order."""
    shape = shape if isinstance(shape, tuple) else (shape,)
    return torch.randint(-kmax, kmax + 1, shape, generator=g, dtype=torch.int32).to(dtype) / denom


def softmax_inputs(rows, K, seed):
    """Production scale, spread over +-80 (the max subtraction matters), all-equal rows.

    The spread logits lie in [-80, 80] on a grid of 2^-10, at most 80 apart within a row. A bound
    relative to each weight needs both: weights below e^-87 are not normal fp32 numbers, and
    off-grid logits 80 apart make x - max itself round (2^-18 of the weight, above the bound),
    which is the input's representation and no rounding of the softmax under test."""
    g = torch.Generator().manual_seed(seed)
    grid = lambda *shape: torch.randint(0, 80 * 1024 + 1, shape, generator=g).to(F32) / 1024.0
    spread = grid(rows, 1) - grid(rows, K)
    spread[::2] = -spread[::2]
    return {"production": 1e-3 * torch.randn(rows, K, generator=g), "spread": spread,
            "equal": torch.full((rows, K), 0.37)}


def first_stable(make, seed, tries=8):
    """``make(generator)`` -> the vector whose norm a kernel takes. Returns make's result for the
    first seed >= ``seed`` at which that norm passes norm_is_stable (1-2 % of totals do not), and
    the seed. Deterministic on the CPU; the callers assert the condition again on what they use."""
    for s in range(seed, seed + tries):
        x = make(torch.Generator().manual_seed(s))
        if norm_is_stable(x):
            return x, s
    raise AssertionError("no seed in [%d, %d) gives a stable fp32 norm" % (seed, seed + tries))


def ulp_err(got, want, scale=None):
    """max |got - want| in units of 2^-23 of ``scale`` (default max |want|)."""
    scale = float(want.abs().max()) if scale is None else float(scale)
    if scale == 0.0:
        return float((got.to(F64) - want.to(F64)).abs().max())
    return float((got.to(F64) - want.to(F64)).abs().max()) / (scale * ULP)
