"""Reference for one ``HipCNN`` train step (katib_amd/workloads/mnist_cnn.py on the kernels of
csrc/hip/mnist_cnn.hip and csrc/hip/mlp.hip), in torch ops on the CPU, in torch's layout throughout.

``train_step`` walks the step the way ``HipCNN.train_step`` does - forward, cross-entropy and its
gradient, then from the top layer down the dgrad through the pre-update weight and that layer's
weight / bias gradient and SGD update - with two knobs:

``gemm_dtype``  fp32 or fp64: the type every convolution, matrix product, softmax and sum runs in.
``round``       ``torch.bfloat16`` or ``None``: applied where the kernels round - the images, the weight
                shadows, ``p1``, ``p2``, the ``fc1`` activations, the logits, ``dl``, ``dh``, ``dp2``, ``dp1``.

Bias and ReLU act on the unrounded accumulators; the 2x2 maximum is taken over those four values
before rounding, the first maximum in row-major window order wins (``F.max_pool2d``'s rule), and the
ReLU derivative is the mask ``p > 0`` on the pooled value. Masters and momentum stay fp32 (fp64 when
``gemm_dtype`` is fp64 and ``round`` is None). The update is not re-derived: it is ``torch.optim.SGD``
stepped on parameters whose ``grad`` and ``momentum_buffer`` are preset.

The per-kernel pieces (``conv_pool_fwd``, ``conv_dgrad``, ``conv_wgrad``) are what the GPU file compares
each kernel with; ``state_failures`` / ``exact_mismatches`` / ``near_tie`` are the checkers it uses, and
``MUTANTS`` are wrong steps those checkers must reject (tests/test_mnist_cnn_oracle.py).
"""
import torch
import torch.nn.functional as F

from katib_amd.workloads import mnist_cnn

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
PARAMS = mnist_cnn.PARAMS
MUTANTS = ("tie_last", "fc1_kernel_cols", "dampening", "zero_window_grad", "post_update_dgrad")


def state_dtype(gemm_dtype, round):
    return F64 if gemm_dtype == F64 and round is None else F32


def _r(v, gd, round):
    return v.to(round).to(gd) if round is not None else v.to(gd)


def state_from_module(model, dtype=F32):
    """(parameters, zero momentum buffers) as name -> tensor in the module's layout."""
    p = {n: t.detach().to("cpu", dtype).clone() for n, t in model.state_dict().items()}
    return p, {n: torch.zeros_like(t) for n, t in p.items()}


# ------------------------------------------------------------------------------ pooling
def windows(z):
    """[B, C, H, W] -> [B, C, H/2, W/2, 4]: each 2x2 window's values in row-major order."""
    B, C, H, W = z.shape
    return z.reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)


def first_max(w, last=False):
    """Maximum of the last axis and the position of its first (``last``: last) occurrence."""
    best = w.max(-1).values
    eq = w == best[..., None]
    if last:
        return best, 3 - (eq.flip(-1).cumsum(-1) == 0).sum(-1)
    return best, (eq.cumsum(-1) == 0).sum(-1)


def unpool(dp, win):
    """dp [B, C, H, W] placed at each window's winner, zeros elsewhere -> [B, C, 2H, 2W]."""
    B, C, H, W = dp.shape
    d = torch.zeros(B, C, H, W, 4, dtype=dp.dtype).scatter_(-1, win[..., None], dp[..., None])
    return d.view(B, C, H, W, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, 2 * H, 2 * W)


# ------------------------------------------------------------------------------ per-kernel pieces
def conv_pool_fwd(x, w, b, gemm_dtype=F32, round=None, tie_last=False):
    """pool(relu(conv5x5(x, w) + b)): the rounded pooled values, the winners (int64 0..3) and the
    unrounded pre-ReLU window values [B, C, H, W, 4]."""
    gd = gemm_dtype
    wz = windows(F.conv2d(_r(x, gd, round), _r(w, gd, round)) + b.to(gd)[None, :, None, None])
    best, win = first_max(torch.relu(wz), last=tie_last)
    return _r(best, gd, round), win, wz


def conv_dgrad(dp, win, w, p_in, gemm_dtype=F32, round=None, mask=True):
    """Gradient of the convolution's input: dz (dp at the winners) correlated with the flipped filter,
    masked by the ReLU derivative of the layer below (p_in > 0), rounded."""
    gd = gemm_dtype
    d = F.conv_transpose2d(unpool(_r(dp, gd, round), win), _r(w, gd, round))
    return _r(d * (p_in > 0) if mask else d, gd, round)


def conv_wgrad(dp, win, inp, gemm_dtype=F32, round=None):
    """(dW [Co, Ci, 5, 5], db [Co]) of the convolution from the pooled gradient and the winners."""
    gd = gemm_dtype
    dz = unpool(_r(dp, gd, round), win)
    patches = F.unfold(_r(inp, gd, round), 5)  # [B, Ci * 25, L]
    gw = torch.einsum("bol,bkl->ok", dz.flatten(2), patches).view(dz.shape[1], inp.shape[1], 5, 5)
    return gw, dz.sum((0, 2, 3))


def sgd_step(pairs, lr, momentum, dampening=0.0):
    """One step of torch.optim.SGD on ``pairs`` = [(value, grad, momentum buffer)] -> [(value, buffer)]."""
    params = [torch.nn.Parameter(v.clone()) for v, _, _ in pairs]
    opt = torch.optim.SGD(params, lr=lr, momentum=momentum, dampening=dampening)
    for p, (_, g, buf) in zip(params, pairs):
        p.grad = g.to(p.dtype).clone()
        opt.state[p]["momentum_buffer"] = buf.clone()
    opt.step()
    return [(p.detach(), opt.state[p]["momentum_buffer"]) for p in params]


# ------------------------------------------------------------------------------ the step
def train_step(p, m, x, y, lr, momentum, gemm_dtype=F32, round=None, mutant=None):
    """One train step on ``p`` / ``m`` (name -> tensor, the module's layout, updated in place). ``x``
    [B, 1, 28, 28]: the minibatch, already gathered; ``y`` [B]. Returns the intermediates and the
    pre-SGD gradients (``g.<name>``), all in torch's layout."""
    assert mutant is None or mutant in MUTANTS
    gd, sd = gemm_dtype, state_dtype(gemm_dtype, round)
    B = x.shape[0]
    tie_last, mask = mutant == "tie_last", mutant != "zero_window_grad"

    def r(v):
        return _r(v, gd, round)

    def update(name, gw, gb):
        (w, wm), (b, bm) = sgd_step([(p[name + ".weight"].to(sd), gw.to(sd), m[name + ".weight"].to(sd)),
                                     (p[name + ".bias"].to(sd), gb.to(sd), m[name + ".bias"].to(sd))],
                                    lr, momentum, momentum if mutant == "dampening" else 0.0)
        p[name + ".weight"], m[name + ".weight"], p[name + ".bias"], m[name + ".bias"] = w, wm, b, bm

    out = {}
    x0 = r(x)
    p1, a1, _ = conv_pool_fwd(x0, p["conv1.weight"], p["conv1.bias"], gd, round, tie_last)
    p2, a2, _ = conv_pool_fwd(p1, p["conv2.weight"], p["conv2.bias"], gd, round, tie_last)
    f = p2.flatten(1)
    h = r(torch.relu(f @ r(p["fc1.weight"]).t() + p["fc1.bias"].to(gd)))
    logits = r(h @ r(p["fc2.weight"]).t() + p["fc2.bias"].to(gd))
    lsm = torch.log_softmax(logits, 1)
    loss = -lsm[torch.arange(B), y].mean()
    d = lsm.exp()
    d[torch.arange(B), y] -= 1.0
    dl = r(d / B)
    out.update(p1=p1, a1=a1, p2=p2, a2=a2, h=h, logits=logits, dl=dl, loss=float(loss))

    def dgrad_w(name):  # the weight a dgrad reads: the shadow from before this step's update of the layer
        return r(p[name + ".weight"])

    w_fc2 = dgrad_w("fc2")
    gw, gb = dl.t() @ h, dl.sum(0)
    out["g.fc2.weight"], out["g.fc2.bias"] = gw, gb
    if mutant == "post_update_dgrad":
        update("fc2", gw, gb)
        w_fc2 = dgrad_w("fc2")
    dh = r((dl @ w_fc2) * (h > 0))
    if mutant != "post_update_dgrad":
        update("fc2", gw, gb)

    w_fc1 = dgrad_w("fc1")
    gw, gb = dh.t() @ f, dh.sum(0)
    out["g.fc1.weight"], out["g.fc1.bias"] = gw, gb
    if mutant == "post_update_dgrad":
        update("fc1", gw, gb)
        w_fc1 = dgrad_w("fc1")
    dp2 = (dh @ w_fc1)
    dp2 = r(dp2 * (f > 0) if mask else dp2).view_as(p2)
    if mutant != "post_update_dgrad":
        update("fc1", gw, gb)

    gw, gb = conv_wgrad(dp2, a2, p1, gd, round)
    out["g.conv2.weight"], out["g.conv2.bias"] = gw, gb
    if mutant == "post_update_dgrad":
        update("conv2", gw, gb)
    dp1 = conv_dgrad(dp2, a2, p["conv2.weight"], p1, gd, round, mask)
    if mutant != "post_update_dgrad":
        update("conv2", gw, gb)

    gw, gb = conv_wgrad(dp1, a1, x0, gd, round)
    out["g.conv1.weight"], out["g.conv1.bias"] = gw, gb
    update("conv1", gw, gb)
    out.update(dh=dh, dp2=dp2, dp1=dp1)
    return out


def state_dict(p, m, mutant=None):
    """The oracle's state under ``HipCNN.state_dict()``'s names. Mutant ``fc1_kernel_cols``: the fc1
    columns as the kernels keep them, (pooled pixel, channel), not permuted back."""
    out = {n: p[n].clone() for n in PARAMS}
    out.update({"momentum_buffer." + n: m[n].clone() for n in PARAMS})
    if mutant == "fc1_kernel_cols":
        for n in ("fc1.weight", "momentum_buffer.fc1.weight"):
            out[n] = out[n].view(500, 50, 16).permute(0, 2, 1).reshape(500, 800).contiguous()
    return out


# ------------------------------------------------------------------------------ checkers
def rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-6))


def state_failures(got, ref32, ref64, before, label="", out=print):
    """Momentum buffers and updates (new - before) of ``got`` against the fp32-GEMM oracle, each held to
    the larger of 1e-2 and four times the fp32-GEMM oracle's own distance from the fp64-GEMM one. All
    four are ``state_dict()``s. Prints every figure; returns the list of (name, figure, bar) that miss."""
    fails = []
    for n in PARAMS:
        mb = "momentum_buffer." + n
        for name, g, a, b in ((mb, got[mb], ref32[mb], ref64[mb]),
                              (n + " upd", got[n].cpu().double() - before[n].double(),
                               ref32[n].double() - before[n].double(), ref64[n].double() - before[n].double())):
            if g.shape != a.shape:
                fails.append((name, "shape", tuple(g.shape)))
                continue
            bar, fig = max(1e-2, 4 * rel(a, b)), rel(g, a)
            out("%s %-32s %.2e/%.2e" % (label, name, fig, bar))
            if not fig < bar:
                fails.append((name, fig, bar))
    return fails


def exact_mismatches(got, ref, names):
    """Names among ``names`` whose tensors in ``got`` and ``ref`` are not torch.equal (after a cast of
    ``got`` to the reference's dtype; the exact arm's values are all representable in bf16)."""
    return [n for n in names if got[n].shape != ref[n].shape or not torch.equal(got[n].cpu().to(ref[n].dtype), ref[n])]


def near_tie(wz32, wz64):
    """Pooled elements left out of the generic arm's comparisons, from the two arms' pre-ReLU window
    values: the top two of the window's four post-ReLU fp64 values lie closer than the fp32 arm's largest
    error against fp64 on this tensor, so fp32 accumulation in another order may pick another winner.
    A window whose four fp64 values all lie below minus that error is no near tie: every order clamps
    all four to zero, its value is 0 and its winner is position 0 by rule. Returns (mask, error)."""
    err = float((wz32.double() - wz64).abs().max())
    top = torch.relu(wz64).sort(-1, descending=True).values
    dead = wz64.max(-1).values < -err
    return ((top[..., 0] - top[..., 1]) <= err) & ~dead, err


# ------------------------------------------------------------------------------ kernel layouts
def nhwc_pad(t, cpad, dtype):
    """[B, C, H, W] -> contiguous [B, H, W, cpad] with zero channels appended."""
    return F.pad(t.permute(0, 2, 3, 1), (0, cpad - t.shape[1])).contiguous().to(dtype)


def from_nhwc(t, c):
    """[B, H, W, cpad] -> ([B, c, H, W], the padded channels [B, H, W, cpad - c])."""
    return t[..., :c].permute(0, 3, 1, 2).contiguous(), t[..., c:]


def p2_rows(t, dtype):
    """[B, 50, 4, 4] -> [B, 800] in the order conv2 writes it: (pooled pixel, channel)."""
    return t.permute(0, 2, 3, 1).reshape(t.shape[0], 800).contiguous().to(dtype)


def from_p2_rows(t):
    return t.view(t.shape[0], 4, 4, 50).permute(0, 3, 1, 2).contiguous()


# ------------------------------------------------------------------------------ the cases both test files use
# B = 1; 3 with a repeated gather index; 17; and 65 = 64 + 1, where 64 is a common multiple of the images
# per workgroup (1 forward / dgrad, 8 and 4 in the two weight-gradient partial kernels) and of the 64-row
# stage of the linear kernels
BATCHES = (1, 3, 17, 65)
ROWS = 80          # rows of the data set the gather index addresses
LR, MOMENTUM, STEPS = 0.05, 0.9, 3


def gather_index(B, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    idx = torch.randint(0, ROWS, (B,), generator=g)
    if B == 3:
        idx[1] = idx[0]
    return idx


def generic_case(B, seed):
    """Gaussian images (bf16-representable), ``Net``'s own initialisation, labels and a gather index."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(ROWS, 1, 28, 28, generator=g).to(BF16).float()
    y = torch.randint(0, 10, (ROWS,), generator=g)
    torch.manual_seed(seed)
    return x, y, gather_index(B, seed), mnist_cnn.Net()


def exact_case(B, seed):
    """Small-integer / power-of-two operands for every kernel, so that every sum is exact in fp32 in any
    order: images and conv1 filter in {-1, 0, 1, 2} / {-1, 0, 1}, a non-negative p1 with many zeros, conv2
    filter in {-1, -0.5, 0, 0.5, 1} (zero mean: half of the conv2 outputs survive ReLU), integer biases and pooled gradients. The filters are random, hence asymmetric."""
    g = torch.Generator().manual_seed(seed)

    def ints(lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=g).float()

    c = {"x": ints(-1, 2, ROWS, 1, 28, 28), "idx": gather_index(B, seed),
         "w1": ints(-1, 1, 20, 1, 5, 5), "b1": ints(-2, 2, 20),
         "p1": torch.relu(ints(-3, 3, B, 20, 12, 12)),
         "w2": torch.tensor([-1.0, -0.5, 0.0, 0.5, 1.0])[torch.randint(0, 5, (50, 20, 5, 5), generator=g)],
         "b2": ints(-2, 2, 50), "dp2": ints(-2, 2, B, 50, 4, 4), "dp1": ints(-2, 2, B, 20, 12, 12)}
    return c
