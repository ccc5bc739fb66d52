"""Reference for one ``HipTFCNN`` train step (katib_amd/workloads/mnist_tfcnn.py on the kernels of
csrc/hip/mnist_tfcnn.hip and csrc/hip/mlp.hip), in torch ops on the CPU, in the module's layout throughout.

``train_step`` walks the step the way ``HipTFCNN.train_step`` does - forward, cross-entropy and its
gradient, then from the top layer down the dgrad through the pre-update weight and that layer's weight /
bias gradient and optimizer update - with two knobs:

``gemm_dtype``  fp32 or fp64: the type every convolution, matrix product, softmax and sum runs in.
``round``       ``torch.bfloat16`` or ``None``: applied where the kernels round - the images, the weight
                shadows, ``z``, ``h``, the logits, ``dl``, ``dh``, ``dz``.

Bias and ReLU act on the unrounded accumulators; the ReLU derivative is the mask ``> 0`` on the stored
activation. Masters and optimizer state stay fp32 (fp64 when ``gemm_dtype`` is fp64 and ``round`` is None).
The optimizer is not re-derived: it is ``torch.optim.SGD`` / ``torch.optim.Adam`` (eps 1e-7, as the
workload passes it) stepped on parameters whose ``grad`` and state are preset.

Activations of the convolution come in two shapes: ``[B, 32, 26, 26]`` (torch) and rows ``[B, 21632]`` in
Keras' Flatten order (pixel, channel), which is what the kernels store and ``fc1`` reads; ``z_rows`` /
``from_z_rows`` convert. The per-kernel pieces (``conv_fwd``, ``conv_wgrad``, ``lin``) are what the GPU
file compares each kernel with; ``held`` / ``state_failures`` / ``exact_mismatches`` are the checkers it
uses, and ``MUTANTS`` are wrong steps those checkers must reject (tests/test_mnist_tfcnn_oracle.py).
"""
import torch
import torch.nn.functional as F

from katib_amd.workloads import mnist_tfcnn

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
PARAMS = mnist_tfcnn.PARAMS
ADAM_BETAS, ADAM_EPS = mnist_tfcnn.ADAM_BETAS, mnist_tfcnn.ADAM_EPS
MUTANTS = ("nchw_flatten", "post_update_dgrad", "relu_mask_ge", "adam_no_bias_correction", "no_db")
STATE = {"sgd": ("momentum_buffer",), "adam": ("exp_avg", "exp_avg_sq")}


def state_dtype(gemm_dtype, round):
    return F64 if gemm_dtype == F64 and round is None else F32


def _r(v, gd, round):
    return v.to(round).to(gd) if round is not None else v.to(gd)


def params_from_module(model, dtype=F32):
    return {n: t.detach().to("cpu", dtype).clone() for n, t in model.state_dict().items()}


def zero_state(p, optimizer):
    """Optimizer state as ``{"t": steps done, <state name>: {param name: tensor}}``."""
    st = {"t": 0}
    for s in STATE[optimizer]:
        st[s] = {n: torch.zeros_like(t) for n, t in p.items()}
    return st


def drawn_state(p, optimizer, seed, t=100):
    """A carried, well-conditioned state, as tests/test_gpu_mlp_optim.py draws it: first moments / momentum
    0.01 N(0, 1), second moments U(0.1, 1.1) (sqrt(v) >= 0.3, far above eps), ``t`` steps done."""
    g = torch.Generator().manual_seed(seed)
    st = {"t": t if optimizer == "adam" else 0}
    for s in STATE[optimizer]:
        st[s] = {n: ((torch.rand(v.shape, generator=g) + 0.1) if s == "exp_avg_sq"
                     else 0.01 * torch.randn(v.shape, generator=g)).to(v.dtype) for n, v in p.items()}
    return st


# ------------------------------------------------------------------------------ layouts
def z_rows(t):
    """[B, 32, 26, 26] -> [B, 21632] in Keras' Flatten order (pixel, channel)."""
    return t.permute(0, 2, 3, 1).reshape(t.shape[0], -1).contiguous()


def from_z_rows(t):
    return t.view(t.shape[0], 26, 26, 32).permute(0, 3, 1, 2).contiguous()


# ------------------------------------------------------------------------------ per-kernel pieces
def conv_fwd(x, w, b, gemm_dtype=F32, round=None):
    """relu(conv3x3_valid(x, w) + b), rounded: [B, 32, 26, 26]."""
    gd = gemm_dtype
    return _r(torch.relu(F.conv2d(_r(x, gd, round), _r(w, gd, round)) + b.to(gd)[None, :, None, None]), gd, round)


def conv_wgrad(dz, x, gemm_dtype=F32, round=None):
    """(dW [32, 1, 3, 3], db [32]) from dz [B, 32, 26, 26] (already ReLU-masked) and the images."""
    gd = gemm_dtype
    d = _r(dz, gd, round).flatten(2)
    patches = F.unfold(_r(x, gd, round), 3)  # [B, 9, 676]
    return torch.einsum("bcl,bkl->ck", d, patches).view(32, 1, 3, 3), d.sum((0, 2))


def lin(x, w, b=None, relu=False, gemm_dtype=F32, round=None):
    """act(x w^T + b), rounded."""
    gd = gemm_dtype
    y = _r(x, gd, round) @ _r(w, gd, round).t()
    if b is not None:
        y = y + b.to(gd)
    return _r(torch.relu(y) if relu else y, gd, round)


def optimizer_step(optimizer, pairs, lr, momentum=0.0, t=1):
    """One step of the real optimizer on ``pairs`` = [(value, grad, state 0, state 1 or None)]; ``t`` is the
    1-based number of this step. Returns [(new value, new state 0, new state 1 or None)]."""
    params = [torch.nn.Parameter(v.clone()) for v, _, _, _ in pairs]
    if optimizer == "sgd":
        opt = torch.optim.SGD(params, lr=lr, momentum=momentum)
    else:
        opt = torch.optim.Adam(params, lr=lr, betas=ADAM_BETAS, eps=ADAM_EPS)
    for p, (_, g, s0, s1) in zip(params, pairs):
        p.grad = g.to(p.dtype).clone()
        if optimizer == "sgd":
            opt.state[p]["momentum_buffer"] = s0.clone()
        else:
            opt.state[p].update(step=torch.tensor(float(t - 1)), exp_avg=s0.clone(), exp_avg_sq=s1.clone())
    opt.step()
    if optimizer == "sgd":
        return [(p.detach(), opt.state[p]["momentum_buffer"], None) for p in params]
    return [(p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]) for p in params]


def _adam_no_bias_correction(pairs, lr):
    """A wrong Adam (mutant): the moments as they are, no division by 1 - beta^t."""
    out = []
    for v, g, m, s in pairs:
        m = ADAM_BETAS[0] * m + (1 - ADAM_BETAS[0]) * g
        s = ADAM_BETAS[1] * s + (1 - ADAM_BETAS[1]) * g * g
        out.append((v - lr * m / (s.sqrt() + ADAM_EPS), m, s))
    return out


# ------------------------------------------------------------------------------ the step
def train_step(p, st, x, y, lr, optimizer="adam", momentum=0.0, gemm_dtype=F32, round=None, mutant=None):
    """One train step on ``p`` / ``st`` (``zero_state``'s form; both updated in place). ``x`` [B, 1, 28, 28]:
    the minibatch, already gathered; ``y`` [B]. Returns the intermediates (``z``, ``dz`` as rows) and the
    pre-optimizer gradients (``g.<name>``), in the module's layout."""
    assert mutant is None or mutant in MUTANTS
    gd, sd = gemm_dtype, state_dtype(gemm_dtype, round)
    B = x.shape[0]
    names = STATE[optimizer]
    st["t"] += 1

    def r(v):
        return _r(v, gd, round)

    def mask(a):
        return a >= 0 if mutant == "relu_mask_ge" else a > 0

    def update(layer, gw, gb):
        if mutant == "no_db":
            gb = torch.zeros_like(gb)
        pairs = [(p[n].to(sd), g.to(sd), st[names[0]][n].to(sd), st[names[1]][n].to(sd) if len(names) > 1 else None)
                 for n, g in ((layer + ".weight", gw), (layer + ".bias", gb))]
        if mutant == "adam_no_bias_correction" and optimizer == "adam":
            new = _adam_no_bias_correction(pairs, lr)
        else:
            new = optimizer_step(optimizer, pairs, lr, momentum, st["t"])
        for n, (v, s0, s1) in zip((layer + ".weight", layer + ".bias"), new):
            p[n], st[names[0]][n] = v, s0
            if len(names) > 1:
                st[names[1]][n] = s1

    def dgrad_then_update(layer, dy, act_in, gw, gb):
        """dy w masked by the layer's input activation, through the weight from before the update."""
        if mutant == "post_update_dgrad":
            update(layer, gw, gb)
        d = r((dy @ r(p[layer + ".weight"])) * mask(act_in))
        if mutant != "post_update_dgrad":
            update(layer, gw, gb)
        return d

    out = {}
    x0 = r(x)
    zc = conv_fwd(x0, p["conv.weight"], p["conv.bias"], gd, round)
    z = zc.flatten(1) if mutant == "nchw_flatten" else z_rows(zc)
    h = lin(z, p["fc1.weight"], p["fc1.bias"], True, gd, round)
    logits = lin(h, p["fc2.weight"], p["fc2.bias"], False, gd, round)
    lsm = torch.log_softmax(logits, 1)
    loss = -lsm[torch.arange(B), y].mean()
    d = lsm.exp()
    d[torch.arange(B), y] -= 1.0
    dl = r(d / B)
    out.update(z=z, h=h, logits=logits, dl=dl, loss=float(loss))

    gw, gb = dl.t() @ h, dl.sum(0)
    out["g.fc2.weight"], out["g.fc2.bias"] = gw, gb
    dh = dgrad_then_update("fc2", dl, h, gw, gb)
    gw, gb = dh.t() @ z, dh.sum(0)
    out["g.fc1.weight"], out["g.fc1.bias"] = gw, gb
    dz = dgrad_then_update("fc1", dh, z, gw, gb)
    dzc = dz.view_as(zc) if mutant == "nchw_flatten" else from_z_rows(dz)
    gw, gb = conv_wgrad(dzc, x0, gd, round)
    out["g.conv.weight"], out["g.conv.bias"] = gw, gb
    update("conv", gw, gb)
    out.update(dh=dh, dz=dz)
    return out


def state_dict(p, st, optimizer):
    """The oracle's state under ``HipTFCNN.state_dict()``'s names."""
    out = {n: p[n].clone() for n in PARAMS}
    for s in STATE[optimizer]:
        out.update({s + "." + n: st[s][n].clone() for n in PARAMS})
    if optimizer == "adam":
        out["step"] = torch.tensor(st["t"], dtype=torch.int64)
    return out


# ------------------------------------------------------------------------------ checkers
def rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-6))


def held(name, got, r32, r64, floor=1e-2, out=print):
    """``got`` against the fp32-GEMM oracle, held to the larger of ``floor`` (relative, max norm) and four
    times that oracle's own distance from the fp64-GEMM one. Prints the figure; returns [] or [(name, figure,
    bar)]."""
    if tuple(got.shape) != tuple(r32.shape):
        return [(name, "shape", tuple(got.shape))]
    bar, fig = max(floor, 4 * rel(r32, r64)), rel(got, r32)
    out("  %-34s %.2e/%.2e" % (name, fig, bar))
    return [] if fig < bar else [(name, fig, bar)]


def state_failures(got, ref32, ref64, before, optimizer, label="", out=print):
    """Optimizer state and updates (new - before) of ``got`` against the fp32-GEMM oracle under ``held``'s rule.
    All four are ``state_dict()``s. Prints every figure; returns the list of (name, figure, bar) that miss."""
    fails = []
    for n in PARAMS:
        for s in STATE[optimizer]:
            fails += held(label + " " + s + "." + n, got[s + "." + n], ref32[s + "." + n], ref64[s + "." + n], out=out)
        b = before[n].double()
        if got[n].shape != b.shape:
            fails.append((n, "shape", tuple(got[n].shape)))
            continue
        fails += held(label + " " + n + " upd", got[n].cpu().double() - b, ref32[n].double() - b,
                      ref64[n].double() - b, out=out)
    if optimizer == "adam" and int(got["step"]) != int(ref32["step"]):
        fails.append(("step", int(got["step"]), int(ref32["step"])))
    return fails


def exact_mismatches(got, ref, names):
    """Names among ``names`` whose tensors in ``got`` and ``ref`` are not torch.equal (after a cast of ``got``
    to the reference's dtype)."""
    return [n for n in names if got[n].shape != ref[n].shape or not torch.equal(got[n].cpu().to(ref[n].dtype), ref[n])]


# ------------------------------------------------------------------------------ the cases both test files use
# B = 1; 3 with a repeated gather index; 17, a tail inside one 64-row tile; 65 = 64 + 1, a second M tile of
# one row
BATCHES = (1, 3, 17, 65)
ROWS = 80          # rows of the data set the gather index addresses
LR, MOMENTUM, STEPS = 0.05, 0.9, 3
ADAM_LR = 1e-3
EXACT_LR = 2.0 ** -10


def gather_index(B, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    idx = torch.randint(0, ROWS, (B,), generator=g)
    if B == 3:
        idx[1] = idx[0]
    return idx


def generic_case(B, seed):
    """Gaussian images (bf16-representable), ``TFNet``'s own initialisation, labels and a gather index."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(ROWS, 1, 28, 28, generator=g).to(BF16).float()
    y = torch.randint(0, 10, (ROWS,), generator=g)
    torch.manual_seed(seed)
    return x, y, gather_index(B, seed), mnist_tfcnn.TFNet()


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _halves(g, *shape):
    return torch.tensor([-1.0, -0.5, 0.0, 0.5, 1.0])[torch.randint(0, 5, shape, generator=g)]


def exact_case(B, seed):
    """Small-integer / power-of-two operands for every kernel, so that every sum is exact in fp32 in any
    order: images in {-1..2} and the conv filter in {-1, 0, 1} with an integer bias (|z| <= 20, an integer
    bf16 holds); a drawn fc1 input ``zin`` in {0..3} with many zeros against fc1 weights in {-1, -0.5, 0, 0.5,
    1} (a 21,632-term row sum is a multiple of 0.5 below 2^16: 18 bits) and an integer bias; ``dh`` in
    {-2..2} for the fc1 dgrad (128 terms); ``dz`` in {-2..2} for the conv weight gradient (B x 676 terms
    of magnitude <= 4: below 2^18). The results round to bf16 only after an exact sum, so they are equal bit
    for bit whatever the order."""
    g = torch.Generator().manual_seed(seed)
    return {"x": _ints(g, -1, 2, ROWS, 1, 28, 28), "idx": gather_index(B, seed),
            "w": _ints(g, -1, 1, 32, 1, 3, 3), "b": _ints(g, -2, 2, 32),
            "zin": torch.relu(_ints(g, -3, 3, B, mnist_tfcnn.FEAT)),
            "w1": _halves(g, mnist_tfcnn.HID, mnist_tfcnn.FEAT), "b1": _ints(g, -2, 2, mnist_tfcnn.HID),
            "dh": _ints(g, -2, 2, B, mnist_tfcnn.HID), "dz": _ints(g, -2, 2, B, 32, 26, 26)}


def lin_case(M, N, K, seed, exact):
    """(x [M][K], w [N][K], bias [N]) for ``lin_fwd_splitk``: Gaussian (bf16-representable), or the exact
    arm's integers and halves."""
    g = torch.Generator().manual_seed(seed)
    if exact:
        return torch.relu(_ints(g, -3, 3, M, K)), _halves(g, N, K), _ints(g, -2, 2, N)
    return (torch.randn(M, K, generator=g).to(BF16).float(), (torch.randn(N, K, generator=g) / K ** 0.5).to(BF16).float(),
            torch.randn(N, generator=g))
