"""Reference for one ``HipMLP`` train step (katib_amd/workloads/mnist_mlp.py on the kernels of
csrc/hip/mlp.hip), in torch ops on the CPU.

``train_step`` walks the step the way ``HipMLP.train_step`` does - forward, cross-entropy and its
gradient, then from the top layer down the dgrad through the pre-update weight and that layer's
weight / bias gradient and optimizer update - with two knobs:

``gemm_dtype``  fp32 or fp64: the type every matrix product, the softmax and the sums run in.
``round``       ``torch.bfloat16`` or ``None``: applied where the kernels round - the input rows, each
                layer's activations, the logits, ``dl``, each ``dh`` and the weight shadows.

Masters and optimizer state stay fp32 (fp64 when ``gemm_dtype`` is fp64 and ``round`` is None). The
updates are not re-derived: they are ``torch.optim.SGD``, ``torch.optim.Adam`` and the trial's ``Ftrl``,
stepped on parameters whose ``grad`` and optimizer state are preset from the layer dicts.

A plain helper module of the tests (tests/test_mlp_step_oracle.py validates it against autograd
without a GPU, tests/test_gpu_mlp_optim.py compares ``HipMLP`` with it).
"""
import torch

from katib_amd.workloads import mnist_mlp

F32, F64 = torch.float32, torch.float64
# layer-dict names of (weight state 0, weight state 1, bias state 0, bias state 1), as HipMLP's
STATE = {"sgd": ("wm", None, "bm", None), "adam": ("m", "v", "bm", "bv"), "ftrl": ("z", "n", "bz", "bn")}
ADAM_BETAS, ADAM_EPS = (0.9, 0.999), 1e-8


def state_dtype(gemm_dtype, round):
    return F64 if gemm_dtype == F64 and round is None else F32


def layers_from_module(model, optimizer, dtype=F32, pad_out=None):
    """Layer dicts (``w``, ``b`` and zero optimizer state, all ``dtype``) from an ``MLP`` or a
    ``DeepMLP``; ``pad_out`` zero-pads the output layer to that many rows as ``HipMLP`` does."""
    fcs = [model.fc1, model.fc2, model.fc3] if isinstance(model, mnist_mlp.MLP) else list(model.hidden) + [model.out]
    layers = []
    for i, fc in enumerate(fcs):
        w, b = fc.weight.detach().to("cpu", dtype).clone(), fc.bias.detach().to("cpu", dtype).clone()
        if pad_out is not None and i == len(fcs) - 1:
            w = torch.cat([w, w.new_zeros(pad_out - w.shape[0], w.shape[1])])
            b = torch.cat([b, b.new_zeros(pad_out - b.shape[0])])
        layer = {"w": w, "b": b}
        for name, like in zip(STATE[optimizer], (w, w, b, b)):
            if name is not None:
                layer[name] = torch.zeros_like(like)
        layers.append(layer)
    return layers


def optimizer_step(optimizer, pairs, lr, momentum, t):
    """One step of the real optimizer on ``pairs`` = [(value, grad, state 0, state 1 or None)];
    returns [(new value, new state 0, new state 1 or None)]."""
    params = [torch.nn.Parameter(v.clone()) for v, _, _, _ in pairs]
    if optimizer == "sgd":
        opt = torch.optim.SGD(params, lr=lr, momentum=momentum)
    elif optimizer == "adam":
        opt = torch.optim.Adam(params, lr=lr, betas=ADAM_BETAS, eps=ADAM_EPS)
    else:
        opt = mnist_mlp.Ftrl(params, lr=lr)
    for p, (_, g, s0, s1) in zip(params, pairs):
        p.grad = g.to(p.dtype).clone()
        if optimizer == "sgd":
            opt.state[p]["momentum_buffer"] = s0.clone()
        elif optimizer == "adam":
            opt.state[p].update(step=torch.tensor(float(t - 1)), exp_avg=s0.clone(), exp_avg_sq=s1.clone())
        else:
            opt.state[p].update(z=s0.clone(), n=s1.clone())
    opt.step()
    out = []
    for p in params:
        st = opt.state[p]
        if optimizer == "sgd":
            out.append((p.detach(), st["momentum_buffer"], None))
        elif optimizer == "adam":
            out.append((p.detach(), st["exp_avg"], st["exp_avg_sq"]))
        else:
            out.append((p.detach(), st["z"], st["n"]))
    return out


def train_step(layers, x, y, optimizer, lr, momentum=0.0, t=1, gemm_dtype=F32, round=None, classes=10):
    """One train step on ``layers`` (updated in place; ``w16`` / ``w16t`` are set to the rounded
    shadows of the new masters). ``x`` [M][784]: the minibatch rows, already gathered; ``y`` [M];
    ``t``: the 1-based number of this step (Adam's bias corrections). Returns the logits and the
    mean loss."""
    gd, sd = gemm_dtype, state_dtype(gemm_dtype, round)

    def r(v):
        return v.to(round).to(gd) if round is not None else v.to(gd)

    M = x.shape[0]
    acts, h = [], r(x)
    x0 = h
    for i, l in enumerate(layers):
        pre = h @ r(l["w"]).t() + l["b"].to(gd)
        h = r(torch.relu(pre) if i < len(layers) - 1 else pre)
        acts.append(h)
    logits = acts[-1]
    lsm = torch.log_softmax(logits[:, :classes], 1)
    loss = -lsm[torch.arange(M), y].mean()
    d = lsm.exp()
    d[torch.arange(M), y] -= 1.0
    dy = torch.zeros_like(logits)
    dy[:, :classes] = d / M
    dy = r(dy)
    names = STATE[optimizer]
    for i in range(len(layers) - 1, -1, -1):
        l = layers[i]
        inp = acts[i - 1] if i > 0 else x0
        gw, gb = dy.t() @ inp, dy.sum(0)
        if i > 0:  # dgrad through the pre-update weight, masked by the ReLU derivative
            dh = r((dy @ r(l["w"])) * (inp > 0))
        (w, w0, w1), (b, b0, b1) = optimizer_step(
            optimizer,
            [(l["w"].to(sd), gw.to(sd), l[names[0]].to(sd), None if names[1] is None else l[names[1]].to(sd)),
             (l["b"].to(sd), gb.to(sd), l[names[2]].to(sd), None if names[3] is None else l[names[3]].to(sd))],
            lr, momentum, t)
        l["w"], l["b"], l[names[0]], l[names[2]] = w, b, w0, b0
        if names[1] is not None:
            l[names[1]], l[names[3]] = w1, b1
        l["w16"] = w.to(round) if round is not None else w.clone()
        l["w16t"] = l["w16"].t().contiguous()
        if i > 0:
            dy = dh
    return logits, float(loss)
