"""Keras MNIST CNN trial with TF summaries (reference
``examples/v1beta1/trial-images/tf-mnist-with-summaries/mnist.py`` and the objective of
``examples/v1beta1/sdk/tune-train-from-func.ipynb``).

Same network, ``Conv2D(32, 3, relu) -> Flatten -> Dense(128, relu) -> Dense(10)`` with Keras'
initialisation (Glorot-uniform kernels, zero biases) and softmax cross-entropy on the logits; the
trial's CLI (``--batch-size``, ``--learning-rate``, ``--epochs``, ``--log-interval``, ``--log-path``);
its output lines; and its summaries: scalars ``loss`` and ``accuracy`` at step = epoch in
``<log-path>/train`` and ``<log-path>/test``, which the TensorFlowEvent collector reads. ``--optimizer
adam`` is the trial image, ``--optimizer sgd`` with ``--steps-per-epoch 70`` the notebook, whose
objective is ``train_mnist_model``. Data: the synthetic 28x28 teacher task of ``mnist_cnn.py``.

**Running means, as the reference has them.** The reference creates its four metric objects once and
never resets them - its comment at the top of the epoch loop says it does, its code only flushes the
writers. So every value it prints or writes is a running mean since the start of the trial: the
losses are means of all per-batch mean losses so far, the accuracies the share of correct predictions
among all samples seen so far. This program keeps that behaviour (``train_mnist_model`` does not:
Keras' ``fit`` resets its metrics every epoch). The accuracy in the printed lines is multiplied by
100, as there; the summaries hold the fraction.

**No distribution strategy.** The reference program uses none, so under ``TF_CONFIG`` every worker
trains the same model on its own. So does this one; only task index 0 prints and writes summaries
(the workers of a trial share a file system here).

**Adam.** ``torch.optim.Adam`` with Keras' ``eps = 1e-7``. Keras adds ``eps`` to ``sqrt(v)`` before the
bias correction, torch after it: the two differ by a factor ``sqrt(1 - beta2^t)`` on ``eps`` and in
nothing else (ARCHITECTURE.md section 5).

``--impl hip`` (opt-in; ``module`` is the default) trains the same ``TFNet`` - same seed, initialisation,
data, permutation, batches and output - on hand-written kernels: ``csrc/hip/mnist_tfcnn.hip`` for the
convolution forward and its weight gradient, the split-K ``lin_fwd_splitk`` for ``fc1`` and the fused
linear / cross-entropy kernels of ``csrc/hip/mlp.hip`` for the rest. One train step is 11 launches
(``HipTFCNN.train_step``), captured once as a HIP graph and replayed (``--capture 0``: eager). It is
one process on one GPU and exits with a message when there is none. The numeric contract is in
ARCHITECTURE.md section 2.
"""

from __future__ import annotations

import argparse
import json
import os
import tempfile

import torch
import torch.nn as nn
import torch.nn.functional as F

from .common import CapturedStep
from .mnist_cnn import _data

PIX, C1, FEAT, HID, F2P = 26 * 26, 32, 26 * 26 * 32, 128, 16  # F2P: fc2 rows, 10 padded to 16
PARAMS = ("conv.weight", "conv.bias", "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")
ADAM_BETAS, ADAM_EPS = (0.9, 0.999), 1e-7  # Keras' defaults


class TFNet(nn.Module):
    """The reference's ``MyModel``. The conv output goes to NHWC before the flatten, so ``fc1.weight``'s
    columns are in Keras' order: (pixel, channel)."""

    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(1, C1, 3)
        self.fc1 = nn.Linear(FEAT, HID)
        self.fc2 = nn.Linear(HID, 10)
        for m in (self.conv, self.fc1, self.fc2):  # Keras: glorot_uniform kernels, zero biases
            nn.init.xavier_uniform_(m.weight)
            nn.init.zeros_(m.bias)

    def forward(self, x):
        z = F.relu(self.conv(x)).permute(0, 2, 3, 1).flatten(1)
        return self.fc2(F.relu(self.fc1(z)))


def pack_state(sd, dev="cpu"):
    """The kernels' fp32 masters from tensors in the module's layout (``sd``: name -> tensor for the six
    ``PARAMS``): conv [32][9] (channel, tap), fc1 [128][21632] as it is, fc2 [16][128] and its bias [16]
    with zero rows 10..15. Works for optimizer state too."""
    f = {n: sd[n].detach().to(dev, torch.float32) for n in PARAMS}
    return {"conv.weight": f["conv.weight"].reshape(C1, 9).contiguous(), "conv.bias": f["conv.bias"].clone(),
            "fc1.weight": f["fc1.weight"].contiguous().clone(), "fc1.bias": f["fc1.bias"].clone(),
            "fc2.weight": F.pad(f["fc2.weight"], (0, 0, 0, F2P - 10)).contiguous(),
            "fc2.bias": F.pad(f["fc2.bias"], (0, F2P - 10))}


def unpack_state(k):
    """Inverse of ``pack_state``: the module's names, shapes and layout (pads dropped)."""
    return {"conv.weight": k["conv.weight"].reshape(C1, 1, 3, 3).clone(), "conv.bias": k["conv.bias"].clone(),
            "fc1.weight": k["fc1.weight"].clone(), "fc1.bias": k["fc1.bias"].clone(),
            "fc2.weight": k["fc2.weight"][:10].clone(), "fc2.bias": k["fc2.bias"][:10].clone()}


def conv_shadow(w):
    """bf16 shadow of the packed conv master: [9][32] (tap, channel)."""
    return w.t().contiguous().to(torch.bfloat16)


class HipTFCNN:
    """``TFNet`` on the fused HIP kernels, trained with ``optimizer`` = sgd (momentum, ``torch.optim.SGD``
    defaults) or adam (``torch.optim.Adam``, betas 0.9 / 0.999, eps 1e-7). ``ref`` supplies the initial
    weights. ``p`` holds the fp32 masters in the kernels' layout (``pack_state``), ``s0`` the momentum
    buffers or Adam's ``exp_avg``, ``s1`` Adam's ``exp_avg_sq``; ``ws`` / ``fc[i]["w16"|"w16t"]`` are the
    bf16 shadows the kernels read. ``step_t`` is Adam's device step counter: 0 before the first step,
    advanced by every ``train_step`` (eager or replayed) inside its cross-entropy launch.
    ``state_dict()`` gives all of it back in the module's layout, ``load_optim_state()`` takes it."""

    def __init__(self, ref: TFNet, lr: float, momentum: float, dev, optimizer: str = "adam"):
        assert optimizer in ("adam", "sgd")
        self.k = None
        if torch.device(dev).type == "cuda":  # the state and its layouts need no GPU, the steps do
            from ..ops.conv import kernels

            self.k = kernels()
        self.optimizer, self.momentum = optimizer, momentum
        self.lr = torch.full((1,), lr, device=dev, dtype=torch.float32)
        self.step_t = torch.zeros(1, device=dev, dtype=torch.int32)
        self.p = pack_state(ref.state_dict(), dev)
        self.s0 = {n: torch.zeros_like(t) for n, t in self.p.items()}
        self.s1 = {n: torch.zeros_like(t) for n, t in self.p.items()} if optimizer == "adam" else None
        self.ws = conv_shadow(self.p["conv.weight"])
        self.fc = []
        for name in ("fc1", "fc2"):
            w = self.p[name + ".weight"]
            self.fc.append({"w": name + ".weight", "b": name + ".bias", "w16": w.to(torch.bfloat16),
                            "w16t": w.t().contiguous().to(torch.bfloat16)})
        self.stats = torch.zeros(2, device=dev, dtype=torch.float32)

    def forward(self, x, idx=None, save=False):
        """Logits [B][16] bf16 (columns 0..9 are real) of the rows ``idx`` of ``x`` [rows][784] bf16, or
        of every row. ``save``: also return what the backward needs."""
        k, dev = self.k, x.device
        B = idx.numel() if idx is not None else x.shape[0]
        f1, f2 = self.fc
        z = torch.empty((B, FEAT), device=dev, dtype=torch.bfloat16)
        k.tfcnn_conv_fwd(x, idx, self.ws, self.p["conv.bias"], z)
        h = torch.empty((B, HID), device=dev, dtype=torch.bfloat16)
        part = torch.empty(k.lin_splitk_part_size(B, HID, FEAT), device=dev, dtype=torch.float32)
        k.lin_fwd_splitk(z, f1["w16"], self.p["fc1.bias"], part, h, True)
        logits = torch.empty((B, F2P), device=dev, dtype=torch.bfloat16)
        k.lin_fwd(h, None, f2["w16"], self.p["fc2.bias"], None, logits, False)
        return (z, h, logits) if save else logits

    def _lin_update(self, dy, x, l):
        k, p, s0, s1 = self.k, self.p, self.s0, self.s1
        w, b = l["w"], l["b"]
        if self.optimizer == "adam":
            k.lin_wgrad_adam(dy, x, None, p[w], s0[w], s1[w], l["w16"], l["w16t"], p[b], s0[b], s1[b], self.lr,
                             self.step_t, ADAM_BETAS[0], ADAM_BETAS[1], ADAM_EPS)
        else:
            k.lin_wgrad_sgd(dy, x, None, p[w], s0[w], l["w16"], l["w16t"], p[b], s0[b], self.lr, self.momentum)

    def train_step(self, x, y, idx):
        """One optimizer step on the rows ``idx`` of ``x`` / ``y``; 11 launches. Every dgrad runs before
        the update of the layer it reads. Returns ``stats`` (+= mean loss, correct count)."""
        k, p, s0, s1 = self.k, self.p, self.s0, self.s1
        adam = self.optimizer == "adam"
        B = idx.numel() if idx is not None else x.shape[0]
        z, h, logits = self.forward(x, idx, save=True)
        dl = torch.empty_like(logits)
        k.xent_small(logits, y, idx, dl, 10, self.stats, self.step_t if adam else None)
        f1, f2 = self.fc
        dh = torch.empty_like(h)
        k.lin_fwd(dl, None, f2["w16t"], None, h, dh, False)
        self._lin_update(dl, h, f2)
        dz = torch.empty_like(z)
        k.lin_fwd(dh, None, f1["w16t"], None, z, dz, False)  # masked by z > 0: the conv's ReLU derivative
        self._lin_update(dh, z, f1)
        part = torch.empty(k.tfcnn_part_size(B), device=x.device, dtype=torch.float32)
        if adam:
            k.tfcnn_conv_wgrad_adam(dz, x, idx, part, p["conv.weight"], s0["conv.weight"], s1["conv.weight"],
                                    p["conv.bias"], s0["conv.bias"], s1["conv.bias"], self.ws, self.lr, self.step_t,
                                    ADAM_BETAS[0], ADAM_BETAS[1], ADAM_EPS)
        else:
            k.tfcnn_conv_wgrad_sgd(dz, x, idx, part, p["conv.weight"], s0["conv.weight"], p["conv.bias"],
                                   s0["conv.bias"], self.ws, self.lr, self.momentum)
        return self.stats

    def state_dict(self):
        """fp32 tensors in the module's names, shapes and layout: the six parameters and the optimizer
        state, as ``momentum_buffer.<name>`` (sgd) or ``exp_avg.<name>`` / ``exp_avg_sq.<name>`` plus
        ``step`` (adam; an int64 scalar)."""
        out = unpack_state(self.p)
        if self.optimizer == "adam":
            out.update({"exp_avg." + n: t for n, t in unpack_state(self.s0).items()})
            out.update({"exp_avg_sq." + n: t for n, t in unpack_state(self.s1).items()})
            out["step"] = self.step_t[0].to(torch.int64)
        else:
            out.update({"momentum_buffer." + n: t for n, t in unpack_state(self.s0).items()})
        return out

    def load_optim_state(self, sd):
        """Inverse of ``state_dict()`` for the optimizer state (the names it uses; parameters in ``sd`` are
        ignored): the next step starts from it."""
        names = ("exp_avg.", "exp_avg_sq.") if self.optimizer == "adam" else ("momentum_buffer.",)
        for prefix, dst in zip(names, (self.s0, self.s1)):
            for n, t in pack_state({n: sd[prefix + n] for n in PARAMS}, self.lr.device).items():
                dst[n].copy_(t)
        if self.optimizer == "adam":
            self.step_t.fill_(int(sd["step"]))


def parse_args(argv):
    p = argparse.ArgumentParser(description="Keras MNIST CNN trial with summaries (katib-amd)")
    p.add_argument("--batch-size", type=int, default=64)
    p.add_argument("--learning-rate", type=float, default=0.001)
    p.add_argument("--epochs", type=int, default=10)
    p.add_argument("--log-interval", type=int, default=100)
    p.add_argument("--log-path", type=str,
                   default=os.path.join(os.getenv("TEST_TMPDIR", tempfile.gettempdir()),
                                        "tensorflow/mnist/logs/mnist_with_summaries"))
    p.add_argument("--optimizer", default="adam", choices=["adam", "sgd"],
                   help="adam: the trial image; sgd: the notebook's objective")
    p.add_argument("--momentum", type=float, default=0.0)
    p.add_argument("--steps-per-epoch", type=int, default=0, help="0: the whole shard; the notebook uses 70")
    p.add_argument("--num-train", type=int, default=60000)
    p.add_argument("--num-test", type=int, default=10000)
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--impl", default="module", choices=["module", "hip"],
                   help="module: nn.Module + torch.optim (default, runs on the CPU too); hip: the fused HIP "
                        "kernels (one GPU, one process)")
    p.add_argument("--capture", type=int, default=1, choices=[0, 1],
                   help="--impl hip only: replay the train step as a captured HIP graph (1) or run it eagerly (0)")
    return p.parse_args(argv)


def _task_index():
    try:
        return int(json.loads(os.environ.get("TF_CONFIG") or "{}").get("task", {}).get("index", 0))
    except (ValueError, AttributeError, TypeError):
        return 0


class _Trainer:
    """Model, optimizer and data of one trial; ``step(idx)`` trains on one batch and adds the batch's mean
    loss and its number of correct predictions to ``stats`` (device fp32 [2]), ``logits(rows)`` evaluates."""

    def __init__(self, args, dev):
        torch.manual_seed(args.seed)
        x, y = _data(args.num_train + args.num_test, 55, dev)
        self.tx, self.ty = x[:args.num_train], y[:args.num_train]
        self.vx, self.vy = x[args.num_train:], y[args.num_train:]
        self.model = TFNet().to(dev)
        self.hip = None
        bs = args.batch_size
        if args.impl == "hip":
            self.hip = HipTFCNN(self.model, args.learning_rate, args.momentum, dev, args.optimizer)
            self.txb = self.tx.reshape(-1, 784).to(torch.bfloat16).contiguous()
            self.vxb = self.vx.reshape(-1, 784).to(torch.bfloat16).contiguous()
            self.idx = torch.zeros(bs, dtype=torch.long, device=dev)
            self.stats = self.hip.stats
            self.hip_step = CapturedStep(lambda: self.hip.train_step(self.txb, self.ty, self.idx),
                                         enabled=bool(args.capture))
        else:
            params = self.model.parameters()
            self.opt = (torch.optim.Adam(params, lr=args.learning_rate, eps=ADAM_EPS) if args.optimizer == "adam"
                        else torch.optim.SGD(params, lr=args.learning_rate, momentum=args.momentum))
            self.stats = torch.zeros(2, device=dev, dtype=torch.float32)

    def step(self, idx):
        if self.hip is not None:
            self.idx.copy_(idx)
            self.hip_step()
            return
        yb = self.ty[idx]
        out = self.model(self.tx[idx])
        loss = F.cross_entropy(out, yb)
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()
        with torch.no_grad():
            self.stats[0] += loss.detach()
            self.stats[1] += (out.argmax(1) == yb).sum()

    @torch.no_grad()
    def test_logits(self, chunk=1000):
        n = self.vy.numel()
        if self.hip is not None:
            return torch.cat([self.hip.forward(self.vxb[i:i + chunk])[:, :10].float() for i in range(0, n, chunk)])
        self.model.eval()
        out = torch.cat([self.model(self.vx[i:i + chunk]) for i in range(0, n, chunk)])
        self.model.train()
        return out


def _check_hip(args):
    if args.impl == "hip" and not torch.cuda.is_available():
        raise SystemExit("--impl hip needs a GPU: its train step is HIP kernels only (use --impl module)")


def main(argv=None):
    args = parse_args(argv if argv is not None else [])
    _check_hip(args)
    dev = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
    chief = _task_index() == 0
    t = _Trainer(args, dev)
    writers = None
    if chief:
        from ..metricscollector.tfevent import EventWriter

        writers = {k: EventWriter(os.path.join(args.log_path, k)) for k in ("train", "test")}
    bs, n_train = args.batch_size, args.num_train
    nb = n_train // bs
    if args.steps_per_epoch > 0:
        nb = min(nb, args.steps_per_epoch)
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    # the reference never resets its metrics: sums since the start of the trial
    steps = seen = 0
    test_loss_sum, test_batches, test_correct, test_seen = 0.0, 0, 0, 0
    test_acc = 0.0
    for epoch in range(args.epochs):
        perm = torch.randperm(n_train, device=dev, generator=gen)
        for b in range(nb):
            t.step(perm[b * bs:(b + 1) * bs])
            steps += 1
            seen += bs
            if b % args.log_interval == 0 and chief:
                loss_sum, correct = t.stats.tolist()
                print("Train Epoch: {} [{}/{} ({:.0f}%)]\tloss={:.4f}, accuracy={:.4f}".format(
                    epoch + 1, b * bs, n_train, 100. * b * bs / n_train, loss_sum / steps, correct / seen * 100),
                    flush=True)
        loss_sum, correct = t.stats.tolist()
        train_loss, train_acc = loss_sum / max(steps, 1), correct / max(seen, 1)
        out = t.test_logits()
        per = F.cross_entropy(out, t.vy, reduction="none")
        batch_means = torch.stack([c.mean() for c in per.split(bs)])  # the reference tests in batches of --batch-size
        test_loss_sum += float(batch_means.sum())
        test_batches += batch_means.numel()
        test_correct += int((out.argmax(1) == t.vy).sum())
        test_seen += t.vy.numel()
        test_loss, test_acc = test_loss_sum / test_batches, test_correct / test_seen
        if chief:
            writers["train"].add_scalar("loss", train_loss, epoch)
            writers["train"].add_scalar("accuracy", train_acc, epoch)
            writers["test"].add_scalar("loss", test_loss, epoch)
            writers["test"].add_scalar("accuracy", test_acc, epoch)
            print("Test Loss: {:.4f}, Test Accuracy: {:.4f}\n".format(test_loss, test_acc * 100), flush=True)
    if writers is not None:
        for w in writers.values():
            w.close()
    return test_acc


def fit_notebook(lr, num_epoch, num_train=60000, seed=1, impl=None):
    """The notebook's ``model.fit``: plain SGD, batch 64, 70 steps per epoch, one line per epoch with that
    epoch's mean accuracy and loss (Keras resets its metrics every epoch). On the HIP step when a GPU is
    present, on the module otherwise. Returns the last epoch's (accuracy, loss)."""
    impl = impl or ("hip" if torch.cuda.is_available() else "module")
    args = parse_args(["--optimizer", "sgd", "--learning-rate", str(lr), "--batch-size", "64", "--num-train",
                       str(num_train), "--num-test", "0", "--seed", str(seed), "--impl", impl])
    _check_hip(args)
    dev = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
    t = _Trainer(args, dev)
    gen = torch.Generator(device=dev).manual_seed(seed)
    bs, spe = 64, 70
    perm, at = None, 0
    acc = loss = 0.0
    for epoch in range(num_epoch):
        t.stats.zero_()
        for _ in range(spe):  # shuffle(60000).repeat().batch(64): a new permutation when one runs out
            if perm is None or at + bs > perm.numel():
                perm, at = torch.randperm(num_train, device=dev, generator=gen), 0
            t.step(perm[at:at + bs])
            at += bs
        loss_sum, correct = t.stats.tolist()
        acc, loss = correct / (spe * bs), loss_sum / spe
        print("Epoch {}/{}. accuracy={:.4f} - loss={:.4f}".format(epoch + 1, num_epoch, acc, loss), flush=True)
    return acc, loss


def train_mnist_model(parameters):
    """The notebook's objective for ``KatibClient.tune()``: reads ``lr`` and ``num_epoch`` from the dict.
    Self-contained (``tune`` ships this function's source to the trial)."""
    from katib_amd.workloads.mnist_tfcnn import fit_notebook

    fit_notebook(float(parameters["lr"]), int(parameters["num_epoch"]),
                 num_train=int(parameters.get("num_train", 60000)))


if __name__ == "__main__":
    import sys

    main(sys.argv[1:])
