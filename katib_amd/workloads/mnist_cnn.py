"""PyTorch (Fashion)MNIST CNN trial with optional data parallelism (reference
``examples/v1beta1/trial-images/pytorch-mnist/mnist.py:32-205``).

Same network (Conv 1->20 5x5, pool, Conv 20->50 5x5, pool, FC 800->500, FC 500->10,
log-softmax / NLL, SGD with momentum), same CLI (``--lr``, ``--momentum``,
``--batch-size``, ``--epochs``, ``--log-interval``, ``--backend``, ``--log-path``,
``--logger {standard,hypertune}``), same metric lines (``{metricName}={value}``
or hypertune JSON into ``--log-path``). As a ``PyTorchJob`` trial every replica is a
rank (``WORLD_SIZE``/``RANK``/``MASTER_ADDR`` set by the scheduler) and gradients are
averaged with one flat all-reduce per step over ``--backend`` (``nccl`` = RCCL over
xGMI on MI355X, or ``gloo``); only rank 0 prints metrics (the primary replica).
``--tb-dir`` additionally writes TensorBoard event files for the TFEvent collector.
Data: a synthetic 28x28 teacher task resident on the device.

``--impl hip`` (opt-in; ``module`` is the default and is the program described above, unchanged)
trains the same ``Net`` - same seed, same initialisation, same data, permutation, batches and
output lines - on hand-written kernels: ``csrc/hip/mnist_cnn.hip`` for convolution + bias + ReLU +
max-pool forward, the conv2 data gradient and the two convolution weight gradients, and the
fused linear / cross-entropy kernels of ``csrc/hip/mlp.hip`` for ``fc1`` / ``fc2``. One train step is 14
launches (``HipCNN.train_step``), captured once as a HIP graph and replayed (``--capture 0``: eager).
SGD with momentum is fused into the weight-gradient kernels, so a step never holds a gradient that
could be all-reduced: ``--impl hip`` is single-process and exits with a message when ``WORLD_SIZE > 1``
(the PyTorchJob example stays on the module path) or when there is no GPU. The numeric contract is in
ARCHITECTURE.md section 2.
"""

from __future__ import annotations

import argparse
import json
import os
import time

_T_MODULE = time.time()  # cold-trial phases: the module starts importing (interpreter + katib_amd up)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from ..parallel.comm import Comm  # noqa: E402
from .common import CapturedStep, phase, process_start_time  # noqa: E402

_T_TORCH = time.time()
_PHASES = os.environ.get("KATIB_AMD_TRIAL_PHASES") == "1"


def _mark(name, dev):
    """A cold-trial phase mark (common.phase) once the device has caught up. Off - no
    synchronisation, no line - unless KATIB_AMD_TRIAL_PHASES=1."""
    if _PHASES:
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        phase(name)


class Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(1, 20, 5, 1)
        self.conv2 = nn.Conv2d(20, 50, 5, 1)
        self.fc1 = nn.Linear(4 * 4 * 50, 500)
        self.fc2 = nn.Linear(500, 10)

    def forward(self, x):
        x = F.max_pool2d(F.relu(self.conv1(x)), 2, 2)
        x = F.max_pool2d(F.relu(self.conv2(x)), 2, 2)
        x = F.relu(self.fc1(x.view(-1, 4 * 4 * 50)))
        return F.log_softmax(self.fc2(x), dim=1)


C1P, COP, F1P, F2P = 24, 64, 504, 16  # padded: conv1 channels, conv2 shadow rows, fc1 rows, fc2 rows
PARAMS = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "fc1.weight", "fc1.bias", "fc2.weight",
          "fc2.bias")


def pack_state(sd, dev="cpu"):
    """The kernels' fp32 masters from tensors in the module's layout (``sd``: name -> tensor for the
    eight ``PARAMS``): conv1 [24][25] (channel, tap); conv2 [50][600] (co, r, s, ci padded to 24);
    fc1 [504][800] with its columns in the order conv2 writes ``p2``, (pooled pixel, channel) instead of
    torch's (channel, pooled pixel); fc2 [16][504]. Every pad is zero. Works for momentum buffers too."""
    f = {n: sd[n].detach().to(dev, torch.float32) for n in PARAMS}
    w1 = F.pad(f["conv1.weight"].reshape(20, 25), (0, 0, 0, C1P - 20))
    w2 = F.pad(f["conv2.weight"].permute(0, 2, 3, 1), (0, C1P - 20)).reshape(50, 25 * C1P)
    fw1 = F.pad(f["fc1.weight"].view(500, 50, 16).permute(0, 2, 1).reshape(500, 800), (0, 0, 0, F1P - 500))
    fw2 = F.pad(f["fc2.weight"], (0, F1P - 500, 0, F2P - 10))
    return {"conv1.weight": w1.contiguous(), "conv1.bias": F.pad(f["conv1.bias"], (0, C1P - 20)),
            "conv2.weight": w2.contiguous(), "conv2.bias": f["conv2.bias"].clone(),
            "fc1.weight": fw1.contiguous(), "fc1.bias": F.pad(f["fc1.bias"], (0, F1P - 500)),
            "fc2.weight": fw2.contiguous(), "fc2.bias": F.pad(f["fc2.bias"], (0, F2P - 10))}


def unpack_state(k):
    """Inverse of ``pack_state``: the module's names, shapes and layout (pads dropped)."""
    return {"conv1.weight": k["conv1.weight"][:20].reshape(20, 1, 5, 5).clone(),
            "conv1.bias": k["conv1.bias"][:20].clone(),
            "conv2.weight": k["conv2.weight"].view(50, 5, 5, C1P)[..., :20].permute(0, 3, 1, 2).contiguous(),
            "conv2.bias": k["conv2.bias"].clone(),
            "fc1.weight": k["fc1.weight"][:500].view(500, 16, 50).permute(0, 2, 1).reshape(500, 800).contiguous(),
            "fc1.bias": k["fc1.bias"][:500].clone(),
            "fc2.weight": k["fc2.weight"][:10, :500].clone(), "fc2.bias": k["fc2.bias"][:10].clone()}


def conv_shadows(w1, w2):
    """bf16 shadows of the packed conv masters: conv1 [25][24] (tap, channel); conv2 forward [64][608]
    (co, k = (r, s, ci)) and dgrad [24][25][64] (ci, tap, co), zero where padded."""
    w1s = w1.t().contiguous().to(torch.bfloat16)
    w2f = torch.zeros(COP, 608, device=w2.device, dtype=torch.bfloat16)
    w2f[:50, :600] = w2.to(torch.bfloat16)
    w2d = torch.zeros(C1P, 25, COP, device=w2.device, dtype=torch.bfloat16)
    w2d[:, :, :50] = w2.to(torch.bfloat16).view(50, 25, C1P).permute(2, 1, 0)
    return w1s, w2f, w2d


class HipCNN:
    """``Net`` on the fused HIP kernels, trained with SGD + momentum (``torch.optim.SGD`` defaults).
    ``ref`` supplies the initial weights. ``p`` holds the fp32 masters in the kernels' layout
    (``pack_state``), ``m`` their momentum buffers, ``w1s`` / ``w2f`` / ``w2d`` / ``fc[i]["w16"|"w16t"]`` the
    bf16 shadows the kernels read; ``state_dict()`` gives all of it back in the module's layout."""

    def __init__(self, ref: Net, lr: float, momentum: float, dev):
        from ..ops.conv import kernels

        self.k = kernels()
        self.momentum = momentum
        self.lr = torch.full((1,), lr, device=dev, dtype=torch.float32)
        self.p = pack_state(ref.state_dict(), dev)
        self.m = {n: torch.zeros_like(t) for n, t in self.p.items()}
        self.w1s, self.w2f, self.w2d = conv_shadows(self.p["conv1.weight"], self.p["conv2.weight"])
        self.fc = []
        for name in ("fc1", "fc2"):
            w = self.p[name + ".weight"]
            self.fc.append({"w": w, "wm": self.m[name + ".weight"], "b": self.p[name + ".bias"],
                            "bm": self.m[name + ".bias"], "w16": w.to(torch.bfloat16),
                            "w16t": w.t().contiguous().to(torch.bfloat16)})
        self.stats = torch.zeros(2, device=dev, dtype=torch.float32)

    def forward(self, x, idx=None, save=False):
        """Logits [B][16] bf16 (columns 0..9 are real) of the rows ``idx`` of ``x`` [rows][784] bf16, or
        of every row. ``save``: also keep what the backward needs (and write the pooling winners)."""
        k, dev = self.k, x.device
        B = idx.numel() if idx is not None else x.shape[0]
        p1 = torch.empty((B, 12, 12, C1P), device=dev, dtype=torch.bfloat16)
        p2 = torch.empty((B, 800), device=dev, dtype=torch.bfloat16)
        a1 = torch.empty((B, 12, 12, C1P), device=dev, dtype=torch.uint8) if save else None
        a2 = torch.empty((B, 800), device=dev, dtype=torch.uint8) if save else None
        k.cnn_conv1_pool_fwd(x, idx, self.w1s, self.p["conv1.bias"], p1, a1)
        k.cnn_conv2_pool_fwd(p1, self.w2f, self.p["conv2.bias"], p2, a2)
        h = torch.empty((B, F1P), device=dev, dtype=torch.bfloat16)
        k.lin_fwd(p2, None, self.fc[0]["w16"], self.fc[0]["b"], None, h, True)
        logits = torch.empty((B, F2P), device=dev, dtype=torch.bfloat16)
        k.lin_fwd(h, None, self.fc[1]["w16"], self.fc[1]["b"], None, logits, False)
        return (p1, a1, p2, a2, h, logits) if save else logits

    def train_step(self, x, y, idx):
        """One SGD step on the rows ``idx`` of ``x`` / ``y``; 14 launches. Every dgrad runs before the
        update of the layer it reads. Returns ``stats`` (+= mean loss, correct count)."""
        k, mom = self.k, self.momentum
        B = idx.numel() if idx is not None else x.shape[0]
        p1, a1, p2, a2, h, logits = self.forward(x, idx, save=True)
        dl = torch.empty_like(logits)
        k.xent_small(logits, y, idx, dl, 10, self.stats, None)
        f1, f2 = self.fc
        dh = torch.empty_like(h)
        k.lin_fwd(dl, None, f2["w16t"], None, h, dh, False)
        k.lin_wgrad_sgd(dl, h, None, f2["w"], f2["wm"], f2["w16"], f2["w16t"], f2["b"], f2["bm"], self.lr, mom)
        dp2 = torch.empty_like(p2)
        k.lin_fwd(dh, None, f1["w16t"], None, p2, dp2, False)  # masked by p2 > 0: conv2's ReLU derivative
        k.lin_wgrad_sgd(dh, p2, None, f1["w"], f1["wm"], f1["w16"], f1["w16t"], f1["b"], f1["bm"], self.lr, mom)
        dp1 = torch.empty_like(p1)
        k.cnn_conv2_dgrad(dp2, a2, self.w2d, p1, dp1)
        n1, n2 = k.cnn_part_sizes(B)
        part2 = torch.empty(n2, device=x.device, dtype=torch.float32)
        k.cnn_conv2_wgrad_sgd(dp2, a2, p1, part2, self.p["conv2.weight"], self.m["conv2.weight"],
                              self.p["conv2.bias"], self.m["conv2.bias"], self.w2f, self.w2d, self.lr, mom)
        part1 = torch.empty(n1, device=x.device, dtype=torch.float32)
        k.cnn_conv1_wgrad_sgd(dp1, a1, x, idx, part1, self.p["conv1.weight"], self.m["conv1.weight"],
                              self.p["conv1.bias"], self.m["conv1.bias"], self.w1s, self.lr, mom)
        return self.stats

    def state_dict(self):
        """fp32 tensors in the module's names, shapes and layout: the eight parameters, and their
        momentum buffers as ``momentum_buffer.<name>``."""
        out = unpack_state(self.p)
        out.update({"momentum_buffer." + n: t for n, t in unpack_state(self.m).items()})
        return out


def parse_args(argv):
    p = argparse.ArgumentParser(description="PyTorch MNIST trial (katib-amd)")
    p.add_argument("--batch-size", type=int, default=64)
    p.add_argument("--test-batch-size", type=int, default=1000)
    p.add_argument("--epochs", type=int, default=1)
    p.add_argument("--lr", type=float, default=0.01)
    p.add_argument("--momentum", type=float, default=0.5)
    p.add_argument("--no-cuda", action="store_true", default=False)
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--log-interval", type=int, default=10)
    p.add_argument("--log-path", type=str, default="")
    p.add_argument("--logger", type=str, choices=["standard", "hypertune"], default="standard")
    p.add_argument("--backend", type=str, default="nccl" if torch.cuda.is_available() else "gloo")
    p.add_argument("--num-train", type=int, default=60000)
    p.add_argument("--num-test", type=int, default=10000)
    p.add_argument("--tb-dir", type=str, default="")
    p.add_argument("--impl", default="module", choices=["module", "hip"],
                   help="module: nn.Module + torch.optim.SGD (default); hip: the fused HIP kernels (one GPU, "
                        "one process)")
    p.add_argument("--capture", type=int, default=1, choices=[0, 1],
                   help="--impl hip only: replay the train step as a captured HIP graph (1) or run it eagerly (0)")
    return p.parse_args(argv)


def _data(n, seed, dev):
    g = torch.Generator().manual_seed(seed)
    protos = torch.randn(10, 1, 7, 7, generator=g)
    y = torch.randint(0, 10, (n,), generator=g)
    x = F.interpolate(protos[y], size=(28, 28), mode="bilinear", align_corners=False) + \
        0.8 * torch.randn(n, 1, 28, 28, generator=g)
    return x.to(dev), y.to(dev)


def main(argv=None):
    args = parse_args(argv if argv is not None else [])
    if args.impl == "hip":
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise SystemExit("--impl hip is single-process: SGD is fused into the weight-gradient kernels, so "
                             "there is no gradient to all-reduce (WORLD_SIZE > 1 needs --impl module)")
        if args.no_cuda or not torch.cuda.is_available():
            raise SystemExit("--impl hip needs a GPU: its train step is HIP kernels only (use --impl module)")
    # DDP (mnist.py:130-133,164-166,189-192): one rank per GPU, rank r on device LOCAL_RANK %
    # device_count; ranks sharing a GPU fall back to gloo + the one-shot IPC all-reduce (Comm)
    comm = Comm.from_env("cpu" if args.no_cuda or not torch.cuda.is_available() else "cuda",
                         backend=args.backend if args.backend != "mpi" else None)
    ws, rank, dev = comm.world_size, comm.rank, comm.device
    if _PHASES:
        phase("process", process_start_time())
        phase("module", _T_MODULE)
        phase("torch", _T_TORCH)
        if dev.type == "cuda":
            torch.cuda.init()
        _mark("hip_init", dev)
    torch.manual_seed(args.seed)
    dist = comm if comm.distributed else None
    if dist is not None and dev.type == "cuda":
        comm.enable_xgmi()
    x, y = _data(args.num_train + args.num_test, 55, dev)
    tx, ty, vx, vy = x[:args.num_train], y[:args.num_train], x[args.num_train:], y[args.num_train:]
    _mark("data", dev)
    model = Net().to(dev)
    params = list(model.parameters())
    if dist is not None:
        flat = torch.nn.utils.parameters_to_vector(params).detach()
        comm.broadcast_(flat, 0)
        torch.nn.utils.vector_to_parameters(flat, params)
    opt = torch.optim.SGD(params, lr=args.lr, momentum=args.momentum)
    writer = None
    if args.tb_dir and rank == 0:
        from ..metricscollector.tfevent import EventWriter

        writer = EventWriter(os.path.join(args.tb_dir, "test"))
    log_file = None
    if args.log_path and args.logger == "standard" and rank == 0:
        os.makedirs(os.path.dirname(os.path.abspath(args.log_path)), exist_ok=True)
        log_file = open(args.log_path, "a")

    def log(msg):  # logging.info to --log-path when set, else stdout (mnist.py:150-156)
        if rank != 0:
            return
        if log_file is not None:
            log_file.write(msg + "\n")
            log_file.flush()
        else:
            print(msg, flush=True)

    hip_net = hip_step = None
    if args.impl == "hip":
        hip_net = HipCNN(model, args.lr, args.momentum, dev)
        txb = tx.reshape(-1, 784).to(torch.bfloat16).contiguous()
        vxb = vx.reshape(-1, 784).to(torch.bfloat16).contiguous()
        hip_idx = torch.zeros(args.batch_size, dtype=torch.long, device=dev)
        hip_step = CapturedStep(lambda: hip_net.train_step(txb, ty, hip_idx), enabled=bool(args.capture))
    _mark("model", dev)
    shard = args.num_train // ws
    gen = torch.Generator(device=dev).manual_seed(args.seed + rank)
    step = 0
    for epoch in range(1, args.epochs + 1):
        model.train()
        perm = torch.randperm(shard, device=dev, generator=gen) + rank * shard
        nb = shard // args.batch_size
        for b in range(nb):
            idx = perm[b * args.batch_size:(b + 1) * args.batch_size]
            if hip_net is not None:
                hip_idx.copy_(idx)
                if b % args.log_interval == 0:  # stats accumulates the mean losses: read this step's alone
                    hip_net.stats.zero_()
                hip_step()
                loss = hip_net.stats[0] if b % args.log_interval == 0 else None
            else:
                loss = F.nll_loss(model(tx[idx]), ty[idx])
                opt.zero_grad()
                loss.backward()
                if dist is not None:
                    g = torch.cat([p.grad.reshape(-1) for p in params])
                    comm.allreduce_mean_(g)
                    torch.nn.utils.vector_to_parameters(g, [p.grad for p in params])
                opt.step()
            step += 1
            if step == (hip_step.warmup + 1 if hip_step is not None and hip_step.enabled else 1):
                _mark("captured", dev)  # warm-up steps + graph capture + first replay (module path: first step)
            if b % args.log_interval == 0:
                log("Train Epoch: {} [{}/{} ({:.0f}%)]\tloss={:.4f}".format(
                    epoch, b * args.batch_size * ws, args.num_train, 100.0 * b / max(nb, 1), float(loss)))
        model.eval()
        with torch.no_grad():
            if hip_net is not None:
                out = torch.cat([hip_net.forward(vxb[i:i + args.test_batch_size])[:, :10].float()
                                 for i in range(0, args.num_test, args.test_batch_size)]).log_softmax(1)
            else:
                out = torch.cat([model(vx[i:i + args.test_batch_size]) for i in range(0, args.num_test,
                                                                                        args.test_batch_size)])
            test_loss = float(F.nll_loss(out, vy, reduction="sum")) / args.num_test
            acc = float((out.argmax(1) == vy).float().mean())
        if rank == 0:
            if args.logger == "hypertune" and args.log_path:
                os.makedirs(os.path.dirname(os.path.abspath(args.log_path)), exist_ok=True)
                with open(args.log_path, "a") as f:
                    f.write(json.dumps({"metric": "accuracy", "accuracy": str(acc), "timestamp": time.time()}) +
                            "\n")
                    f.write(json.dumps({"metric": "loss", "loss": str(test_loss), "timestamp": time.time()}) + "\n")
            else:
                log("{{metricName: accuracy, metricValue: {:.4f}}};{{metricName: loss, metricValue: {:.4f}}}"
                    .format(acc, test_loss))
            if writer is not None:
                writer.add_scalar("accuracy", acc, epoch)
                writer.add_scalar("loss", test_loss, epoch)
        if epoch == 1:
            _mark("first_metric", dev)
    _mark("trained", dev)
    if writer is not None:
        writer.close()
    if log_file is not None:
        log_file.close()
    if dist is not None:
        comm.barrier()
        comm.destroy()
    return acc


if __name__ == "__main__":
    import sys

    main(sys.argv[1:])
