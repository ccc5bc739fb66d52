"""Per-step time of the MNIST CNN trial (workloads/mnist_cnn.py): the fused HIP step (``--impl hip``,
captured and replayed as the trial does) against the module path's step, eager as the trial runs it
and under ``CapturedStep``, at batch 64 and 16 on 60k device-resident images.

The three paths live in one process and are timed in alternating windows (hip, module eager, module
captured, hip, ...), each window a host clock around ``--steps`` steps (one index copy + one step each)
ending in a device synchronise. Reported per path: the median window's time per step, the spread
(min .. max over windows) and the launches per step - counted, not assumed: the HIP path by counting
its kernel calls in one eager step, the module path from a torch.profiler trace of one eager step. A
path that cannot be captured is reported as such, never guessed. Per-kernel device times come from a
kernel trace of the trial itself (``rocprofv3 --kernel-trace --stats -- python -m
katib_amd.workloads.mnist_cnn --impl hip ...``), a run of its own.

    python benchmarks/bench_mnist_cnn.py [--out profiles/mnist_cnn_hip.log]

One JSON line per batch size, a table at the end. Needs a GPU: there is no CPU fall-back.
"""
import argparse
import collections
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from katib_amd.workloads import mnist_cnn  # noqa: E402
from katib_amd.workloads.common import CapturedStep  # noqa: E402


class _Counting:
    """Counts the kernel-launching calls made through a kernels module."""

    def __init__(self, k):
        self._k, self.n = k, 0

    def __getattr__(self, name):
        fn = getattr(self._k, name)
        if name == "cnn_part_sizes":
            return fn

        def call(*a, **kw):
            self.n += 1
            return fn(*a, **kw)
        return call


def _kernel_events(fn, steps):
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
    return [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
            and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]


def hip_path(model, lr, dev, tx16, ty, idx):
    net = mnist_cnn.HipCNN(model, lr, 0.9, dev)
    step = CapturedStep(lambda: net.train_step(tx16, ty, idx))

    def launches():
        real, net.k = net.k, _Counting(net.k)
        try:
            net.train_step(tx16, ty, idx)
            # conv2_wgrad_sgd and conv1_wgrad_sgd are two launches each (partials, then sum + SGD)
            return net.k.n + 2
        finally:
            net.k = real
    return step, launches


def module_path(model, lr, dev, tx, ty, idx, captured):
    """The trial's module step (mnist_cnn.main, one process), statement for statement."""
    opt = torch.optim.SGD(model.parameters(), lr=lr, momentum=0.9)

    def train_step():
        loss = F.nll_loss(model(tx[idx]), ty[idx])
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss

    step = CapturedStep(train_step, enabled=captured)
    return step, lambda: len(_kernel_events(train_step, 1))


def window(step, idx, perm, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(steps):
        idx.copy_(perm[s % perm.shape[0]])
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-sizes", default="64,16")
    ap.add_argument("--num-train", type=int, default=60000)
    ap.add_argument("--steps", type=int, default=900, help="steps per window (about an epoch at batch 64)")
    ap.add_argument("--windows", type=int, default=5, help="windows per path, alternating")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mnist_cnn needs a GPU")
    dev = torch.device("cuda", 0)
    tx, ty = mnist_cnn._data(args.num_train, 55, dev)
    tx16 = tx.reshape(-1, 784).to(torch.bfloat16).contiguous()
    rows, text = [], []
    for bs in (int(v) for v in args.batch_sizes.split(",")):
        gen = torch.Generator(device=dev).manual_seed(0)
        perm = torch.randperm(args.num_train, device=dev, generator=gen)[:args.steps * bs].view(-1, bs)
        idx = torch.zeros(bs, dtype=torch.long, device=dev)
        torch.manual_seed(1)
        paths = collections.OrderedDict()
        paths["hip"] = hip_path(mnist_cnn.Net().to(dev), 0.01, dev, tx16, ty, idx)
        paths["module_eager"] = module_path(mnist_cnn.Net().to(dev), 0.01, dev, tx, ty, idx, False)
        paths["module_captured"] = module_path(mnist_cnn.Net().to(dev), 0.01, dev, tx, ty, idx, True)
        row = {"batch": bs, "steps_per_window": args.steps, "windows": args.windows}
        for name in list(paths):  # warm-up steps, capture, first replays
            try:
                window(paths[name][0], idx, perm, 20)
            except Exception as exc:
                row[name + "_us_per_step"] = "not measured (%s: %s)" % (type(exc).__name__, str(exc)[:120])
                del paths[name]
        us = {name: [] for name in paths}
        for _ in range(args.windows):
            for name, (step, _) in paths.items():
                us[name].append(window(step, idx, perm, args.steps))
        for name, (_, launches) in paths.items():
            row[name + "_us_per_step"] = round(statistics.median(us[name]), 2)
            row[name + "_us_min_max"] = [round(min(us[name]), 2), round(max(us[name]), 2)]
            if name != "module_captured":
                try:
                    row[name + "_launches_per_step"] = launches()
                except Exception as exc:
                    row[name + "_launches_per_step"] = "not measured (%s)" % type(exc).__name__
        for other in ("module_eager", "module_captured"):
            if other in us and "hip" in us:
                row[other + "_over_hip"] = round(row[other + "_us_per_step"] / row["hip_us_per_step"], 3)
                row["hip_beats_" + other] = max(us["hip"]) < min(us[other])
        rows.append(row)
        print(json.dumps(row), flush=True)
        for name in ("hip", "module_eager", "module_captured"):
            v = row.get(name + "_us_per_step")
            text.append("batch %3d  %-16s %s us/step %s  launches %s" % (
                bs, name, v, row.get(name + "_us_min_max", ""), row.get(name + "_launches_per_step", "-")))
        for other in ("module_eager", "module_captured"):
            if other + "_over_hip" in row:
                text.append("batch %3d  %s / hip = %.3f%s" % (bs, other, row[other + "_over_hip"], "" if row[
                    "hip_beats_" + other] else "   <- the HIP step does not win outside the spread"))
    print("\n".join(text), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("# bench_mnist_cnn: us per step, %d device-resident images, %d windows x %d steps alternating\n"
                    % (args.num_train, args.windows, args.steps))
            f.write("\n".join(json.dumps(r) for r in rows) + "\n" + "\n".join(text) + "\n")


if __name__ == "__main__":
    main()
