"""Per-step time of the Keras MNIST CNN trial (workloads/mnist_tfcnn.py): the fused HIP step (``--impl
hip``, captured and replayed as the trial does) against the module path's step, eager as the trial runs
it and under ``CapturedStep``, at batch 64 and 32 (the example's range) with Adam and with SGD, on 60k
device-resident images; ``lin_fwd_splitk`` against ``lin_fwd`` on the ``fc1`` shape; and the notebook's
epoch of 70 SGD steps at batch 64.

All paths of one configuration live in one process and are timed in alternating windows (hip, module
eager, module captured, hip, ...), each window a host clock around ``--steps`` steps (one index copy + one
step each) ending in a device synchronise. Reported per path: the median window's time per step, the
spread (min .. max over windows) and the launches per step - counted, not assumed: the HIP path by
counting its kernel calls in one eager step, the module path from a torch.profiler trace of one eager
step. A path that cannot be captured is reported as such, never guessed. Per-kernel device times come from
a kernel trace of the trial itself (``rocprofv3 --kernel-trace --stats -- python -m
katib_amd.workloads.mnist_tfcnn --impl hip ...``), a run of its own.

The 70-step epoch is set beside BASELINE.md B9 (about 87 s per epoch for the notebook on one CPU worker)
for what it is: another machine class (one MI355X against one CPU pod), the synthetic task instead of the
MNIST files, and a train step only - no input pipeline, no Keras callbacks.

    python benchmarks/bench_mnist_tfcnn.py [--out profiles/mnist_tfcnn_hip.log]

One JSON line per configuration, a table at the end. Needs a GPU: there is no CPU fall-back.
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

from katib_amd.workloads import mnist_tfcnn  # noqa: E402
from katib_amd.workloads.common import CapturedStep  # noqa: E402
from katib_amd.workloads.mnist_cnn import _data  # noqa: E402

# bindings of HipTFCNN.train_step that launch two kernels (the others launch one; *_size launch none)
TWO_LAUNCHES = ("lin_fwd_splitk", "tfcnn_conv_wgrad_sgd", "tfcnn_conv_wgrad_adam")


class _Counting:
    """Counts the kernels launched through a kernels module."""

    def __init__(self, k):
        self._k, self.n = k, 0

    def __getattr__(self, name):
        fn = getattr(self._k, name)
        if name.endswith("_size"):
            return fn

        def call(*a, **kw):
            self.n += 2 if name in TWO_LAUNCHES else 1
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


def module_path(model, optimizer, lr, dev, tx, ty, idx, captured):
    """The trial's module step (mnist_tfcnn._Trainer.step), statement for statement; under capture Adam is
    ``capturable`` (its step counter on the device), which the eager trial does not need."""
    if optimizer == "adam":
        opt = torch.optim.Adam(model.parameters(), lr=lr, eps=mnist_tfcnn.ADAM_EPS, capturable=captured)
    else:
        opt = torch.optim.SGD(model.parameters(), lr=lr, momentum=0.0)
    stats = torch.zeros(2, device=dev)

    def train_step():
        yb = ty[idx]
        out = model(tx[idx])
        loss = F.cross_entropy(out, yb)
        opt.zero_grad()
        loss.backward()
        opt.step()
        with torch.no_grad():
            stats[0] += loss.detach()
            stats[1] += (out.argmax(1) == yb).sum()
        return stats

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


def bench_steps(args, dev, tx, tx16, ty, rows, text):
    for optimizer, lr in (("adam", 0.001), ("sgd", 0.1)):
        for bs in (int(v) for v in args.batch_sizes.split(",")):
            gen = torch.Generator(device=dev).manual_seed(0)
            perm = torch.randperm(args.num_train, device=dev, generator=gen)[:args.steps * bs].view(-1, bs)
            idx = torch.zeros(bs, dtype=torch.long, device=dev)
            torch.manual_seed(1)
            paths = collections.OrderedDict()
            net = mnist_tfcnn.TFNet().to(dev)
            hip = mnist_tfcnn.HipTFCNN(net, lr, 0.0, dev, optimizer)
            paths["hip"] = (CapturedStep(lambda hip=hip, idx=idx: hip.train_step(tx16, ty, idx)), None)
            paths["module_eager"] = module_path(mnist_tfcnn.TFNet().to(dev), optimizer, lr, dev, tx, ty, idx, False)
            paths["module_captured"] = module_path(mnist_tfcnn.TFNet().to(dev), optimizer, lr, dev, tx, ty, idx, True)
            row = {"optimizer": optimizer, "batch": bs, "steps_per_window": args.steps, "windows": args.windows}
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
            for name in paths:
                row[name + "_us_per_step"] = round(statistics.median(us[name]), 2)
                row[name + "_us_min_max"] = [round(min(us[name]), 2), round(max(us[name]), 2)]
            if "hip" in paths:
                real, hip.k = hip.k, _Counting(hip.k)
                try:
                    hip.train_step(tx16, ty, idx)
                    row["hip_launches_per_step"] = hip.k.n
                finally:
                    hip.k = real
            if "module_eager" in paths:
                try:
                    row["module_eager_launches_per_step"] = paths["module_eager"][1]()
                except Exception as exc:
                    row["module_eager_launches_per_step"] = "not measured (%s)" % type(exc).__name__
            if optimizer == "sgd" and bs == 64 and "hip" in paths:  # the notebook's epoch: 70 steps
                ep = [window(paths["hip"][0], idx, perm, 70) * 70 / 1e3 for _ in range(args.windows)]
                row["hip_notebook_epoch_ms"] = round(statistics.median(ep), 3)
                row["hip_notebook_epoch_ms_min_max"] = [round(min(ep), 3), round(max(ep), 3)]
            for other in ("module_eager", "module_captured"):
                if other in us and "hip" in us:
                    row[other + "_over_hip"] = round(row[other + "_us_per_step"] / row["hip_us_per_step"], 3)
                    row["hip_beats_" + other] = max(us["hip"]) < min(us[other])
            rows.append(row)
            print(json.dumps(row), flush=True)
            for name in ("hip", "module_eager", "module_captured"):
                text.append("%-4s batch %3d  %-16s %s us/step %s  launches %s" % (
                    optimizer, bs, name, row.get(name + "_us_per_step"), row.get(name + "_us_min_max", ""),
                    row.get(name + "_launches_per_step", "-")))
            for other in ("module_eager", "module_captured"):
                if other + "_over_hip" in row:
                    text.append("%-4s batch %3d  %s / hip = %.3f%s" % (
                        optimizer, bs, other, row[other + "_over_hip"],
                        "" if row["hip_beats_" + other] else "   <- the HIP step does not win outside the spread"))
            if "hip_notebook_epoch_ms" in row:
                text.append("sgd  batch  64  the notebook's epoch (70 steps), HIP step: %.3f ms %s; BASELINE B9: about "
                            "87 s per epoch on one CPU worker - another machine class, not a like-for-like figure"
                            % (row["hip_notebook_epoch_ms"], row["hip_notebook_epoch_ms_min_max"]))


def bench_fc1(args, dev, rows, text):
    """``lin_fwd_splitk`` against ``lin_fwd`` on fc1's forward, M x 128 x 21632, alternating windows."""
    from katib_amd.ops.conv import kernels

    k = kernels()
    N, K = mnist_tfcnn.HID, mnist_tfcnn.FEAT
    g = torch.Generator(device=dev).manual_seed(2)
    w = (torch.randn(N, K, device=dev, generator=g) / K ** 0.5).to(torch.bfloat16)
    b = torch.randn(N, device=dev, generator=g)
    for M in (int(v) for v in args.batch_sizes.split(",")):
        x = torch.relu(torch.randn(M, K, device=dev, generator=g)).to(torch.bfloat16)
        y0, y1 = (torch.empty(M, N, device=dev, dtype=torch.bfloat16) for _ in range(2))
        part = torch.empty(k.lin_splitk_part_size(M, N, K), device=dev, dtype=torch.float32)
        fns = collections.OrderedDict(lin_fwd=lambda: k.lin_fwd(x, None, w, b, None, y0, True),
                                      lin_fwd_splitk=lambda: k.lin_fwd_splitk(x, w, b, part, y1, True))
        graphs = {}
        for name, fn in fns.items():  # one launch sequence of 50 calls per graph: device time, no launch gaps
            fn()
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                for _ in range(50):
                    fn()
            graphs[name] = gr
        us = {name: [] for name in fns}
        for _ in range(args.windows):
            for name, gr in graphs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(20):
                    gr.replay()
                torch.cuda.synchronize()
                us[name].append((time.perf_counter() - t0) / 1000 * 1e6)
        diff = float((y0.float() - y1.float()).abs().max() / y0.float().abs().max())
        row = {"fc1_forward_M": M, "N": N, "K": K, "KS": k.LIN_SPLITK_KS, "max_rel_diff": diff}
        for name in fns:
            row[name + "_us"] = round(statistics.median(us[name]), 2)
            row[name + "_us_min_max"] = [round(min(us[name]), 2), round(max(us[name]), 2)]
        row["splitk_wins"] = max(us["lin_fwd_splitk"]) < min(us["lin_fwd"])
        rows.append(row)
        print(json.dumps(row), flush=True)
        text.append("fc1 forward M %3d  lin_fwd %s us %s  lin_fwd_splitk %s us %s  (outputs differ by %.1e of the maximum)"
                    % (M, row["lin_fwd_us"], row["lin_fwd_us_min_max"], row["lin_fwd_splitk_us"],
                       row["lin_fwd_splitk_us_min_max"], diff))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-sizes", default="64,32")
    ap.add_argument("--num-train", type=int, default=60000)
    ap.add_argument("--steps", type=int, default=400, help="steps per window")
    ap.add_argument("--windows", type=int, default=5, help="windows per path, alternating")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mnist_tfcnn needs a GPU")
    dev = torch.device("cuda", 0)
    tx, ty = _data(args.num_train, 55, dev)
    tx16 = tx.reshape(-1, 784).to(torch.bfloat16).contiguous()
    rows, text = [], []
    bench_fc1(args, dev, rows, text)
    bench_steps(args, dev, tx, tx16, ty, rows, text)
    print("\n".join(text), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("# bench_mnist_tfcnn: us per step, %d device-resident images, %d windows x %d steps alternating\n"
                    % (args.num_train, args.windows, args.steps))
            f.write("\n".join(json.dumps(r) for r in rows) + "\n" + "\n".join(text) + "\n")


if __name__ == "__main__":
    main()
