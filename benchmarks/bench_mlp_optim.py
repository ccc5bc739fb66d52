"""Per-step time of the B1 search space (depth x optimizer) on the fused HIP MLP kernels against the
``nn.Module`` path, at the B1 shape: batch 64, hidden 256, 60k device-resident rows, bf16, both as
captured HIP graphs replayed the way the trial replays them (one index copy + one replay per step).

For each optimizer in {sgd, adam, ftrl} and L in {2, 3, 5} both paths live in one process and are
timed in alternating windows (hip, module, hip, module, ...), each window a host clock around
``--steps`` steps ending in a device synchronise. Reported per path: the median window's time per
step, the spread (min .. max over windows) and the launches per step - counted, not assumed: the HIP
path by counting its kernel calls in one eager step, the module path from a torch.profiler trace of
one eager step (``--count-launches 0`` skips the trace).

    python benchmarks/bench_mlp_optim.py [--out profiles/mlp_optim.log]

One JSON line per configuration, a table at the end. Needs a GPU: there is no CPU fall-back.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from katib_amd.workloads import mnist_mlp  # noqa: E402
from katib_amd.workloads.common import CapturedStep, teacher_vectors  # noqa: E402


class _Counting:
    """Counts the kernel-launching calls made through a kernels module."""

    def __init__(self, k):
        self._k, self.n = k, 0

    def __getattr__(self, name):
        fn = getattr(self._k, name)

        def call(*a, **kw):
            self.n += 1
            return fn(*a, **kw)
        return call


def hip_path(model, optimizer, lr, dev, tx16, ty, idx):
    net = mnist_mlp.HipMLP(model, lr, 0.9, dev, optimizer)
    step = CapturedStep(lambda: net.train_step(tx16, ty, idx))

    def launches():
        real, net.k = net.k, _Counting(net.k)
        try:
            net.train_step(tx16, ty, idx)
            return net.k.n
        finally:
            net.k = real
    return step, launches


def module_path(model, optimizer, lr, dev, tx, ty, idx):
    """The trial's module step (mnist_mlp.main with --unroll 1), statement for statement."""
    if optimizer == "adam":
        opt = torch.optim.Adam(model.parameters(), lr=lr, capturable=True)
    elif optimizer == "ftrl":
        opt = mnist_mlp.Ftrl(model.parameters(), lr=lr)
    else:
        opt = torch.optim.SGD(model.parameters(), lr=lr, momentum=0.9)
    loss_buf = torch.zeros((), device=dev)
    correct_buf = torch.zeros((), device=dev)

    def train_step():
        xb, yb = tx.index_select(0, idx), ty.index_select(0, idx)
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
            logits = model(xb)
            loss = F.cross_entropy(logits, yb)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        loss_buf.add_(loss.detach())
        correct_buf.add_((logits.detach().argmax(1) == yb).sum())
        return loss_buf

    for p_ in model.parameters():
        p_.grad = torch.zeros_like(p_)
    if optimizer == "adam":
        opt.step()
        with torch.no_grad():
            for st in opt.state.values():
                for v in st.values():
                    if torch.is_tensor(v):
                        v.zero_()
    step = CapturedStep(train_step)

    def launches():
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            train_step()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                   and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
    return step, launches


def window(step, idx, perm, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(steps):
        idx.copy_(perm[s])
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--num-train", type=int, default=60000)
    ap.add_argument("--layers", default="2,3,5")
    ap.add_argument("--optimizers", default="sgd,adam,ftrl")
    ap.add_argument("--steps", type=int, default=900, help="steps per window (about an epoch at batch 64)")
    ap.add_argument("--windows", type=int, default=5, help="windows per path, alternating")
    ap.add_argument("--count-launches", type=int, default=1)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mlp_optim needs a GPU")
    dev = torch.device("cuda", 0)
    tx, ty = teacher_vectors(args.num_train, seed=1234, dev=dev)
    tx16 = tx.to(torch.bfloat16).contiguous()
    bs = args.batch_size
    gen = torch.Generator(device=dev).manual_seed(0)
    perm = torch.randperm(args.num_train, device=dev, generator=gen)[:args.steps * bs].view(args.steps, bs)
    idx = torch.zeros(bs, dtype=torch.long, device=dev)
    rows = []
    for optimizer in args.optimizers.split(","):
        lr = 0.001 if optimizer == "adam" else 0.02
        for L in (int(v) for v in args.layers.split(",")):
            torch.manual_seed(0)
            paths = {"hip": hip_path(mnist_mlp.DeepMLP(args.hidden, L).to(dev), optimizer, lr, dev, tx16, ty, idx),
                     "module": module_path(mnist_mlp.DeepMLP(args.hidden, L).to(dev), optimizer, lr, dev, tx, ty, idx)}
            for name, (step, _) in paths.items():  # warm-up steps, capture, first replays
                window(step, idx, perm, 20)
            us = {name: [] for name in paths}
            for _ in range(args.windows):
                for name, (step, _) in paths.items():
                    us[name].append(window(step, idx, perm, args.steps))
            row = {"optimizer": optimizer, "num_layers": L, "batch": bs, "hidden": args.hidden,
                   "steps_per_window": args.steps, "windows": args.windows}
            for name in paths:
                row[name + "_us_per_step"] = round(statistics.median(us[name]), 2)
                row[name + "_us_min_max"] = [round(min(us[name]), 2), round(max(us[name]), 2)]
            row["module_over_hip"] = round(row["module_us_per_step"] / row["hip_us_per_step"], 3)
            row["hip_wins"] = max(us["hip"]) < min(us["module"])
            rows.append((row, paths))
            print(json.dumps(row), flush=True)
    if args.count_launches:
        for row, paths in rows:
            for name, (_, launches) in paths.items():
                try:
                    row[name + "_launches_per_step"] = launches()
                except Exception as exc:  # a trace that cannot be taken is reported, never guessed
                    row[name + "_launches_per_step"] = "not measured (%s)" % type(exc).__name__
    lines = ["%-5s %2s  %10s %19s %4s  %10s %19s %4s  %s" % ("opt", "L", "hip us", "[min, max]", "ln", "module us",
                                                             "[min, max]", "ln", "module/hip")]
    for row, _ in rows:
        lines.append("%-5s %2d  %10.2f %19s %4s  %10.2f %19s %4s  %.3f%s" % (
            row["optimizer"], row["num_layers"], row["hip_us_per_step"], row["hip_us_min_max"],
            row.get("hip_launches_per_step", "-"), row["module_us_per_step"], row["module_us_min_max"],
            row.get("module_launches_per_step", "-"), row["module_over_hip"],
            "" if row["hip_wins"] else "   <- the HIP step does not win outside the spread"))
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("# bench_mlp_optim: us per captured step, batch %d hidden %d rows %d bf16, %d windows x %d steps "
                    "alternating; ln = launches per step\n" % (bs, args.hidden, args.num_train, args.windows,
                                                               args.steps))
            f.write("\n".join(json.dumps(r) for r, _ in rows) + "\n" + text + "\n")


if __name__ == "__main__":
    main()
