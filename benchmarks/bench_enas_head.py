"""Cost of the ENAS child's head (csrc/hip/enas_head.hip: pooling, dropout, dense, softmax
cross-entropy and the accuracy sums in two launches forward and one backward) on one GPU, everything
that is compared measured interleaved in one process.

Per call (default): forward + backward of the fused head against the composition the trial runs with
``--head module`` - ``global_avg_pool``, ``F.dropout``, the autocast linear, fp32 cross-entropy, the
accuracy ops and their autograd mirror - at batch 128 for the last-layer shapes of SHAPES. Each is
captured as a graph of ``--launches`` back-to-back calls; the graphs are replayed round-robin and
timed with device events. ``--segs 1,2,4,...`` adds the fused head with the backward's data role cut
into that many pixel segments per sample (the A/B behind ``kSegBytes``); ``rule`` is the default.

``--step``: the captured three-layer child step, ``--head hip`` against ``--head module``, in
alternating windows of ``--window`` steps. Prints one JSON line per measurement."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (H, W, C) of the last layer; 32x32x67 takes the element path, 32x32x528 is a 1 MB sample per workgroup
SHAPES = [(32, 32, 64), (16, 16, 64), (8, 8, 128), (32, 32, 67), (32, 32, 528)]
K = 10

# enas-gpu.yaml ops: a convolution, a separable convolution with stride 2, a convolution; skips 1->3
EMB = {"0": {"opt_type": "convolution", "filter_size": "3", "num_filter": "64", "stride": "1"},
       "1": {"opt_type": "separable_convolution", "filter_size": "3", "num_filter": "64", "stride": "2",
             "depth_multiplier": "1"},
       "2": {"opt_type": "convolution", "filter_size": "3", "num_filter": "64", "stride": "1"}}
NN_CONFIG = {"num_layers": 3, "input_sizes": [32, 32, 3], "output_sizes": [10], "embedding": EMB}
ARCH = [[0], [1, 0], [2, 0, 1]]


def _stats(v):
    s = sorted(v)
    return {"median": round(s[len(s) // 2], 4), "min": round(s[0], 4), "max": round(s[-1], 4)}


def _timed(fn):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def per_call(B, launches, rounds, segs):
    import torch
    import torch.nn.functional as F

    from katib_amd.ops import enas_head as hh
    from katib_amd.workloads.common import global_avg_pool

    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    graphs, keep = {}, []
    for H, W, C in SHAPES:
        x = torch.randn(B, C, H, W, device=dev, generator=gen).to(torch.bfloat16).contiguous(
            memory_format=torch.channels_last).requires_grad_(True)
        w = (torch.randn(K, C, device=dev, generator=gen) * 0.1).requires_grad_(True)
        b = torch.zeros(K, device=dev, requires_grad=True)
        y = torch.randint(0, K, (B,), device=dev, generator=gen)
        acc, step = torch.zeros(2, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        one = torch.ones(1, device=dev)
        drop = hh.Drop(0.4, 0, 0, step)
        keep.append((x, w, b, y, acc, step, one))  # the graphs hold their addresses

        def fused(s=0, x=x, w=w, b=b, y=y, acc=acc, drop=drop, one=one, H=H, W=W):
            if s == 0:
                return torch.autograd.grad(hh.head_loss(x, w, b, y, drop, acc), (x, w, b))
            parts = hh.forward_parts(x, w, b, y, drop, acc)
            return hh.backward_parts(parts, w, one, H, W, drop.p, segs=s)

        def module(x=x, w=w, b=b, y=y, acc=acc):
            with torch.autocast("cuda", dtype=torch.bfloat16):
                logits = F.linear(F.dropout(global_avg_pool(x), 0.4), w, b)
            loss = F.cross_entropy(logits.float(), y)
            g = torch.autograd.grad(loss, (x, w, b))
            acc[0].add_(loss.detach())
            acc[1].add_((logits.argmax(1) == y).sum())
            return g

        runs = {"module": module, "fused rule": fused}
        runs.update({"fused S=%d" % s: (lambda s=s, f=fused: f(s)) for s in segs if s <= H * W})
        for name, run in runs.items():
            for _ in range(3):
                run()
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                for _ in range(launches):
                    run()
            gr.replay()
            graphs[((H, W, C), name)] = gr
    torch.cuda.synchronize()
    times = {k: [] for k in graphs}
    for _ in range(rounds):  # round-robin: every variant sees the same moments of the machine
        for k, gr in graphs.items():
            times[k].append(_timed(gr.replay) * 1e3 / launches)
    for (shape, name), v in times.items():
        st = _stats(v)
        base = _stats(times[(shape, "module")])["median"]
        print(json.dumps({"shape": "%dx%dx%d" % shape, "batch": B, "path": name, "fwd+bwd_us": st,
                          "vs_module": round(st["median"] / base, 3),
                          "sample_KB": round(shape[0] * shape[1] * shape[2] * 2 / 1024, 1)}), flush=True)


def step_ab(B, window, rounds):
    import torch

    from katib_amd.workloads.enas_child import ChildTrainer

    trs = {h: ChildTrainer(ARCH, NN_CONFIG, num_train=4096, num_valid=256, batch_size=B, capture=True, seed=0, head=h)
           for h in ("module", "hip")}
    gen = torch.Generator(device="cuda").manual_seed(1)
    idx = [torch.randint(0, 4096, (B,), device="cuda", generator=gen) for _ in range(8)]
    for tr in trs.values():
        for s in range(tr.step_fn.warmup + 5):
            tr.step(idx[s % 8])
    torch.cuda.synchronize()
    times = {h: [] for h in trs}
    for _ in range(rounds):
        for h, tr in trs.items():
            def run(tr=tr):
                for s in range(window):
                    tr.step(idx[s % 8])
            times[h].append(_timed(run) / window)
    for h, v in times.items():
        print(json.dumps({"step": "3-layer child, batch %d, captured" % B, "head": h, "ms": _stats(v),
                          "loss_sum": round(float(trs[h].acc_buf[0]), 3)}), flush=True)
    m, f = _stats(times["module"])["median"], _stats(times["hip"])["median"]
    print(json.dumps({"step_ms": {"module": m, "hip": f, "ratio": round(f / m, 4)}}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--segs", type=str, default="", help="comma list of segment counts for the backward A/B")
    ap.add_argument("--step", action="store_true", help="time the captured child step, --head hip against module")
    ap.add_argument("--window", type=int, default=200)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_enas_head: no GPU")
    if a.step:
        step_ab(a.batch, a.window, a.rounds)
    else:
        per_call(a.batch, a.launches, a.rounds, [int(s) for s in a.segs.split(",") if s])


if __name__ == "__main__":
    main()
