"""Cost of the ENAS child's fused separable convolution (csrc/hip/enas_sepconv.hip) against the split path
on one GPU, everything that is compared measured interleaved in one process (the method of
bench_enas_head.py).

Per call (default), at batch 128 for SHAPES: the fused forward against ``dw_fwd`` + the 1x1 ``conv_fwd`` +
the bias add, and forward + backward of each (the fused backward is ``sep_bwd_pw`` + ``dw_dgrad`` +
``dw_wgrad`` + the bias sum); the backward alone is reported as the difference of the two. Each arm is
captured as a graph of ``--launches`` back-to-back calls; the graphs are replayed round-robin and timed
with device events. ``GB_moved`` is what the arm has to move through HBM by its algorithm (every tensor
once per kernel that reads or writes it, weights left out), ``GB_per_s`` that over the median time.

``--step``: a captured child whose layers 1-3 are separable (``--head hip --optim hip``), ``--sep fused``
against ``--sep split`` in alternating windows of ``--window`` steps, with the peak memory of each arm's
step. ``--split-only`` times the ``split`` step alone, for runs of this commit against its parent in
alternating processes. Prints one JSON line per measurement."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (H, W, C, dm, K, S, F): what the service emits; a wider input; k5 s2 dm 2; the 528-channel all-skip layer
SHAPES = [(32, 32, 64, 1, 3, 1, 64), (32, 32, 128, 1, 3, 1, 64), (16, 16, 64, 2, 5, 2, 128), (32, 32, 528, 1, 3, 1, 64)]

SEP = {"opt_type": "separable_convolution", "filter_size": "3", "num_filter": "64", "stride": "1", "depth_multiplier": "1"}
EMB = {"0": {"opt_type": "convolution", "filter_size": "3", "num_filter": "64", "stride": "1"}, "1": SEP}
NN_CONFIG = {"num_layers": 4, "input_sizes": [32, 32, 3], "output_sizes": [10], "embedding": EMB}
ARCH = [[0], [1, 0], [1, 0, 1], [1, 0, 1, 1]]  # the stem convolution, then separable layers on 64 / 128 / 192 channels


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


def _bytes(B, H, W, C, dm, K, S, F):
    """HBM bytes each arm must move, bf16 activations: x, d, y / gy, gd, gx."""
    OH, OW = -(-H // S), -(-W // S)
    x, d, y = 2 * B * H * W * C, 2 * B * OH * OW * C * dm, 2 * B * OH * OW * F
    nch = -(-C * dm // 64)
    return {"fwd split": x + d + d + y + 2 * y,  # dw_fwd, conv_fwd, the bias add
            "fwd fused": x + y,
            # bias sum, 1x1 dgrad (gy -> gd), 1x1 wgrad (d, gy), dw_dgrad (gd -> gx), dw_wgrad (x, gd)
            "bwd split": y + (y + d) + (d + y) + (d + x) + (x + d),
            # sep_bwd_pw reads x and gy once per chunk and writes gd
            "bwd fused": y + (x + nch * y + d) + (d + x) + (x + d)}


def per_call(B, launches, rounds):
    import torch

    from katib_amd.ops import conv as hconv, dwconv as hdw, enas_sepconv as hs

    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    graphs, keep, moved = {}, [], {}
    for shape in SHAPES:
        H, W, C, dm, K, S, F = shape
        x = torch.randn(B, C, H, W, device=dev, generator=gen).to(torch.bfloat16).contiguous(
            memory_format=torch.channels_last).requires_grad_(True)
        wd = (torch.randn(C * dm, 1, K, K, device=dev, generator=gen) * 0.2).requires_grad_(True)
        wp = (torch.randn(F, C * dm, 1, 1, device=dev, generator=gen) * 0.05).requires_grad_(True)
        b = torch.zeros(F, device=dev, requires_grad=True)
        gy = torch.randn(B, F, -(-H // S), -(-W // S), device=dev, generator=gen).to(torch.bfloat16).contiguous(
            memory_format=torch.channels_last)
        assert hs.supported(x, wd, wp, S)
        leaves = (x, wd, wp, b)
        keep.append(leaves + (gy,))
        fwd = {"fused": lambda x=x, wd=wd, wp=wp, b=b, S=S: hs.separable_same(x, wd, wp, b, S),
               "split": lambda x=x, wd=wd, wp=wp, b=b, S=S: hconv.conv2d(hdw.depthwise_same(x, wd, None, S), wp, b)}
        for name, f in fwd.items():
            # forward and backward of one call are built inside the same graph: a backward captured apart from
            # its forward would run on the stream the forward ran on, outside the capture
            runs = {"fwd " + name: lambda f=f: [f() for _ in range(launches)],
                    "f+b " + name: lambda f=f, gy=gy, leaves=leaves: [
                        torch.autograd.grad(f(), leaves, gy) for _ in range(launches)]}
            for key, run in runs.items():
                for _ in range(2):
                    run()
                torch.cuda.synchronize()
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr):
                    run()
                gr.replay()
                graphs[(shape, key)] = gr
        moved[shape] = _bytes(B, *shape)
    torch.cuda.synchronize()
    times = {k: [] for k in graphs}
    for _ in range(rounds):  # round-robin: every variant sees the same moments of the machine
        for k, gr in graphs.items():
            times[k].append(_timed(gr.replay) * 1e3 / launches)
    med = {k: _stats(v)["median"] for k, v in times.items()}
    for (shape, key), v in times.items():
        st, arm = _stats(v), key[4:]
        gb = moved[shape]["fwd " + arm] + (moved[shape]["bwd " + arm] if key[:3] == "f+b" else 0)
        print(json.dumps({"shape": "%dx%dx%d dm%d k%d s%d -> %d" % shape, "batch": B, "arm": key, "us": st,
                          "vs_split": round(st["median"] / med[(shape, key[:4] + "split")], 3),
                          "GB_moved": round(gb / 1e9, 4), "GB_per_s": round(gb / 1e3 / st["median"], 1)}), flush=True)
    for shape in SHAPES:  # the backward alone: the difference of the two medians of an arm
        bw = {arm: med[(shape, "f+b " + arm)] - med[(shape, "fwd " + arm)] for arm in ("split", "fused")}
        print(json.dumps({"shape": "%dx%dx%d dm%d k%d s%d -> %d" % shape, "bwd_us_by_difference": {
            a: round(t, 2) for a, t in bw.items()}, "vs_split": round(bw["fused"] / bw["split"], 3),
            "GB_moved": {a: round(moved[shape]["bwd " + a] / 1e9, 4) for a in bw}}), flush=True)


def step_ab(B, window, rounds, arms):
    import torch

    from katib_amd.workloads.enas_child import ChildTrainer

    trs, peak = {}, {}
    gen = torch.Generator(device="cuda").manual_seed(1)
    idx = [torch.randint(0, 4096, (B,), device="cuda", generator=gen) for _ in range(8)]
    for sep in arms:
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        kw = {"sep": sep} if sep != "split" else {}  # the split arm also runs on the parent commit
        trs[sep] = tr = ChildTrainer(ARCH, NN_CONFIG, num_train=4096, num_valid=256, batch_size=B, capture=True, seed=0,
                                     head="hip", optim="hip", **kw)
        for s in range(tr.step_fn.warmup + 5):
            tr.step(idx[s % 8])
        torch.cuda.synchronize()
        peak[sep] = round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1)
    times = {h: [] for h in trs}
    for _ in range(rounds):
        for h, tr in trs.items():
            def run(tr=tr):
                for s in range(window):
                    tr.step(idx[s % 8])
            times[h].append(_timed(run) / window)
    for h, v in times.items():
        print(json.dumps({"step": "stem + 3 separable layers, batch %d, captured, head hip, optim hip" % B, "sep": h,
                          "ms": _stats(v), "loss_sum": round(float(trs[h].acc_buf[0]), 3),
                          "peak_MiB_over_start": peak[h]}), flush=True)
    if len(arms) == 2:
        m, f = _stats(times["split"])["median"], _stats(times["fused"])["median"]
        print(json.dumps({"step_ms": {"split": m, "fused": f, "ratio": round(f / m, 4)}}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--step", action="store_true", help="time the captured child step, --sep fused against split")
    ap.add_argument("--split-only", action="store_true", help="with --step: the split arm alone")
    ap.add_argument("--window", type=int, default=200)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_enas_sepconv: no GPU")
    if a.step:
        step_ab(a.batch, a.window, a.rounds, ["split"] if a.split_only else ["split", "fused"])
    else:
        per_call(a.batch, a.launches, a.rounds)


if __name__ == "__main__":
    main()
