"""Cost of the ENAS child's one-launch Adam (csrc/hip/enas_optim.hip, ops/enas_optim.py) on one GPU,
everything that is compared measured interleaved in one process.

Per call (default): ``ChildAdam.step()`` against what it replaces in the ``--optim module`` step - fused
capturable ``torch.optim.Adam``, ``zero_grad``, and per layer the bf16 weight copies of the forward and the
backward, the accumulator ``zeros``, the gradient slice + permute and ``part.sum(0)`` - on the parameter
sets of the three-layer child of ``bench_enas_head.py`` and of an eight-layer all-skip child. Each is
captured as a graph of ``--launches`` back-to-back calls; the graphs are replayed round-robin and timed
with device events.

``--step``: the captured three-layer child step with ``--head hip``, ``--optim hip`` against ``--optim
module``, in alternating windows of ``--window`` steps. ``--step --only module`` times the default path
alone (for a comparison between two checkouts). Prints one JSON line per measurement."""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EMB = {"0": {"opt_type": "convolution", "filter_size": "3", "num_filter": "64", "stride": "1"},
       "1": {"opt_type": "separable_convolution", "filter_size": "3", "num_filter": "64", "stride": "2",
             "depth_multiplier": "1"},
       "2": {"opt_type": "convolution", "filter_size": "3", "num_filter": "64", "stride": "1"}}
CHILDREN = {"3-layer": (3, [[0], [1, 0], [2, 0, 1]]),
            "8-layer all-skip": (8, [[l % 3] + [1] * l for l in range(8)])}


def _config(layers):
    return {"num_layers": layers, "input_sizes": [32, 32, 3], "output_sizes": [10], "embedding": EMB}


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


def _replaced(model, opt, segs):
    """The framework work of one ``--optim module`` step that ``ChildAdam.step()`` stands for, on buffers of
    the same sizes: what ``_ConvFn`` / ``_DwFn`` run around their kernels on a layer without a ``prep`` record
    (the image copies, the accumulator ``zeros``, the gradient permute, ``part.sum(0)``), ``zero_grad`` and the
    fused Adam."""
    import torch
    import torch.nn.functional as F

    from katib_amd.ops.enas_optim import CONV, DEPTHWISE

    params = dict(model.named_parameters())

    def run():
        opt.zero_grad(set_to_none=False)
        for s in segs:
            w = params[s.name]
            if s.kind == CONV:
                K, C, R, S = s.shape
                wk = F.pad(w.detach().permute(0, 2, 3, 1).to(torch.bfloat16), (0, s.C8 - C)).contiguous()
                if s.wt is not None:
                    wk.permute(3, 1, 2, 0).contiguous()
                dw32 = torch.zeros((K, R * S * s.C8), device=w.device)
                w.grad.add_(dw32.view(K, R, S, s.C8)[..., :C].permute(0, 3, 1, 2))
            elif s.kind == DEPTHWISE:
                w.detach().reshape(s.K, s.RS).t().contiguous()
                w.grad.add_(s.g.sum(0).view(s.shape))
        opt.step()
    return run


def per_call(launches, rounds):
    import torch

    from katib_amd.ops.enas_optim import ChildAdam
    from katib_amd.workloads.enas_child import ChildNet

    dev = torch.device("cuda", 0)
    graphs, keep = {}, []
    for name, (layers, arch) in CHILDREN.items():
        torch.manual_seed(0)
        model = ChildNet(arch, _config(layers)).to(dev).to(memory_format=torch.channels_last)
        plain = copy.deepcopy(model)
        hip = ChildAdam(model)
        x = torch.randn(16, 3, 32, 32, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        with torch.autocast("cuda", dtype=torch.bfloat16):  # sizes the depthwise partials; the values do not matter
            model(x).float().sum().backward()
        adam = torch.optim.Adam(plain.parameters(), lr=1e-3, fused=True, capturable=True)
        for p in plain.parameters():
            p.grad = torch.zeros_like(p)
        keep.append((model, plain, hip, adam))
        kinds = [s.kind for s in hip.segs]
        info = {"child": name, "tensors": len(kinds), "conv": kinds.count(1), "depthwise": kinds.count(2),
                "flat": kinds.count(0), "elements": sum(s.p.numel() for s in hip.segs)}
        for path, run in (("module", _replaced(plain, adam, hip.segs)), ("hip", hip.step)):
            for _ in range(3):
                run()
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                for _ in range(launches):
                    run()
            gr.replay()
            graphs[(name, path)] = (gr, info)
    torch.cuda.synchronize()
    times = {k: [] for k in graphs}
    for _ in range(rounds):  # round-robin: every variant sees the same moments of the machine
        for k, (gr, _) in graphs.items():
            times[k].append(_timed(gr.replay) * 1e3 / launches)
    for (name, path), v in times.items():
        st = _stats(v)
        base = _stats(times[(name, "module")])["median"]
        print(json.dumps(dict(graphs[(name, path)][1], path=path, us=st, vs_module=round(st["median"] / base, 3))),
              flush=True)


def step_ab(B, window, rounds, only):
    import torch

    from katib_amd.workloads.enas_child import ChildTrainer

    layers, arch = CHILDREN["3-layer"]
    trs = {}
    for o in ([only] if only else ["module", "hip"]):
        kw = {"optim": o} if o != "module" else {}  # the default path takes no new argument
        trs[o] = ChildTrainer(arch, _config(layers), num_train=4096, num_valid=256, batch_size=B, capture=True, seed=0,
                              head="hip", **kw)
    gen = torch.Generator(device="cuda").manual_seed(1)
    idx = [torch.randint(0, 4096, (B,), device="cuda", generator=gen) for _ in range(8)]
    for tr in trs.values():
        for s in range(tr.step_fn.warmup + 5):
            tr.step(idx[s % 8])
    torch.cuda.synchronize()
    times = {o: [] for o in trs}
    for _ in range(rounds):
        for o, tr in trs.items():
            def run(tr=tr):
                for s in range(window):
                    tr.step(idx[s % 8])
            times[o].append(_timed(run) / window)
    for o, v in times.items():
        print(json.dumps({"step": "3-layer child, batch %d, captured, head hip" % B, "optim": o, "ms": _stats(v),
                          "loss_sum": round(float(trs[o].acc_buf[0]), 3)}), flush=True)
    if not only:
        m, f = _stats(times["module"])["median"], _stats(times["hip"])["median"]
        print(json.dumps({"step_ms": {"module": m, "hip": f, "ratio": round(f / m, 4)}}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--step", action="store_true", help="time the captured child step, --optim hip against module")
    ap.add_argument("--only", type=str, default="", choices=["", "module", "hip"])
    ap.add_argument("--window", type=int, default=200)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_enas_optim: no GPU")
    if a.step:
        step_ab(a.batch, a.window, a.rounds, a.only)
    else:
        per_call(a.launches, a.rounds)


if __name__ == "__main__":
    main()
