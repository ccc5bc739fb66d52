"""Cost of the ENAS child's gradient fan-in (csrc/hip/enas_fanin.hip, ops/enas_fanin.py) on one GPU,
everything that is compared measured interleaved in one process.

Per call (default): one ``enas_fanin`` launch over ``n`` readers of a 64-channel 32x32 layer at the child's
batch of 128, against what it replaces - per reader the concat backward that writes that reader's full-size
gradient of the layer (``enas_concat_bwd`` with the layer as the one source that wants a gradient), then the
``n - 1`` bf16 adds with which autograd folds them - for 2, 4 and 7 readers, and for 4 readers of which one
took the 3-channel image in front under ``pad8`` (the funnel path). Every reader is a two-source ReLU layer
with the producer second. Each arm is captured as a graph of ``--launches`` back-to-back calls; the graphs
are replayed round-robin and timed with device events.

``--step``: the captured step of an 8-layer all-skip child with ``--head hip --optim hip``, ``--gradsum hip``
against ``autograd``, in alternating windows of ``--window`` steps, and each arm's peak device memory above
what was allocated before it was built (the readers' output gradients now live until the producer's fan-in
runs). ``--pad8 1`` sets ``enas_child.PAD8_INPUT`` for both arms. Prints one JSON line per measurement."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, H = 64, 32
CASES = {"2 readers": (2, False), "4 readers": (4, False), "7 readers": (7, False), "4 readers, one pad8": (4, True)}
EMB = {"0": {"opt_type": "convolution", "filter_size": "3", "num_filter": "64", "stride": "1"},
       "1": {"opt_type": "separable_convolution", "filter_size": "3", "num_filter": "64", "stride": "2",
             "depth_multiplier": "1"},
       "2": {"opt_type": "convolution", "filter_size": "3", "num_filter": "64", "stride": "1"}}
ARCH = [[l % 3] + [1] * l for l in range(8)]
CONFIG = {"num_layers": 8, "input_sizes": [32, 32, 3], "output_sizes": [10], "embedding": EMB}


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


def per_call(B, launches, rounds):
    import torch

    from katib_amd.ops.conv import kernels

    k, dev = kernels(), torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B, H, H, C, device=dev, generator=gen).to(torch.bfloat16)
    graphs, keep = {}, []
    for name, (n, pad8) in CASES.items():
        # reader r: sources (other 64 channels | the image under pad8, the producer), so off = 64 | 3
        readers = []
        for r in range(n):
            first = 3 if pad8 and r == 0 else 64
            Cs = (first + C + 7) // 8 * 8
            readers.append((first, torch.randn(B, H, H, Cs, device=dev, generator=gen).to(torch.bfloat16)))
        gxs = [torch.empty_like(x) for _ in range(n)]
        out = torch.empty_like(x)
        terms = [(g, first, True) for first, g in readers]

        def replaced(readers=readers, gxs=gxs):
            for (first, g), gx in zip(readers, gxs):
                k.enas_concat_bwd([[H, first], [H, C]], B, [None, x], [None, gx], g, True, first == 3)
            s = gxs[0]
            for gx in gxs[1:]:
                s = s + gx
            return s

        def fanin(terms=terms, out=out):
            k.enas_fanin(x, terms, out)
            return out

        a, b = replaced().float(), fanin().float()
        # a sanity check, not a test: n - 1 bf16 roundings of partial sums against one
        assert (a - b).abs().max() <= 2.0 ** -5 * b.abs().max(), "the two arms differ by more than bf16 rounding"
        keep.append((readers, gxs, out))
        for arm, fn in (("replaced", replaced), ("fanin", fanin)):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                for _ in range(launches):
                    fn()
            gr.replay()
            graphs[(name, arm)] = gr
    torch.cuda.synchronize()
    times = {key: [] for key in graphs}
    for _ in range(rounds):  # round-robin: every arm sees the same moments of the machine
        for key, gr in graphs.items():
            times[key].append(_timed(gr.replay) * 1e3 / launches)
    for name, (n, pad8) in CASES.items():
        st = {arm: _stats(times[(name, arm)]) for arm in ("replaced", "fanin")}
        least = 2 * x.numel() * (n + 2)  # n gradient reads of the producer's channels, the mask, the write
        print(json.dumps({"case": name, "batch": B, "us": st,
                          "fanin/replaced": round(st["fanin"]["median"] / st["replaced"]["median"], 3),
                          "fanin_least_GBps": round(least / (st["fanin"]["median"] * 1e-6) / 1e9, 1)}), flush=True)


def step_ab(B, window, rounds, pad8):
    import torch

    from katib_amd.workloads import enas_child

    enas_child.PAD8_INPUT = bool(pad8)
    trs, peak = {}, {}
    gen = torch.Generator(device="cuda").manual_seed(1)
    idx = [torch.randint(0, 4096, (B,), device="cuda", generator=gen) for _ in range(8)]
    for arm in ("autograd", "hip"):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        trs[arm] = tr = enas_child.ChildTrainer(ARCH, CONFIG, num_train=4096, num_valid=256, batch_size=B, capture=True,
                                                seed=0, head="hip", optim="hip", gradsum=arm)
        for s in range(tr.step_fn.warmup + 5):
            tr.step(idx[s % 8])
        torch.cuda.synchronize()
        peak[arm] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
    times = {arm: [] for arm in trs}
    for _ in range(rounds):
        for arm, tr in trs.items():
            def run(tr=tr):
                for s in range(window):
                    tr.step(idx[s % 8])
            times[arm].append(_timed(run) / window)
    for arm, v in times.items():
        print(json.dumps({"step": "8-layer all-skip child, batch %d, captured, head hip, optim hip, pad8 %d" % (B, pad8),
                          "gradsum": arm, "ms": _stats(v), "peak_MiB": peak[arm],
                          "loss_sum": round(float(trs[arm].acc_buf[0]), 3)}), flush=True)
    a, h = _stats(times["autograd"])["median"], _stats(times["hip"])["median"]
    print(json.dumps({"step_ms": {"autograd": a, "hip": h, "ratio": round(h / a, 4)}, "peak_MiB": peak}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--step", action="store_true", help="time the captured child step, --gradsum hip against autograd")
    ap.add_argument("--window", type=int, default=200)
    ap.add_argument("--pad8", type=int, default=0, choices=[0, 1])
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_enas_fanin: no GPU")
    if a.step:
        step_ab(a.batch, a.window, a.rounds, a.pad8)
    else:
        per_call(a.batch, a.launches, a.rounds)


if __name__ == "__main__":
    main()
