"""Cost of the ENAS child's flip + translation augmentation (csrc/hip/augment.hip: augment_nhwc_k)
on one GPU, everything that is compared measured interleaved in one process.

1. The batch gathers at the child's batch of 128 out of a 50,000-image set: the translating gather
   (u8 and bf16 sources), the plain and the crop-mode gather into NHWC, the existing crop-mode gather
   into NCHW fp32, and the ``index_select`` of the channels-last bf16 set that the child's step runs
   without the new flags. Each is captured as a graph of ``--launches`` back-to-back launches and the
   graphs are replayed round-robin, timed with device events; bytes written over time is the rate.
2. One captured child step (a fixed 3-layer architecture, batch 128, synthetic set) with and without
   augmentation: two trainers in this process, alternating windows of ``--steps`` steps.
3. ``--baseline DIR``: the un-augmented step of this tree against the step of another revision's
   Python tree (``DIR``, loading this tree's kernels), alternating processes - the step that runs
   without the new flags is meant to be the same code.

Prints one JSON line per measurement. ``--mode kernels`` only launches every gather ``--launches``
times, for a kernel trace taken by a profiler in a run of its own."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EMB = {"0": {"opt_type": "convolution", "opt_id": 0, "filter_size": "3", "num_filter": "32", "stride": "1"},
       "1": {"opt_type": "separable_convolution", "opt_id": 1, "filter_size": "3", "num_filter": "32", "stride": "2",
             "depth_multiplier": "1"},
       "2": {"opt_type": "convolution", "opt_id": 2, "filter_size": "3", "num_filter": "64", "stride": "1"}}
NN_CONFIG = {"num_layers": 3, "input_sizes": [32, 32, 3], "output_sizes": [10], "embedding": EMB}
ARCH = [[0], [1, 0], [2, 0, 0]]


def _stats(v):
    s = sorted(v)
    return {"median": round(s[len(s) // 2], 4), "min": round(s[0], 4), "max": round(s[-1], 4)}


def gather_variants(B, n_set):
    """name -> (fn, bytes written), every fn writing a static buffer from fixed random indices."""
    import torch

    from katib_amd.ops.augment import AugSpec, augment_gather, cifar_lut

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    u8 = torch.randint(0, 256, (n_set, 32, 32, 4), device=dev, generator=g, dtype=torch.uint8)
    lut = cifar_lut((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)).to(dev)
    nchw = torch.randn(n_set, 3, 32, 32, device=dev, generator=g).to(torch.bfloat16).contiguous(
        memory_format=torch.channels_last)
    bf = nchw.permute(0, 2, 3, 1)  # the same memory as [N, H, W, C]
    idx = torch.randint(0, n_set, (B,), device=dev, generator=g)
    epoch_t = torch.zeros(1, dtype=torch.int32, device=dev)
    tr = AugSpec(pad=0, flip=True, translate=0.1, seed=1, epoch=epoch_t)
    crop = AugSpec(pad=4, flip=True, seed=1, epoch=epoch_t)
    plain = AugSpec(pad=0, flip=False)
    o_nhwc = torch.empty(B, 32, 32, 3, device=dev, dtype=torch.bfloat16)
    o_nchw = torch.empty(B, 3, 32, 32, device=dev)
    nb, nf = o_nhwc.numel() * 2, o_nchw.numel() * 4
    return {
        "translate u8 -> NHWC": (lambda: augment_gather(u8, idx, tr, lut, out=o_nhwc, nhwc=True), nb),
        "translate bf16 -> NHWC": (lambda: augment_gather(bf, idx, tr, out=o_nhwc, nhwc=True), nb),
        "plain u8 -> NHWC": (lambda: augment_gather(u8, idx, plain, lut, out=o_nhwc, nhwc=True), nb),
        "plain bf16 -> NHWC": (lambda: augment_gather(bf, idx, plain, out=o_nhwc, nhwc=True), nb),
        "crop u8 -> NHWC": (lambda: augment_gather(u8, idx, crop, lut, out=o_nhwc, nhwc=True), nb),
        "crop u8 -> NCHW fp32": (lambda: augment_gather(u8, idx, crop, lut, out=o_nchw), nf),
        "index_select bf16": (lambda: nchw.index_select(0, idx), nb),
    }


def gathers(B, n_set, launches, rounds):
    import torch

    variants = gather_variants(B, n_set)
    graphs = {}
    for name, (fn, _) in variants.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(launches):
                fn()
        g.replay()
        graphs[name] = g
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(rounds):  # round-robin: every variant sees the same moments of the machine
        for name, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / launches)
    base = _stats(times["index_select bf16"])["median"]
    for name, (_, nbytes) in variants.items():
        st = _stats(times[name])
        print(json.dumps({"gather": name, "batch": B, "us": st, "written_MB": round(nbytes / 1e6, 3),
                          "GBps": round(nbytes / (st["median"] * 1e-6) / 1e9, 1),
                          "vs_index_select": round(st["median"] / base, 2)}), flush=True)


def kernels_only(B, n_set, launches):
    import torch

    for name, (fn, _) in gather_variants(B, n_set).items():
        for _ in range(launches):
            fn()
    torch.cuda.synchronize()
    print("kernels: %d launches of every gather done" % launches, flush=True)


def _trainer(augment, B, num_train):
    from katib_amd.workloads.enas_child import ChildTrainer

    kw = {"augment": True} if augment else {}  # no new argument: the step another revision's tree runs too
    return ChildTrainer(ARCH, NN_CONFIG, num_train=num_train, num_valid=128, batch_size=B, capture=True, seed=0, **kw)


def _window(tr, batches, steps):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(steps):
        tr.step(batches[s % len(batches)])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def child_steps(B, num_train, steps, windows, which):
    import torch

    trs = {name: _trainer(name == "augment 1", B, num_train) for name in which}
    any_tr = next(iter(trs.values()))
    g = torch.Generator(device=any_tr.dev).manual_seed(1)
    batches = [torch.randint(0, num_train, (B,), device=any_tr.dev, generator=g) for _ in range(16)]
    for tr in trs.values():  # warm-up runs, the capture and a first window
        _window(tr, batches, 20)
        assert tr.step_fn.graph is not None
    times = {name: [] for name in trs}
    for w in range(windows):
        for name, tr in trs.items():
            if getattr(tr, "epoch_t", None) is not None:
                tr.epoch_t.fill_(w)
            times[name].append(_window(tr, batches, steps))
    for name, tr in trs.items():
        print(json.dumps({"child_step": name, "batch": B, "steps_per_window": steps, "ms": _stats(times[name]),
                          "windows": [round(t, 4) for t in times[name]],
                          "loss_finite": bool(torch.isfinite(tr.acc_buf[0]))}), flush=True)
    if len(trs) == 2:
        a, b = (_stats(times[n])["median"] for n in ("augment 0", "augment 1"))
        print(json.dumps({"child_step": "augment 1 / augment 0", "ratio": round(b / a, 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mode", default="all", choices=["all", "gathers", "kernels", "steps", "plain-step"])
    ap.add_argument("--tree", default=ROOT, help="the Python tree to import katib_amd from")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--set-size", type=int, default=50000)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--num-train", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--baseline", default="", help="Python tree of the revision to compare the plain step against")
    ap.add_argument("--baseline-rounds", type=int, default=3)
    a = ap.parse_args()
    if a.baseline and a.mode == "all":  # child processes first: this one has not opened the GPU yet
        import glob

        so = glob.glob(os.path.join(ROOT, "katib_amd", "_hipkern.*.so")) + glob.glob(
            os.path.join(ROOT, "katib_amd", "_hipkern.so"))
        env = dict(os.environ, KATIB_AMD_HIPKERN=so[0])
        for r in range(a.baseline_rounds):
            for label, tree in (("baseline", os.path.abspath(a.baseline)), ("this tree", ROOT)):
                print("-- round %d %s" % (r + 1, label), flush=True)
                subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", "plain-step", "--tree", tree,
                                "--batch", str(a.batch), "--num-train", str(a.num_train), "--steps", str(a.steps),
                                "--windows", str(a.windows)], env=env, check=True, timeout=600)
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_augment_translate: no GPU")
    if a.mode == "kernels":
        return kernels_only(a.batch, a.set_size, a.launches)
    if a.mode == "plain-step":
        return child_steps(a.batch, a.num_train, a.steps, a.windows, ["augment 0"])
    if a.mode in ("all", "gathers"):
        gathers(a.batch, a.set_size, a.launches, a.rounds)
    if a.mode in ("all", "steps"):
        child_steps(a.batch, a.num_train, a.steps, a.windows, ["augment 0", "augment 1"])


if __name__ == "__main__":
    main()
