"""Cost of the fused dropout of the GPT-2 PBT member (csrc/hip/transformer.hip) on one GPU.

1. The residual-add LayerNorm forward and backward at the member's batch (M = 16384 rows, D = 768),
   graph-captured and warmed, timed with HIP events: the existing kernels (p = 0) against the
   dropout kernels (p = 0.1).
2. The trial itself, ``python -m katib_amd.workloads.gpt2_pbt --batch-size 16``, at ``--dropout 0``
   and ``--dropout 0.1``: tokens/s as the trial reports them, each run a fresh process.
3. ``--baseline DIR``: the same trial command (no ``--dropout``) from a built checkout of another
   revision, run ``--baseline-runs`` times, for the run-to-run spread to hold 2. against.

Prints one JSON line per measurement."""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timeit_graph(fn, it=20, reps=10):
    import torch

    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(it):
            fn()
    g.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / it)
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def kernels(M, D, p):
    import torch

    from katib_amd.ops.transformer import Drop, HipOps

    dev = torch.device("cuda", 0)
    ops = HipOps()
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(M, D, device=dev, generator=g)
    r = torch.randn(M, D, device=dev, generator=g).to(torch.bfloat16)
    dy = torch.randn(M, D, device=dev, generator=g).to(torch.bfloat16)
    gamma = torch.ones(D, device=dev, dtype=torch.bfloat16)
    beta = torch.zeros(D, device=dev, dtype=torch.bfloat16)
    G = torch.randn(M, D, device=dev, generator=g)
    dr = torch.empty(M, D, device=dev, dtype=torch.bfloat16)
    dg, db, dbias = (torch.empty(D, device=dev, dtype=torch.bfloat16) for _ in range(3))
    step = torch.ones(1, device=dev)
    xin, _, mean, rstd = ops.ln_fwd(x, r, gamma, beta)
    # bytes the two kernels move: x32 + r in, xo + y out; dy + xin + G in, G + dr out
    gb = {"ln_fwd": M * D * (4 + 2 + 4 + 2) / 1e9, "ln_bwd": M * D * (2 + 4 + 4 + 4 + 2) / 1e9}
    for pp in (0.0, p):
        drop = Drop(pp, 3, 1234, step) if pp > 0 else None
        runs = {"ln_fwd": lambda: ops.ln_fwd(x, r, gamma, beta, drop=drop),
                "ln_bwd": lambda: ops.ln_bwd(dy, xin, mean, rstd, gamma, G, dr, dg, db, dbias=dbias, drop=drop)}
        for name, fn in runs.items():
            med, lo, hi = timeit_graph(fn)
            extra = " (+ ln_reduce)" if name == "ln_bwd" else ""
            print(json.dumps({"kernel": name + extra, "M": M, "D": D, "p": pp, "us": round(med * 1e3, 2),
                              "us_min": round(lo * 1e3, 2), "us_max": round(hi * 1e3, 2),
                              "GBps": round(gb[name] / (med * 1e-3), 1)}), flush=True)


def trial(cwd, extra, steps, label):
    cmd = [sys.executable, "-m", "katib_amd.workloads.gpt2_pbt", "--batch-size", "16", "--steps", str(steps),
           "--p2p", "0"] + extra
    env = dict(os.environ, PYTHONPATH=cwd)
    out = subprocess.run(cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=900)
    m = re.search(r"tokens_per_s=([0-9.e+]+)", out.stdout)
    v = re.search(r"Validation-loss=([0-9.e+-]+)", out.stdout)
    if out.returncode != 0 or not m:
        print(out.stdout[-2000:], out.stderr[-2000:], file=sys.stderr)
        raise SystemExit("trial failed: %s (exit %d)" % (" ".join(cmd), out.returncode))
    print(json.dumps({"trial": label, "args": " ".join(cmd[2:]), "tokens_per_s": float(m.group(1)),
                      "validation_loss": float(v.group(1)) if v else None}), flush=True)
    return float(m.group(1))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--M", type=int, default=16384)
    ap.add_argument("--D", type=int, default=768)
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--steps", type=int, default=60, help="trial steps (0: kernels only)")
    ap.add_argument("--runs", type=int, default=2, help="runs of each trial variant")
    ap.add_argument("--baseline", default="", help="built checkout of the revision to compare against")
    ap.add_argument("--baseline-runs", type=int, default=2)
    ap.add_argument("--skip-kernels", action="store_true")
    a = ap.parse_args()
    if a.steps > 0:  # the trials first: each is a process of its own and this one has not opened the GPU yet
        for i in range(max(a.runs, a.baseline_runs if a.baseline else 0)):
            if a.baseline and i < a.baseline_runs:
                trial(os.path.abspath(a.baseline), [], a.steps, "baseline run %d" % (i + 1))
            if i < a.runs:
                trial(ROOT, ["--dropout", "0"], a.steps, "dropout 0 run %d" % (i + 1))
                trial(ROOT, ["--dropout", str(a.p)], a.steps, "dropout %g run %d" % (a.p, i + 1))
    if not a.skip_kernels:
        kernels(a.M, a.D, a.p)


if __name__ == "__main__":
    main()
