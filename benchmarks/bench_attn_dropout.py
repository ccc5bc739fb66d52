"""Cost of attention-probability dropout in the flash attention kernels (csrc/hip/transformer.hip):
forward and backward time of the HIP kernels at each ``--p`` (0 = the plain kernels, the path a
member without --attn-dropout runs), bf16, graph-captured timing as benchmarks/bench_attn.py.

Shape: the PBT member's batch (B=16, T=1024, H=12, d=64; ``ATTN_SHAPE`` overrides). Each p is timed
``--rounds`` times, the p values interleaved within a round, and reported as median / min / max so
a difference can be read against the spread. Prints one JSON line per p. To compare two builds of
the extension, run this script alternately with ``KATIB_AMD_HIPKERN`` pointing at each (``--p 0``
uses only entry points every build has).

``--trial-steps N`` first runs the whole PBT member (``katib_amd.workloads.gpt2_pbt``, batch 16, N
steps, a fresh process each, ``--trial-runs`` times) with ``--attn-dropout 0`` and with the last
``--p``, and prints the tokens/s each reports."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from benchmarks.bench_attn import timeit_graph  # noqa: E402


def main(argv=None):
    from katib_amd.ops.transformer import Drop, HipOps, attn_dropout_threshold

    ap = argparse.ArgumentParser()
    ap.add_argument("--p", type=float, nargs="+", default=[0.0, 0.1])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tag", default="")
    ap.add_argument("--trial-steps", type=int, default=0, help="also time whole member trials (0: kernels only)")
    ap.add_argument("--trial-runs", type=int, default=2)
    args = ap.parse_args(argv)
    if args.trial_steps > 0:  # before this process opens the GPU: each trial is a process of its own
        from benchmarks.bench_ln_dropout import ROOT, trial

        for i in range(args.trial_runs):
            for p in (0.0, args.p[-1]):
                trial(ROOT, ["--attn-dropout", str(p)], args.trial_steps, "attn-dropout %g run %d" % (p, i + 1))
    B, T, H, d = (int(v) for v in os.environ.get("ATTN_SHAPE", "16,1024,12,64").split(","))
    dev = torch.device("cuda", 0)
    ops = HipOps()
    g = torch.Generator(device=dev).manual_seed(0)
    qkv = (torch.randn(B * T, 3 * H * d, device=dev, generator=g) * 0.5).to(torch.bfloat16)
    dout = torch.randn(B * T, H * d, device=dev, generator=g).to(torch.bfloat16)
    step = torch.ones(1, device=dev)
    times = {p: {"fwd": [], "bwd": []} for p in args.p}
    for _ in range(args.rounds):
        for p in args.p:
            kw = {"drop": Drop(p, 25, 1234, step)} if attn_dropout_threshold(p) > 0 else {}
            o, lse = ops.attn_fwd(qkv, B, T, H, **kw)
            times[p]["fwd"].append(timeit_graph(lambda: ops.attn_fwd(qkv, B, T, H, **kw)))
            times[p]["bwd"].append(timeit_graph(lambda: ops.attn_bwd(qkv, o, dout, lse, B, T, H, **kw)))
    fwd_flops = 4.0 * B * H * T * T * d / 2
    for p in args.p:
        out = {"shape": [B, T, H, d], "p": p, "thr8": attn_dropout_threshold(p), "rounds": args.rounds}
        if args.tag:
            out["tag"] = args.tag
        for k, mult in (("fwd", 1.0), ("bwd", 2.5)):
            v = times[p][k]
            out["hip_%s_ms" % k] = round(statistics.median(v), 4)
            out["hip_%s_ms_min_max" % k] = [round(min(v), 4), round(max(v), 4)]
            out["hip_%s_tflops" % k] = round(mult * fwd_flops / statistics.median(v) / 1e9, 1)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
