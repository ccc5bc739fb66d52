"""Kernel time of the four cross-entropy kernels of the GPT-2 PBT member (csrc/hip/transformer.hip) at
its batch, 16384 token rows x 50304 padded columns of bf16 logits, with HIP events: the one-pass
training kernel (xent_fused_k), the two-pass pair (xent_fwd_k, xent_bwd_k) and the evaluation kernel
(xent_eval_k). ``KATIB_AMD_HIPKERN=<path to another build's _hipkern .so>`` times that build instead
of the in-tree one, for an A/B against another revision.

Prints one JSON line per kernel: median and minimum of ``--reps`` launches in ms."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timeit(fn, reps):
    import torch

    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return round(ts[len(ts) // 2], 4), round(ts[0], 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--vocab", type=int, default=50257)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--label", default=os.environ.get("KATIB_AMD_HIPKERN", "in-tree"))
    args = ap.parse_args()
    import torch

    from katib_amd.ops.transformer import HipOps

    hip, dev = HipOps(), torch.device("cuda", 0)
    N, V = args.rows, args.vocab
    Vp = -(-V // 64) * 64
    g = torch.Generator(device=dev).manual_seed(1)
    logits = (torch.randn(N, Vp, device=dev, generator=g) * 3).to(torch.bfloat16)
    tgt = torch.randint(0, V, (N,), device=dev, generator=g)
    gs = torch.full((1,), 0.7, device=dev)
    work = logits.clone()  # the gradient kernels overwrite their input; their time does not depend on its values
    _, lse = hip.xent_fwd(logits, tgt, V)
    for name, fn in (("xent_fused", lambda: hip.xent_train(work, tgt, gs, V)),
                     ("xent_fwd", lambda: hip.xent_fwd(logits, tgt, V)),
                     ("xent_bwd", lambda: hip.xent_bwd(work, tgt, lse, gs, V)),
                     ("xent_eval", lambda: hip.xent_eval(logits, tgt, V))):
        med, lo = timeit(fn, args.reps)
        print(json.dumps({"build": args.label, "kernel": name, "rows": N, "Vp": Vp, "median_ms": med, "min_ms": lo}))


if __name__ == "__main__":
    main()
