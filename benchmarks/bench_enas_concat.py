"""Cost of building an ENAS child layer's input (csrc/hip/enas_concat.hip: ReLU + zero-pad concat in
one kernel per direction) on one GPU, everything that is compared measured interleaved in one process.

The op alone against ``reference`` (F.pad per source, torch.cat, F.relu and their autograd backward)
at the child's batch of 128, for a 2-source and an 8-source layer of enas-gpu.yaml sizes: the
forward, and the forward with the backward of all sources. Each is captured as a graph of
``--launches`` back-to-back calls; the graphs are replayed round-robin and timed with device events.
The backward alone is the difference of the two medians. Prints one JSON line per measurement.

The captured child step with ``enas_child.FUSED_INPUT`` on and off is not measured here."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (C, H) per source
LAYERS = {"2 sources": [(64, 16), (32, 32)],
          "8 sources": [(64, 16), (32, 32), (64, 32), (32, 16), (128, 8), (64, 16), (96, 8), (48, 32)]}


def _stats(v):
    s = sorted(v)
    return {"median": round(s[len(s) // 2], 4), "min": round(s[0], 4), "max": round(s[-1], 4)}


def op_alone(B, launches, rounds):
    import torch

    from katib_amd.ops.enas_concat import reference, relu_pad_concat

    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    graphs, nbytes, inputs = {}, {}, []
    for lname, srcs in LAYERS.items():
        xs = [torch.randn(B, c, h, h, device=dev, generator=gen).to(torch.bfloat16).contiguous(
            memory_format=torch.channels_last).requires_grad_(True) for c, h in srcs]
        m, Ct = max(h for _, h in srcs), sum(c for c, _ in srcs)
        g = torch.randn(B, m, m, Ct, device=dev, generator=gen).to(torch.bfloat16).permute(0, 3, 1, 2)
        inputs.append((xs, g))  # the graphs hold their addresses: they live as long as the graphs are replayed
        nbytes[lname] = 2 * (sum(x.numel() for x in xs) + B * m * m * Ct)  # read once, written once
        for fname, fn in (("fused", relu_pad_concat), ("reference", reference)):
            assert torch.equal(fn(xs, True), reference(xs, True))
            for bwd in (False, True):
                def run(fn=fn, xs=xs, g=g, bwd=bwd):
                    if bwd:
                        torch.autograd.grad(fn(xs, True), xs, g)
                    else:
                        with torch.no_grad():
                            fn(xs, True)
                for _ in range(3):
                    run()
                torch.cuda.synchronize()
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr):
                    for _ in range(launches):
                        run()
                gr.replay()
                graphs[(lname, fname, "fwd+bwd" if bwd else "fwd")] = gr
    torch.cuda.synchronize()
    times = {k: [] for k in graphs}
    for _ in range(rounds):  # round-robin: every variant sees the same moments of the machine
        for k, gr in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            gr.replay()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / launches)
    for lname in LAYERS:
        med = {}
        for fname in ("fused", "reference"):
            for d in ("fwd", "fwd+bwd"):
                st = _stats(times[(lname, fname, d)])
                med[(fname, d)] = st["median"]
                passes = 1 if d == "fwd" else 2
                print(json.dumps({"op": lname, "path": fname, "what": d, "batch": B, "us": st,
                                  "least_GBps": round(passes * nbytes[lname] / (st["median"] * 1e-6) / 1e9, 1)}),
                      flush=True)
        f, r = med[("fused", "fwd")], med[("reference", "fwd")]
        fb, rb = med[("fused", "fwd+bwd")] - f, med[("reference", "fwd+bwd")] - r
        print(json.dumps({"op": lname, "fwd_us": {"fused": f, "reference": r, "ratio": round(f / r, 3)},
                          "bwd_us": {"fused": round(fb, 4), "reference": round(rb, 4), "ratio": round(fb / rb, 3)}}),
              flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=15)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_enas_concat: no GPU")
    op_alone(a.batch, a.launches, a.rounds)


if __name__ == "__main__":
    main()
