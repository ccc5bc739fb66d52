"""Cost of building an ENAS child layer's input (csrc/hip/enas_concat.hip: ReLU + zero-pad concat in
one kernel per direction) on one GPU, everything that is compared measured interleaved in one process.

The op alone against ``reference`` (F.pad per source, torch.cat, F.relu and their autograd backward)
at the child's batch of 128, for a 2-source and an 8-source layer of enas-gpu.yaml sizes: the
forward, and the forward with the backward of all sources. Each is captured as a graph of
``--launches`` back-to-back calls; the graphs are replayed round-robin and timed with device events.
The backward alone is the difference of the two medians. Prints one JSON line per measurement.
Then the same method for two layers with the 3-channel image as second source (``image_second``).

The captured child step with ``enas_child.FUSED_INPUT`` on and off is not measured here."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (C, H) per source
LAYERS = {"2 sources": [(64, 16), (32, 32)],
          "8 sources": [(64, 16), (32, 32), (64, 32), (32, 16), (128, 8), (64, 16), (96, 8), (48, 32)]}
# the 3-channel image as second source: Ct = 67 and 531
IMAGE_LAYERS = {"64 ch + image": [(64, 32), (3, 32)],
                "8 sources + image": LAYERS["8 sources"][:1] + [(3, 32)] + LAYERS["8 sources"][1:]}


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


def image_second(B, launches, rounds):
    """The image as second source (``ChildNet.inputs`` order): the element kernels (``pad8=False``, what the
    step ran before the shifted path), the shifted kernels (``pad8=True``), ``reference``, and the element
    kernels followed by the channel ``F.pad`` the convolution adds - the pair the shifted path replaces."""
    import torch
    import torch.nn.functional as F

    from katib_amd.ops.enas_concat import reference, relu_pad_concat

    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(1)
    variants = {"element": lambda xs: relu_pad_concat(xs, True),
                "shifted": lambda xs: relu_pad_concat(xs, True, pad8=True),
                "reference": lambda xs: reference(xs, True),
                "element+pad": lambda xs: F.pad(relu_pad_concat(xs, True),
                                                (0, 0, 0, 0, 0, -sum(x.shape[1] for x in xs) % 8))}
    graphs, nbytes, keep = {}, {}, []
    for lname, srcs in IMAGE_LAYERS.items():
        xs = [torch.randn(B, c, h, h, device=dev, generator=gen).to(torch.bfloat16).contiguous(
            memory_format=torch.channels_last).requires_grad_(c != 3) for c, h in srcs]
        wanted = [x for x in xs if x.requires_grad]
        m, Ct = max(h for _, h in srcs), sum(c for c, _ in srcs)
        Cs = (Ct + 7) // 8 * 8
        g8 = torch.randn(B, m, m, Cs, device=dev, generator=gen).to(torch.bfloat16)
        # what the convolution hands back: all Cs channels to a padded input, the [..., :Ct] slice otherwise
        gs = {True: g8.permute(0, 3, 1, 2), False: g8[..., :Ct].permute(0, 3, 1, 2)}
        keep.append((xs, g8))
        # sources read once, the Ct channels written once; the gradients of the wanted sources likewise
        nbytes[lname] = (2 * (sum(x.numel() for x in xs) + B * m * m * Ct),
                         2 * (2 * sum(x.numel() for x in wanted) + B * m * m * Ct))
        with torch.no_grad():  # no autograd graph of the sources may outlive this line: a captured backward
            want = reference(xs, True, pad8=True)  # would meet their gradient accumulators' stream
        for vname, fn in variants.items():
            with torch.no_grad():
                c_out = fn(xs).shape[1]
                assert torch.equal(fn(xs), want[:, :c_out]) and c_out in (Ct, Cs)
            g = gs[c_out == Cs]
            for bwd in (False, True):
                def run(fn=fn, xs=xs, wanted=wanted, g=g, bwd=bwd):
                    if bwd:
                        torch.autograd.grad(fn(xs), wanted, g)
                    else:
                        with torch.no_grad():
                            fn(xs)
                for _ in range(3):
                    run()
                torch.cuda.synchronize()
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr):
                    for _ in range(launches):
                        run()
                gr.replay()
                graphs[(lname, vname, "fwd+bwd" if bwd else "fwd")] = gr
    torch.cuda.synchronize()
    times = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, gr in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            gr.replay()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / launches)
    for lname in IMAGE_LAYERS:
        fwd, bwd = {}, {}
        for vname in variants:
            sf, sb = _stats(times[(lname, vname, "fwd")]), _stats(times[(lname, vname, "fwd+bwd")])
            fwd[vname], bwd[vname] = sf["median"], round(sb["median"] - sf["median"], 4)
            print(json.dumps({"op": lname, "path": vname, "batch": B, "fwd_us": sf, "fwd+bwd_us": sb,
                              "fwd_least_GBps": round(nbytes[lname][0] / (sf["median"] * 1e-6) / 1e9, 1),
                              "bwd_least_GBps": round(nbytes[lname][1] / (max(bwd[vname], 1e-3) * 1e-6) / 1e9, 1)}),
                  flush=True)
        print(json.dumps({"op": lname, "fwd_us": fwd, "bwd_us": bwd,
                          "shifted/element": [round(fwd["shifted"] / fwd["element"], 3),
                                              round(bwd["shifted"] / bwd["element"], 3)],
                          "shifted/element+pad": [round(fwd["shifted"] / fwd["element+pad"], 3),
                                                  round(bwd["shifted"] / bwd["element+pad"], 3)]}), flush=True)


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
    image_second(a.batch, a.launches, a.rounds)


if __name__ == "__main__":
    main()
