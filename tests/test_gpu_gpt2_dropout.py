"""Dropout kernels of the GPT-2 trial (csrc/hip/transformer.hip) against the torch oracle of the
same Philox4x32-10 contract (ops/transformer.py): the mask bit for bit, the fused LayerNorm forward /
backward, the in-place fp32 kernel, a replayed graph drawing a fresh mask per step, a whole flat-model
step and the graph-captured trial. Tolerances are those of tests/test_gpu_transformer.py."""
import math

import pytest
import torch

import gpt2_kernel_oracle as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
# not a multiple of the forward's 4 rows per workgroup; below the backward's row stride of 336, so a wave's
# second row and second iteration never run here (tests/test_gpu_gpt2_kernels.py has M = 1029 and 2051)
M = 333
SHAPES = [256, 768, 1024, 2048]
SEED = (3 << 32) | 77  # both key words in use


def _rel(a, b):
    a, b = a.detach().float(), b.detach().float()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-6))


@pytest.fixture(scope="module")
def ops():
    from katib_amd.ops.transformer import HipOps, TorchOps

    return HipOps(), TorchOps()


def _gen(seed=3):
    return torch.Generator(device=DEV).manual_seed(seed)


def _drop(p, site, step):
    from katib_amd.ops.transformer import Drop

    return Drop(p, site, SEED, torch.full((1,), float(step), device=DEV))


_masks = {}


def _oracle_mask(D, p, site, step):
    """The torch oracle's keep mask, computed once per case and shared (never modified)."""
    from katib_amd.ops.transformer import dropout_mask

    key = (D, p, site, step)
    if key not in _masks:
        _masks[key] = dropout_mask(M, D, p, site, SEED, step, DEV)
    return _masks[key]


@pytest.mark.parametrize("site,step", [(0, 0), (5, 3)])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("D", SHAPES)
def test_mask_parity(ops, D, p, site, step):
    hip, _ = ops
    got = hip.dropout_mask(M, D, _drop(p, site, step))
    want = _oracle_mask(D, p, site, step)
    assert got.dtype == torch.bool and torch.equal(got, want)
    kept = float(want.float().mean())
    assert abs(kept - (1 - p)) < 5 * math.sqrt(p * (1 - p) / want.numel())  # and it is a p-mask at all


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("D", SHAPES)
def test_layernorm_fwd_bwd_drop(ops, D, p):
    hip, ref = ops
    g = _gen()
    site, step = 5, 3
    drop = _drop(p, site, step)
    keep = _oracle_mask(D, p, site, step)
    x = torch.randn(M, D, device=DEV, generator=g) * 2 + 0.5
    r = torch.randn(M, D, device=DEV, generator=g).to(torch.bfloat16)
    gamma = (1 + 0.1 * torch.randn(D, device=DEV, generator=g)).to(torch.bfloat16)
    beta = (0.1 * torch.randn(D, device=DEV, generator=g)).to(torch.bfloat16)
    xh, yh, mh, rh = hip.ln_fwd(x, r, gamma, beta, drop=drop)
    xr, yr, mr, rr = ref.ln_fwd(x, r, gamma, beta, drop=drop)
    assert _rel(xh, xr) < 1e-6 and _rel(mh, mr) < 1e-5 and _rel(rh, rr) < 1e-4
    assert _rel(yh, yr) < 1e-2
    assert torch.equal(xh[~keep], x[~keep])  # a dropped element leaves the residual stream untouched
    assert not torch.equal(xh[keep], x[keep])
    dy = torch.randn(M, D, device=DEV, generator=g).to(torch.bfloat16)
    G0 = torch.randn(M, D, device=DEV, generator=g)
    outs = []
    for o in (hip, ref):
        G = G0.clone()
        dr = torch.full((M, D), 7.0, device=DEV, dtype=torch.bfloat16)
        dg = torch.empty(D, device=DEV, dtype=torch.bfloat16)
        db = torch.empty_like(dg)
        dbias = torch.empty_like(dg)
        o.ln_bwd(dy, xr, mr, rr, gamma, G, dr, dg, db, dbias=dbias, drop=drop)
        outs.append((G, dr, dg, db, dbias))
    (Gh, drh, dgh, dbh, dbiash), (Gr, drr, dgr, dbr, dbiasr) = outs
    assert _rel(Gh, Gr) < 1e-4
    assert float(drh[~keep].abs().max()) == 0.0
    assert _rel(drh, drr) < 1e-2
    assert _rel(dgh, dgr) < 1e-2 and _rel(dbh, dbr) < 1e-2 and _rel(dbiash, dbiasr) < 1e-2
    # G itself is the unmasked residual-stream gradient: the same as without dropout
    G = G0.clone()
    hip.ln_bwd(dy, xr, mr, rr, gamma, G, torch.empty_like(drh), dg, db)
    assert _rel(Gh, G) < 1e-6


@pytest.mark.parametrize("D", [256, 772])
def test_dropout_f32(ops, D):
    from katib_amd.ops.transformer import dropout_mask

    hip, ref = ops
    drop = _drop(0.3, 24, 9)
    x = torch.randn(M, D, device=DEV, generator=_gen())
    got, want = hip.dropout_(x.clone(), drop), ref.dropout_(x.clone(), drop)
    keep = dropout_mask(M, D, 0.3, 24, SEED, 9, DEV)
    assert float(got[~keep].abs().max()) == 0.0 and bool((got[keep] != 0).all())
    assert _rel(got, want) < 1e-6
    assert hip.dropout_(x, None) is x and hip.dropout_(x, drop._replace(p=0.0)) is x  # no launch at all


def test_graph_replay_draws_a_fresh_mask(ops):
    """The kernels read the step counter from device memory: one captured ln_fwd replayed at steps 1
    and 2 gives each step's own mask (a step baked in at capture time gives the same one twice)."""
    from katib_amd.ops.transformer import Drop, dropout_mask

    hip, _ = ops
    D, p, site = 768, 0.5, 2
    g = _gen()
    x = torch.randn(M, D, device=DEV, generator=g)
    r = (torch.rand(M, D, device=DEV, generator=g) + 0.5).to(torch.bfloat16)  # never 0: xo == x only where dropped
    gamma = torch.ones(D, device=DEV, dtype=torch.bfloat16)
    beta = torch.zeros(D, device=DEV, dtype=torch.bfloat16)
    step = torch.zeros(1, device=DEV)
    drop = Drop(p, site, SEED, step)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        hip.ln_fwd(x, r, gamma, beta, drop=drop)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        xo = hip.ln_fwd(x, r, gamma, beta, drop=drop)[0]
    zero = []
    for k in (1, 2):
        step.fill_(float(k))
        graph.replay()
        torch.cuda.synchronize()
        zero.append(xo == x)
        assert torch.equal(zero[-1], ~dropout_mask(M, D, p, site, SEED, k, DEV)), k
    assert not torch.equal(zero[0], zero[1])


def _cfg(dropout=0.0):
    from katib_amd.workloads.gpt2_pbt import GPTConfig

    return GPTConfig(vocab=1000, ctx=128, n_layer=2, n_head=4, d=256, dropout=dropout)


def test_flat_gpt_step_dropout_hip_vs_torch(ops):
    from katib_amd.models.gpt2 import GPT2Flat

    hip, ref = ops
    cfg = _cfg(0.2)
    g = _gen()
    idx = torch.randint(0, cfg.vocab, (2, 128), device=DEV, generator=g)
    tgt = torch.randint(0, cfg.vocab, (2, 128), device=DEV, generator=g)
    mh = GPT2Flat(cfg, DEV, hip, seed=5)
    mr = GPT2Flat(cfg, DEV, ref, seed=5)
    m0 = GPT2Flat(_cfg(0.0), DEV, hip, seed=5)
    for m in (mh, mr, m0):
        m.step_t.fill_(2.0)
    lh = mh.forward_backward(idx, tgt)
    lr = mr.forward_backward(idx, tgt)
    l0 = m0.forward_backward(idx, tgt)
    assert abs(float(lh) - float(lr)) < 2e-2 * abs(float(lr))
    for n in ("wte.weight", "blocks.0.qkv.weight", "blocks.1.fc2.weight", "blocks.0.ln1.weight", "wpe.weight"):
        assert _rel(mh.g[n], mr.g[n]) < 6e-2, (n, _rel(mh.g[n], mr.g[n]))
    assert _rel(mh.g["blocks.1.fc2.weight"], m0.g["blocks.1.fc2.weight"]) > 6e-2  # dropout did act
    assert float(l0) != float(lh)
    # the update itself, row by row, against AdamW in fp64 on the gradient each model computed (see
    # tests/test_gpu_transformer.py::test_flat_gpt_step_hip_vs_torch)
    uh, ur = O.StepUpdate(mh), O.StepUpdate(mr)
    mh.optimizer_step()
    mr.optimizer_step()
    uh.check("flat step update hip")
    ur.check("flat step update torch")
    assert _rel(mh.p32, mr.p32) < 1e-3


def test_gpt2_trial_dropout_captured_vs_eager():
    """The graph-captured trial with dropout follows the eager one: same mask stream (the step counter
    is read on the device), so the validation losses agree within the tolerance the project uses
    between its two implementations."""
    from katib_amd.workloads import gpt2_pbt

    gpt2_pbt.PRESETS["gpu-test"] = _cfg()
    common = ["--model", "gpu-test", "--batch-size", "8", "--lr", "3e-3", "--num-tokens", "200000", "--p2p", "0",
              "--steps", "40", "--impl", "flat", "--dropout", "0.1"]
    v_cap = gpt2_pbt.main(common + ["--capture", "1"])
    v_eag = gpt2_pbt.main(common + ["--capture", "0"])
    assert math.isfinite(v_cap) and math.isfinite(v_eag)
    assert abs(v_cap - v_eag) < 0.15, (v_cap, v_eag)
