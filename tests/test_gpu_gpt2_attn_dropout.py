"""Attention-probability dropout inside the flash attention kernels (csrc/hip/transformer.hip,
attn_fwd_k / attn_dq_k / attn_dkdv_k <true>) against the torch oracle of the same 8-bit Philox contract
(ops/transformer.py attn_dropout_mask): the mask bit for bit through the forward's and the dK/dV
kernel's lane layouts, numerical parity of the forward and of dQ / dK / dV, the inactive site, a
replayed graph drawing a fresh mask per step, a whole flat-model step and the graph-captured trial.
Tolerances are those of tests/test_gpu_transformer.py and tests/test_gpu_gpt2_dropout.py."""
import math

import pytest
import torch

import gpt2_kernel_oracle as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
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


def test_exact_mask_through_the_kernels(ops):
    """Q = K = 0 makes P uniform over the allowed keys, so a one-hot V (dO) reads single elements of
    the dropped P out of O (dV): which of them are non-zero is the kernels' keep mask. T = 256 has
    off-diagonal tiles, B * H = 6 is no multiple of 8, and b = 1 exercises bh = b * H + h."""
    from katib_amd.ops.transformer import attn_dropout_mask

    hip, _ = ops
    B, T, H, p, site, step = 2, 256, 3, 0.5, 7, 5
    drop = _drop(p, site, step)
    causal = torch.ones(T, T, dtype=torch.bool, device=DEV).tril()
    want = attn_dropout_mask(B, H, T, p, site, SEED, step, DEV) & causal
    assert 0.45 < float(want[:, :, causal].float().mean()) < 0.55
    got_f = torch.zeros_like(want)
    got_b = torch.zeros_like(want)
    eye = torch.eye(64, device=DEV, dtype=torch.bfloat16)
    for r in range(T // 64):
        onehot = torch.zeros(T, 64, device=DEV, dtype=torch.bfloat16)
        onehot[64 * r:64 * r + 64] = eye  # [k, d] = (k // 64 == r and k % 64 == d)
        qkv = torch.zeros(B, T, 3, H, 64, device=DEV, dtype=torch.bfloat16)
        qkv[:, :, 2] = onehot[None, :, None, :]
        qkv = qkv.view(B * T, 3 * H * 64)
        o, lse = hip.attn_fwd(qkv, B, T, H, drop=drop)
        got_f[:, :, :, 64 * r:64 * r + 64] = o.view(B, T, H, 64).permute(0, 2, 1, 3) != 0  # O[q, d] = Pd[q, 64 r + d]
        dout = onehot[None, :, None, :].expand(B, T, H, 64).reshape(B * T, H * 64).contiguous()
        dqkv = hip.attn_bwd(qkv, o, dout, lse, B, T, H, drop=drop)
        assert bool(torch.isfinite(dqkv.float()).all())
        dv = dqkv.view(B, T, 3, H, 64)[:, :, 2]  # dV[k, d] = Pd[64 r + d, k]
        got_b[:, :, 64 * r:64 * r + 64, :] = dv.permute(0, 2, 3, 1) != 0
    assert torch.equal(got_f, want)
    assert torch.equal(got_b, want)
    # a fully dropped row (q = 0 whose only key is dropped) is an all-zero output row, not a NaN
    assert not bool(want[:, :, 0, 0].all())


# (B, T, H): one query block; several blocks with off-diagonal tiles; an odd number of blocks
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("B,T,H", [(2, 128, 3), (2, 256, 4), (1, 384, 2)])
def test_attention_dropout_parity(ops, B, T, H, p):
    """Forward and dQ / dK / dV against TorchOps, tolerances of test_attention_fwd_bwd."""
    hip, ref = ops
    g = _gen(B * T + H)
    drop = _drop(p, 2 * H + 1, 4)
    qkv = torch.randn(B * T, 3 * H * 64, device=DEV, generator=g).to(torch.bfloat16)
    oh, lh = hip.attn_fwd(qkv, B, T, H, drop=drop)
    orf, lr = ref.attn_fwd(qkv, B, T, H, drop=drop)
    print("fwd rel %.4g" % _rel(oh, orf))
    assert _rel(oh, orf) < 2e-2, _rel(oh, orf)
    assert float((lh - lr).abs().max()) < 1e-2
    assert torch.equal(lh, hip.attn_fwd(qkv, B, T, H)[1])  # lse is that of the undropped softmax
    do = torch.randn(B * T, H * 64, device=DEV, generator=g).to(torch.bfloat16)
    dh = hip.attn_bwd(qkv, oh, do, lh, B, T, H, drop=drop)
    dr = ref.attn_bwd(qkv, orf, do, lr, B, T, H, drop=drop)
    assert bool(torch.isfinite(dh.float()).all())
    d5h, d5r = dh.view(B, T, 3, H, 64), dr.view(B, T, 3, H, 64)
    rels = [_rel(d5h[:, :, part], d5r[:, :, part]) for part in range(3)]
    print("dq dk dv rel %.4g %.4g %.4g" % tuple(rels))
    for part in range(3):
        assert rels[part] < 3e-2, (part, rels)
    # and dropout acted: the dropout-free gradient is far from it
    d0 = hip.attn_bwd(qkv, hip.attn_fwd(qkv, B, T, H)[0], do, lh, B, T, H).view(B, T, 3, H, 64)
    assert _rel(d0[:, :, 2], d5r[:, :, 2]) > 3e-2


def test_inactive_drop_is_a_noop(ops):
    hip, _ = ops
    B, T, H = 2, 128, 3
    g = _gen()
    qkv = torch.randn(B * T, 3 * H * 64, device=DEV, generator=g).to(torch.bfloat16)
    do = torch.randn(B * T, H * 64, device=DEV, generator=g).to(torch.bfloat16)
    o, lse = hip.attn_fwd(qkv, B, T, H)
    d = hip.attn_bwd(qkv, o, do, lse, B, T, H)
    for drop in (None, _drop(0.0, 3, 1), _drop(0.001, 3, 1)):  # 0.001 < 1/512: thr8 = 0
        o2, lse2 = hip.attn_fwd(qkv, B, T, H, drop=drop)
        assert torch.equal(o, o2) and torch.equal(lse, lse2)
        assert torch.equal(d, hip.attn_bwd(qkv, o, do, lse, B, T, H, drop=drop))
    with pytest.raises(ValueError):
        hip.attn_fwd(qkv, B, T, H, drop=_drop(0.95, 3, 1))


def test_graph_replay_draws_a_fresh_mask(ops):
    """The kernels read the step counter from device memory: one captured attn_fwd replayed at steps
    1 and 2 matches the oracle at each step (a step baked in at capture time gives the same twice)."""
    from katib_amd.ops.transformer import Drop

    hip, ref = ops
    B, T, H, p, site = 2, 128, 3, 0.5, 9
    qkv = torch.randn(B * T, 3 * H * 64, device=DEV, generator=_gen()).to(torch.bfloat16)
    step = torch.zeros(1, device=DEV)
    drop = Drop(p, site, SEED, step)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        hip.attn_fwd(qkv, B, T, H, drop=drop)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o = hip.attn_fwd(qkv, B, T, H, drop=drop)[0]
    outs = []
    for k in (1, 2):
        step.fill_(float(k))
        graph.replay()
        torch.cuda.synchronize()
        outs.append(o.clone())
        want = ref.attn_fwd(qkv, B, T, H, drop=Drop(p, site, SEED, k))[0]
        assert _rel(outs[-1], want) < 2e-2, (k, _rel(outs[-1], want))
    assert _rel(outs[0], outs[1]) > 0.1


def _cfg(dropout=0.0, attn_dropout=0.0):
    from katib_amd.workloads.gpt2_pbt import GPTConfig

    return GPTConfig(vocab=1000, ctx=128, n_layer=2, n_head=4, d=256, dropout=dropout, attn_dropout=attn_dropout)


def test_flat_gpt_step_both_dropouts_hip_vs_torch(ops):
    """Config and tolerances of test_flat_gpt_step_dropout_hip_vs_torch, attention dropout added."""
    from katib_amd.models.gpt2 import GPT2Flat

    hip, ref = ops
    cfg = _cfg(0.2, 0.2)
    g = _gen()
    idx = torch.randint(0, cfg.vocab, (2, 128), device=DEV, generator=g)
    tgt = torch.randint(0, cfg.vocab, (2, 128), device=DEV, generator=g)
    mh = GPT2Flat(cfg, DEV, hip, seed=5)
    mr = GPT2Flat(cfg, DEV, ref, seed=5)
    m0 = GPT2Flat(_cfg(0.2, 0.0), DEV, hip, seed=5)
    for m in (mh, mr, m0):
        m.step_t.fill_(2.0)
    lh = mh.forward_backward(idx, tgt)
    lr = mr.forward_backward(idx, tgt)
    l0 = m0.forward_backward(idx, tgt)
    assert abs(float(lh) - float(lr)) < 2e-2 * abs(float(lr))
    for n in ("wte.weight", "blocks.0.qkv.weight", "blocks.1.qkv.weight", "blocks.1.fc2.weight", "blocks.0.ln1.weight",
              "wpe.weight"):
        assert _rel(mh.g[n], mr.g[n]) < 6e-2, (n, _rel(mh.g[n], mr.g[n]))
    assert _rel(mh.g["blocks.1.qkv.weight"], m0.g["blocks.1.qkv.weight"]) > 6e-2  # attention dropout did act
    assert float(l0) != float(lh)
    # the update itself, row by row, against AdamW in fp64 on the gradient each model computed (see
    # tests/test_gpu_transformer.py::test_flat_gpt_step_hip_vs_torch)
    uh, ur = O.StepUpdate(mh), O.StepUpdate(mr)
    mh.optimizer_step()
    mr.optimizer_step()
    uh.check("flat step update hip")
    ur.check("flat step update torch")
    assert _rel(mh.p32, mr.p32) < 1e-3


def test_gpt2_trial_attn_dropout_captured_vs_eager():
    """Bar of test_gpt2_trial_dropout_captured_vs_eager: the captured trial follows the eager one."""
    from katib_amd.workloads import gpt2_pbt

    gpt2_pbt.PRESETS["gpu-test"] = _cfg()
    common = ["--model", "gpu-test", "--batch-size", "8", "--lr", "3e-3", "--num-tokens", "200000", "--p2p", "0",
              "--steps", "40", "--impl", "flat", "--attn-dropout", "0.1"]
    v_cap = gpt2_pbt.main(common + ["--capture", "1"])
    v_eag = gpt2_pbt.main(common + ["--capture", "0"])
    assert math.isfinite(v_cap) and math.isfinite(v_eag)
    assert abs(v_cap - v_eag) < 0.15, (v_cap, v_eag)
