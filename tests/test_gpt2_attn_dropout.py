"""Attention-probability dropout of the GPT-2 PBT member on the CPU: the 8-bit, 4 x 4-tile Philox
contract shared by the flash attention kernels and the torch oracle (ops/transformer.py), the flat
model's hand-written backward against autograd through the same masks, the train / eval split, the
trial's --attn-dropout flag and the PBT example that tunes it."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

from katib_amd.api.conditions import ExperimentConditions as EC
from katib_amd.api.yaml_io import load_experiment

EX = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
M32 = 0xFFFFFFFF


def _philox_scalar(ctr, key):
    """Philox4x32-10 on Python ints (Random123's reference algorithm)."""
    c, k = list(ctr), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & M32, (p0 >> 32) ^ c[3] ^ k[1], p0 & M32]
        k = [(k[0] + 0x9E3779B9) & M32, (k[1] + 0xBB67AE85) & M32]
    return c


def _keep_scalar(bh, q, k, T, thr8, site, seed, step):
    """One element of the contract, re-derived in plain Python."""
    blk = (bh * (T // 4) + (q >> 2)) * (T // 4) + (k >> 2)
    w = _philox_scalar((blk & M32, blk >> 32, site, step), (seed & M32, seed >> 32))
    return ((w[q & 3] >> (8 * (k & 3))) & 0xFF) >= thr8


@pytest.mark.parametrize("T", [32, 128])
def test_attn_dropout_mask_contract(T):
    from katib_amd.ops.transformer import attn_dropout_mask, attn_dropout_threshold

    B, H, p = 2, 3, 0.3
    seed, site, step = (7 << 32) | 1234, 9, 3
    thr8 = attn_dropout_threshold(p)
    assert thr8 == 77  # floor(0.3 * 256 + 0.5)
    m = attn_dropout_mask(B, H, T, p, site=site, seed=seed, step=step)
    assert m.shape == (B, H, T, T) and m.dtype == torch.bool
    picks = [(bh, q, k) for bh in (0, 1, 5) for q in (0, 3, 4, 7, T - 4, T - 1) for k in (0, 3, T - 5, T - 1)]
    picks += [(2, 17, 18), (4, 21, 6), (3, 10, 13), (0, 1, 2), (5, T - 2, 1)]
    for bh, q, k in picks:
        assert bool(m[bh // H, bh % H, q, k]) == _keep_scalar(bh, q, k, T, thr8, site, seed, step), (bh, q, k)


def test_attn_dropout_mask_properties():
    from katib_amd.ops.transformer import (attn_dropout_mask, attn_dropout_scale, attn_dropout_threshold,
                                           TorchOps, Drop)

    B, H, T, p = 2, 2, 128, 0.1
    m = attn_dropout_mask(B, H, T, p, site=5, seed=0, step=1)
    assert torch.equal(m, attn_dropout_mask(B, H, T, p, site=5, seed=0, step=1))
    assert torch.equal(m, attn_dropout_mask(B, H, T, p, site=5, seed=0, step=torch.tensor([1.0])))  # device counter
    assert not torch.equal(m, attn_dropout_mask(B, H, T, p, site=6, seed=0, step=1))
    assert not torch.equal(m, attn_dropout_mask(B, H, T, p, site=5, seed=0, step=2))
    assert not torch.equal(m, attn_dropout_mask(B, H, T, p, site=5, seed=1, step=1))
    assert not torch.equal(m, attn_dropout_mask(B, H, T, p, site=5, seed=1 << 32, step=1))
    # the realised rate is thr8 / 256, and the scale is unbiased for it
    thr8 = attn_dropout_threshold(p)
    assert thr8 == 26 and abs(attn_dropout_scale(p) - 256 / 230) < 1e-6
    assert attn_dropout_threshold(0.5) == 128 and attn_dropout_scale(0.5) == 2.0
    assert attn_dropout_threshold(0.9) == 230
    tri = torch.ones(T, T, dtype=torch.bool).tril()
    kept = m[:, :, tri].float()
    pr = thr8 / 256.0
    assert abs(float(kept.mean()) - (1 - pr)) < 5 * math.sqrt(pr * (1 - pr) / kept.numel())
    # below 1/512 the site is inactive: thr8 = 0, every element kept, the ops take the p = 0 path
    assert attn_dropout_threshold(0.001) == 0 and attn_dropout_scale(0.001) == 1.0
    assert bool(attn_dropout_mask(1, 1, 8, 0.001, 0, 0, 0).all())
    qkv = torch.randn(2 * 8, 3 * 64)
    ops = TorchOps()
    o0, l0 = ops.attn_fwd(qkv, 2, 8, 1)
    o1, l1 = ops.attn_fwd(qkv, 2, 8, 1, drop=Drop(0.001, 3, 0, 0))
    assert torch.equal(o0, o1) and torch.equal(l0, l1)
    for bad in (0.95, -0.1, float("nan")):
        with pytest.raises(ValueError):
            attn_dropout_threshold(bad)
        with pytest.raises(ValueError):
            attn_dropout_mask(1, 1, 8, bad, 0, 0, 0)
    with pytest.raises(ValueError):
        attn_dropout_mask(1, 1, 30, 0.1, 0, 0, 0)  # T % 4 != 0


def test_torch_ops_attention_dropout():
    """The oracle itself: O = (keep * scale * P) V, lse untouched, a fully dropped row gives O = 0
    and finite gradients."""
    from katib_amd.ops.transformer import Drop, TorchOps, attn_dropout_mask, attn_dropout_scale

    B, T, H, p = 2, 16, 2, 0.5
    ops = TorchOps()
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn(B * T, 3 * H * 64, generator=g)
    dout = torch.randn(B * T, H * 64, generator=g)
    # a step at which some (b, h) drops its q = 0 row's only key
    step = next(s for s in range(64) if not bool(attn_dropout_mask(B, H, T, p, 4, 0, s)[:, :, 0, 0].all()))
    drop = Drop(p, 4, 0, step)
    keep = attn_dropout_mask(B, H, T, p, 4, 0, step)
    o, lse = ops.attn_fwd(qkv, B, T, H, drop=drop)
    o0, lse0 = ops.attn_fwd(qkv, B, T, H)
    assert torch.equal(lse, lse0) and not torch.equal(o, o0)
    q, k, v = qkv.view(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) / 8.0
    s = s.masked_fill(torch.ones(T, T, dtype=torch.bool).triu(1), float("-inf"))
    want = (torch.softmax(s, -1) * keep * attn_dropout_scale(p)) @ v
    assert torch.allclose(o.view(B, T, H, 64).permute(0, 2, 1, 3), want, atol=1e-6)
    b, h = (~keep[:, :, 0, 0]).nonzero()[0].tolist()
    assert float(o.view(B, T, H, 64)[b, 0, h].abs().max()) == 0.0
    dqkv = ops.attn_bwd(qkv, o, dout, lse, B, T, H, drop=drop)
    assert bool(torch.isfinite(dqkv).all())
    assert not torch.equal(dqkv, ops.attn_bwd(qkv, o0, dout, lse, B, T, H))


def _cfg(dropout=0.0, attn_dropout=0.0):
    from katib_amd.workloads.gpt2_pbt import GPTConfig

    return GPTConfig(vocab=100, ctx=32, n_layer=2, n_head=2, d=128, dropout=dropout, attn_dropout=attn_dropout)


def _module_forward_with_masks(ref, idx, p, pa, seed, step):
    """The nn.Module GPT's forward as a function of its parameters, with the flat model's dropout
    masks: sites 2 i / 2 i + 1 / 2 n_layer as in tests/test_gpt2_dropout.py (p), and site
    2 n_layer + 1 + i on the attention probabilities of block i (pa)."""
    from katib_amd.ops.transformer import attn_dropout_mask, attn_dropout_scale, dropout_mask, dropout_scale

    B, T = idx.shape
    D, L = ref.c.d, ref.c.n_layer

    def drop(t, site):
        if p == 0:
            return t
        keep = dropout_mask(B * T, D, p, site=site, seed=seed, step=step).view(B, T, D)
        return torch.where(keep, t * dropout_scale(p), torch.zeros_like(t))

    causal = torch.ones(T, T, dtype=torch.bool).triu(1)
    x = drop(ref.wte(idx) + ref.wpe(torch.arange(T)), 2 * L)
    for i, b in enumerate(ref.blocks):
        q, k, v = b.qkv(b.ln1(x)).split(D, dim=2)
        q, k, v = (t.view(B, T, b.h, D // b.h).transpose(1, 2) for t in (q, k, v))
        s = (q @ k.transpose(-1, -2)) / math.sqrt(D // b.h)
        pr = torch.softmax(s.masked_fill(causal, float("-inf")), -1)
        keep = attn_dropout_mask(B, b.h, T, pa, site=2 * L + 1 + i, seed=seed, step=step)
        a = torch.where(keep, pr * attn_dropout_scale(pa), torch.zeros_like(pr)) @ v
        x = x + drop(b.proj(a.transpose(1, 2).reshape(B, T, D)), 2 * i)
        x = x + drop(b.fc2(F.gelu(b.fc(b.ln2(x)), approximate="tanh")), 2 * i + 1)
    return F.linear(ref.ln_f(x), ref.wte.weight)


@pytest.mark.parametrize("p,pa,step", [(0.0, 0.25, 0), (0.0, 0.25, 3), (0.25, 0.2, 3)])
def test_flat_gpt_attn_dropout_matches_autograd(p, pa, step):
    """Tolerances of test_flat_gpt_dropout_matches_autograd (tests/test_gpt2_dropout.py)."""
    from katib_amd.models.gpt2 import GPT2Flat
    from katib_amd.ops.transformer import TorchOps
    from katib_amd.workloads.gpt2_pbt import GPT

    torch.manual_seed(0)
    ref = GPT(_cfg())  # its own dropout stays off: the masks come from the oracle functions
    flat = GPT2Flat(_cfg(p, pa), "cpu", TorchOps(), dtype=torch.float32, seed=11)
    flat.load_state_dict(ref.state_dict())
    flat.step_t.fill_(float(step))
    idx = torch.randint(0, 100, (3, 32))
    tgt = torch.randint(0, 100, (3, 32))
    loss_ref = F.cross_entropy(_module_forward_with_masks(ref, idx, p, pa, 11, step).view(-1, 100), tgt.view(-1))
    loss_ref.backward()
    loss = flat.forward_backward(idx, tgt)
    assert abs(float(loss) - float(loss_ref.detach())) < 1e-5
    for n, q in ref.named_parameters():
        gf = flat.g[n][:q.shape[0]]
        assert float((gf - q.grad).abs().max()) <= 1e-4 * float(q.grad.abs().max()) + 1e-9, n
    # and the attention masks matter: without them (residual dropout alone) the loss is a different number
    loss_plain = F.cross_entropy(_module_forward_with_masks(ref, idx, p, 0.0, 11, step).view(-1, 100), tgt.view(-1))
    assert abs(float(loss_plain.detach()) - float(loss_ref.detach())) > 1e-4


def test_eval_forward_ignores_attn_dropout():
    from katib_amd.models.gpt2 import GPT2Flat
    from katib_amd.ops.transformer import TorchOps

    a = GPT2Flat(_cfg(0.0, 0.25), "cpu", TorchOps(), dtype=torch.float32, seed=3)
    b = GPT2Flat(_cfg(), "cpu", TorchOps(), dtype=torch.float32, seed=3)
    idx = torch.randint(0, 100, (2, 32), generator=torch.Generator().manual_seed(1))
    assert torch.equal(a.forward(idx), b.forward(idx))
    assert not torch.equal(a.forward(idx, train=True), b.forward(idx, train=True))
    for bad in (0.95, float("nan")):
        with pytest.raises(ValueError):
            GPT2Flat(_cfg(0.0, bad), "cpu", TorchOps(), dtype=torch.float32)


class _CountingOps:
    """TorchOps that records what the model hands to the attention calls."""

    def __new__(cls):
        from katib_amd.ops.transformer import TorchOps

        class Counting(TorchOps):
            def __init__(self):
                super().__init__()
                self.attn_kw = []

            def attn_fwd(self, *a, **kw):
                self.attn_kw.append(dict(kw))
                return super().attn_fwd(*a, **kw)

            def attn_bwd(self, *a, **kw):
                self.attn_kw.append(dict(kw))
                return super().attn_bwd(*a, **kw)

        return Counting()


def test_zero_attn_dropout_changes_nothing():
    """attn_dropout = 0 makes the calls the model made before it had the site: a config object
    without the field gives bit-identical gradients and update, with and without residual dropout,
    and the attention ops never see a Drop."""
    from types import SimpleNamespace

    from katib_amd.models.gpt2 import GPT2Flat
    from katib_amd.ops.transformer import TorchOps

    g = torch.Generator().manual_seed(2)
    idx = torch.randint(0, 100, (3, 32), generator=g)
    tgt = torch.randint(0, 100, (3, 32), generator=g)
    for p in (0.0, 0.2):
        old_cfg = SimpleNamespace(vocab=100, ctx=32, n_layer=2, n_head=2, d=128, dropout=p)
        ops = _CountingOps()
        a = GPT2Flat(_cfg(p, 0.0), "cpu", ops, dtype=torch.float32, seed=4)
        b = GPT2Flat(old_cfg, "cpu", TorchOps(), dtype=torch.float32, seed=4)
        la, lb = a.forward_backward(idx, tgt), b.forward_backward(idx, tgt)
        assert torch.equal(la, lb) and torch.equal(a.g16, b.g16)
        assert len(ops.attn_kw) == 4 and all(kw == {} for kw in ops.attn_kw)
        a.optimizer_step()
        b.optimizer_step()
        assert torch.equal(a.p32, b.p32)
    # a p below 1/512 is inactive too, and an active one hands block i's site to both of its calls
    ops = _CountingOps()
    GPT2Flat(_cfg(0.0, 0.001), "cpu", ops, dtype=torch.float32, seed=4).forward_backward(idx, tgt)
    assert all(kw == {} for kw in ops.attn_kw)
    ops = _CountingOps()
    m = GPT2Flat(_cfg(0.0, 0.25), "cpu", ops, dtype=torch.float32, seed=4)
    m.forward_backward(idx, tgt)
    assert [kw["drop"].site for kw in ops.attn_kw] == [5, 6, 6, 5]  # 2 n_layer + 1 + i; backward in reverse
    assert all(kw["drop"].p == 0.25 and kw["drop"].seed == 4 and kw["drop"].step is m.step_t for kw in ops.attn_kw)


def test_gpt2_trial_attn_dropout_cpu(tmp_path):
    from katib_amd.workloads import gpt2_pbt

    ck = str(tmp_path / "ck")
    common = ["--model", "tiny", "--batch-size", "4", "--num-tokens", "50000", "--checkpoint-dir", ck,
              "--attn-dropout", "0.1"]
    v1 = gpt2_pbt.main(common + ["--steps", "6", "--impl", "flat"])
    v2 = gpt2_pbt.main(common + ["--steps", "3", "--impl", "module"])
    v3 = gpt2_pbt.main(common + ["--steps", "3", "--impl", "flat", "--dropout", "0.1"])
    assert all(math.isfinite(v) for v in (v1, v2, v3))
    for bad in ("1.0", "-0.1", "nan"):
        with pytest.raises(SystemExit) as e:
            gpt2_pbt.main(["--model", "tiny", "--attn-dropout", bad])
        assert e.value.code != 0
    assert gpt2_pbt.PRESETS["tiny"].attn_dropout == 0.0 and gpt2_pbt.PRESETS["tiny"].dropout == 0.0


def test_module_gpt_attn_dropout_train_only():
    from katib_amd.workloads.gpt2_pbt import GPT

    torch.manual_seed(0)
    m, m0 = GPT(_cfg(0.0, 0.25)), GPT(_cfg())
    assert list(m.state_dict()) == list(m0.state_dict())
    m0.load_state_dict(m.state_dict())
    idx = torch.randint(0, 100, (2, 32))
    assert not torch.equal(m(idx), m0(idx))
    m.eval()
    assert torch.equal(m(idx), m0(idx))


def test_gpt2_pbt_attn_dropout_example(manager):
    e = load_experiment(os.path.join(EX, "pbt", "pbt-gpt2-small-attn-dropout.yaml"))
    names = {p.name: p for p in e.spec.parameters}
    assert set(names) == {"lr", "dropout", "attn_dropout"}
    fs = names["attn_dropout"].feasible_space
    assert (float(fs.min), float(fs.max), float(fs.step)) == (0.0, 0.3, 0.05)
    spec = e.spec.trial_template.trial_spec["spec"]
    assert "--attn-dropout=${trialParameters.attn_dropout}" in spec["args"]
    assert "--dropout=${trialParameters.dropout}" in spec["args"]
    spec["gpus"] = 0
    spec["args"] = list(spec["args"]) + ["--model=tiny", "--steps=5", "--num-tokens=20000", "--batch-size=4",
                                         "--capture=0"]
    # shrunk as test_gpt2_pbt_dropout_example: population 5 (the algorithm's minimum), 12 trials
    e.spec.max_trial_count, e.spec.parallel_trial_count = 12, 5
    e.spec.max_failed_trial_count = min(e.spec.max_failed_trial_count or 0, 12)
    for s in e.spec.algorithm.algorithm_settings:
        if s.name == "n_population":
            s.value = "5"
    manager.create_experiment(e)
    done = manager.run_until_complete(e.metadata.name, timeout=600)
    trials = manager.list_trials(e.metadata.name)
    failed = [t.status.conditions[-1].message for t in trials if t.status.conditions[-1].type == "Failed"]
    assert not failed, failed
    assert EC.is_succeeded(done), done.status.conditions
    drops = {a.value for t in trials for a in t.spec.parameter_assignments if a.name == "attn_dropout"}
    assert len(drops) >= 2, drops
    assert all(0.0 <= float(v) <= 0.3 + 1e-9 for v in drops), drops
