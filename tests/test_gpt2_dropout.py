"""Dropout of the GPT-2 PBT member on the CPU: the Philox4x32-10 contract shared by the HIP kernels and
the torch oracle (ops/transformer.py), the flat model's hand-written backward with dropout against
autograd through the same masks, the train / eval split, the trial's --dropout flag and the PBT
example that tunes it."""
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


KAT = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((M32,) * 4, (M32,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
        "d16cfe09 94fdcceb 5001e420 24126ea1"),
       ((5, 0, 3, 7), (0x4D2, 0), "d08ef48a c5c2f6bf 7a9cc398 2aabcf6f")]  # (q, 0, site, step), seed 1234


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    from katib_amd.ops.transformer import philox4x32

    assert " ".join("%08x" % int(w) for w in philox4x32(ctr, key)) == want
    assert " ".join("%08x" % w for w in _philox_scalar(ctr, key)) == want
    # tensor counters broadcast: the same words from a batched call
    words = philox4x32(tuple(torch.tensor([c, c]) for c in ctr), key)
    assert all(int(w[1]) == int(want.split()[i], 16) for i, w in enumerate(words))


def test_dropout_mask_contract():
    from katib_amd.ops.transformer import dropout_mask, dropout_scale, dropout_threshold

    m = dropout_mask(64, 256, 0.1, site=0, seed=0, step=1)
    assert m.shape == (64, 256) and m.dtype == torch.bool
    assert int(m.sum()) == 14800  # of 16384, computed from the contract
    assert torch.equal(m, dropout_mask(64, 256, 0.1, site=0, seed=0, step=1))
    assert torch.equal(m, dropout_mask(64, 256, 0.1, site=0, seed=0, step=torch.tensor([1.0])))  # device counter
    assert not torch.equal(m, dropout_mask(64, 256, 0.1, site=0, seed=0, step=2))
    assert not torch.equal(m, dropout_mask(64, 256, 0.1, site=1, seed=0, step=1))
    assert not torch.equal(m, dropout_mask(64, 256, 0.1, site=0, seed=1, step=1))
    # element e = row * D + col: word e & 3 of the call with counter (e >> 2, 0, site, step)
    seed, site, step, D = (7 << 32) | 1234, 5, 3, 768
    thr = dropout_threshold(0.3)
    assert thr == round(0.3 * 2 ** 32)
    m = dropout_mask(9, D, 0.3, site=site, seed=seed, step=step)
    for row, col in [(0, 0), (0, 1), (0, 2), (0, 3), (0, 4), (1, 0), (3, 255), (3, 256), (4, 513), (7, 767), (8, 6),
                     (8, 767)]:
        e = row * D + col
        words = _philox_scalar((e >> 2, 0, site, step), (seed & M32, seed >> 32))
        assert bool(m[row, col]) == (words[e & 3] >= thr), (row, col)
    assert dropout_threshold(0.0) == 0 and dropout_threshold(0.5) == 1 << 31
    assert dropout_scale(0.5) == 2.0 and abs(dropout_scale(0.1) - 1 / 0.9) < 1e-6
    for bad in (-0.1, 0.95, 1.0, float("nan")):
        with pytest.raises(ValueError):
            dropout_threshold(bad)


def _cfg(dropout):
    from katib_amd.workloads.gpt2_pbt import GPTConfig

    return GPTConfig(vocab=100, ctx=32, n_layer=2, n_head=2, d=128, dropout=dropout)


def _module_forward_with_masks(ref, idx, p, seed, step):
    """The nn.Module GPT's forward as a function of its parameters, with the flat model's dropout
    masks (site 2 i: proj of block i, 2 i + 1: fc2 of block i, 2 n_layer: the embedding sum)."""
    from katib_amd.ops.transformer import dropout_mask, dropout_scale

    B, T = idx.shape
    D, L = ref.c.d, ref.c.n_layer
    scale = dropout_scale(p)

    def drop(t, site):
        keep = dropout_mask(B * T, D, p, site=site, seed=seed, step=step).view(B, T, D)
        return torch.where(keep, t * scale, torch.zeros_like(t))

    x = drop(ref.wte(idx) + ref.wpe(torch.arange(T)), 2 * L)
    for i, b in enumerate(ref.blocks):
        q, k, v = b.qkv(b.ln1(x)).split(D, dim=2)
        q, k, v = (t.view(B, T, b.h, D // b.h).transpose(1, 2) for t in (q, k, v))
        a = F.scaled_dot_product_attention(q, k, v, is_causal=True)
        x = x + drop(b.proj(a.transpose(1, 2).reshape(B, T, D)), 2 * i)
        x = x + drop(b.fc2(F.gelu(b.fc(b.ln2(x)), approximate="tanh")), 2 * i + 1)
    return F.linear(ref.ln_f(x), ref.wte.weight)


@pytest.mark.parametrize("step", [0, 3])
def test_flat_gpt_dropout_matches_autograd(step):
    """Tolerances of test_flat_gpt_matches_autograd (tests/test_gpt2_flat.py)."""
    from katib_amd.models.gpt2 import GPT2Flat
    from katib_amd.ops.transformer import TorchOps
    from katib_amd.workloads.gpt2_pbt import GPT

    torch.manual_seed(0)
    cfg = _cfg(0.25)
    ref = GPT(_cfg(0.0))  # its own F.dropout stays off: the masks come from dropout_mask
    flat = GPT2Flat(cfg, "cpu", TorchOps(), dtype=torch.float32, seed=11)
    flat.load_state_dict(ref.state_dict())
    flat.step_t.fill_(float(step))
    idx = torch.randint(0, 100, (3, 32))
    tgt = torch.randint(0, 100, (3, 32))
    loss_ref = F.cross_entropy(_module_forward_with_masks(ref, idx, 0.25, 11, step).view(-1, 100), tgt.view(-1))
    loss_ref.backward()
    loss = flat.forward_backward(idx, tgt)
    assert abs(float(loss) - float(loss_ref.detach())) < 1e-5
    for n, p in ref.named_parameters():
        gf = flat.g[n][:p.shape[0]]
        assert float((gf - p.grad).abs().max()) <= 1e-4 * float(p.grad.abs().max()) + 1e-9, n
    # and the masks matter: the dropout-free loss is a different number
    loss_plain = F.cross_entropy(ref(idx).view(-1, 100), tgt.view(-1))
    assert abs(float(loss_plain) - float(loss_ref)) > 1e-4


def test_eval_forward_ignores_dropout():
    from katib_amd.models.gpt2 import GPT2Flat
    from katib_amd.ops.transformer import TorchOps

    a = GPT2Flat(_cfg(0.25), "cpu", TorchOps(), dtype=torch.float32, seed=3)
    b = GPT2Flat(_cfg(0.0), "cpu", TorchOps(), dtype=torch.float32, seed=3)
    idx = torch.randint(0, 100, (2, 32), generator=torch.Generator().manual_seed(1))
    assert torch.equal(a.forward(idx), b.forward(idx))
    assert not torch.equal(a.forward(idx, train=True), b.forward(idx, train=True))
    with pytest.raises(ValueError):
        GPT2Flat(_cfg(0.95), "cpu", TorchOps(), dtype=torch.float32)


def test_zero_dropout_changes_nothing():
    """dropout = 0 takes the calls the model made before it had dropout: a config object without the
    field at all (how the model was built then) gives bit-identical gradients and update."""
    from types import SimpleNamespace

    from katib_amd.models.gpt2 import GPT2Flat
    from katib_amd.ops.transformer import TorchOps

    class CountingOps(TorchOps):
        def __init__(self):
            super().__init__()
            self.drops = []

        def ln_fwd(self, *a, drop=None):
            self.drops.append(drop)
            return super().ln_fwd(*a, drop=drop)

        def ln_bwd(self, *a, drop=None, **kw):
            self.drops.append(drop)
            return super().ln_bwd(*a, drop=drop, **kw)

        def dropout_(self, x, drop):
            self.drops.append(drop)
            return super().dropout_(x, drop)

    old_cfg = SimpleNamespace(vocab=100, ctx=32, n_layer=2, n_head=2, d=128)
    g = torch.Generator().manual_seed(2)
    idx = torch.randint(0, 100, (3, 32), generator=g)
    tgt = torch.randint(0, 100, (3, 32), generator=g)
    ops = CountingOps()
    a = GPT2Flat(_cfg(0.0), "cpu", ops, dtype=torch.float32, seed=4)
    b = GPT2Flat(old_cfg, "cpu", TorchOps(), dtype=torch.float32, seed=4)
    la, lb = a.forward_backward(idx, tgt), b.forward_backward(idx, tgt)
    assert torch.equal(la, lb) and torch.equal(a.g16, b.g16)
    assert ops.drops and all(d is None for d in ops.drops)  # no site is ever handed to the ops
    a.optimizer_step()
    b.optimizer_step()
    assert torch.equal(a.p32, b.p32)


def test_gpt2_trial_dropout_cpu(tmp_path):
    from katib_amd.workloads import gpt2_pbt

    ck = str(tmp_path / "ck")
    common = ["--model", "tiny", "--batch-size", "4", "--num-tokens", "50000", "--checkpoint-dir", ck, "--dropout",
              "0.1"]
    v1 = gpt2_pbt.main(common + ["--steps", "6", "--impl", "flat"])
    v2 = gpt2_pbt.main(common + ["--steps", "3", "--impl", "module"])
    v3 = gpt2_pbt.main(common + ["--steps", "3", "--impl", "flat"])
    assert all(math.isfinite(v) for v in (v1, v2, v3))
    st = torch.load(tmp_path / "ck" / "optim.pt", weights_only=True)
    assert int(st["step"]) == 12
    for bad in ("1.0", "-0.1"):
        with pytest.raises(SystemExit) as e:
            gpt2_pbt.main(["--model", "tiny", "--dropout", bad])
        assert e.value.code != 0
    assert gpt2_pbt.PRESETS["tiny"].dropout == 0.0  # the preset itself is not modified


def test_module_gpt_dropout_train_only():
    from katib_amd.workloads.gpt2_pbt import GPT

    torch.manual_seed(0)
    m, m0 = GPT(_cfg(0.25)), GPT(_cfg(0.0))
    assert list(m.state_dict()) == list(m0.state_dict())
    m0.load_state_dict(m.state_dict())
    idx = torch.randint(0, 100, (2, 32))
    assert not torch.equal(m(idx), m0(idx))
    m.eval()
    assert torch.equal(m(idx), m0(idx))


def test_gpt2_pbt_dropout_example(manager):
    e = load_experiment(os.path.join(EX, "pbt", "pbt-gpt2-small-dropout.yaml"))
    names = {p.name: p for p in e.spec.parameters}
    assert set(names) == {"lr", "weight_decay", "dropout"}
    fs = names["dropout"].feasible_space
    assert (float(fs.min), float(fs.max), float(fs.step)) == (0.0, 0.3, 0.05)
    spec = e.spec.trial_template.trial_spec["spec"]
    assert "--dropout=${trialParameters.dropout}" in spec["args"]
    spec["gpus"] = 0
    spec["args"] = list(spec["args"]) + ["--model=tiny", "--steps=5", "--num-tokens=20000", "--batch-size=4",
                                         "--capture=0"]
    # the pbt algorithm refuses a population under 5 (as the reference's service does), so the shrunk
    # experiment keeps test_gpt2_pbt_example's sizes: population 5, 12 trials
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
    drops = {a.value for t in trials for a in t.spec.parameter_assignments if a.name == "dropout"}
    assert len(drops) >= 2, drops
    assert all(0.0 <= float(v) <= 0.3 + 1e-9 for v in drops), drops  # grid points are sums of the step
