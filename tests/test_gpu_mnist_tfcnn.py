"""The Keras MNIST CNN trial on the fused kernels of csrc/hip/mnist_tfcnn.hip (+ csrc/hip/mlp.hip for fc1 /
fc2, fc1's forward on ``lin_fwd_splitk``): each kernel through its binding against
tests/mnist_tfcnn_oracle.py, ``HipTFCNN`` over three steps through ``state_dict()`` for both optimizers,
eager against a replayed graph, the trial's ``--impl hip`` and the example through the scheduler.

B is the only free size: O.BATCHES = 1, 3 (with a repeated gather index), 17 and 65 (see the oracle file).
``lin_fwd_splitk`` is also run at (3, 16, 8), (17, 72, KS + 8), (65, 128, 2 KS + 8) and the model's
(65, 128, 21632), KS its slab width: one short slab, a slab and a tail with N no multiple of the tile, two
M tiles x two N tiles x three slabs, and the 43 slabs of ``fc1``.

Exact arm. Small-integer / power-of-two operands (O.exact_case), so every sum is exact in fp32 in any
order (tests/test_mnist_tfcnn_oracle.py proves that on the reference): ``z``, the split-K output, ``dz``, the
conv gradients (the momentum buffer after a step from zero momentum) and, with lr = 2^-10, the new master
and shadow are compared with torch.equal.

Generic arm. Gaussian images, ``TFNet``'s initialisation. Every output is held, against the oracle with
fp32 GEMMs, to the larger of 1e-2 relative (max norm) and four times that oracle's own distance from the
oracle with fp64 GEMMs at the same rounding points (the rule of tests/test_gpu_mnist_cnn.py and
tests/test_gpu_mlp_optim.py). Every kernel gets the fp32 oracle's rounded outputs as inputs, so the arms
differ by accumulation alone. Model level: the same rule on state and update of every parameter.

Every test prints the figures it measured (``pytest -s``) before it asserts.
"""
import functools
import glob
import math
import os
import re
import sys

import pytest
import torch

import mnist_tfcnn_oracle as O
from katib_amd.api.conditions import ExperimentConditions as EC
from katib_amd.api.yaml_io import load_experiment
from katib_amd.metricscollector import tfevent
from katib_amd.workloads import mnist_tfcnn
from katib_amd.workloads.common import CapturedStep

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FEAT, HID = mnist_tfcnn.FEAT, mnist_tfcnn.HID


@pytest.fixture(scope="module")
def k():
    from katib_amd.ops.conv import kernels

    return kernels()


def _lr(v):
    return torch.full((1,), v, device=DEV, dtype=F32)


def _zero(*ts):
    return all(float(t.float().abs().max()) == 0.0 for t in ts if t.numel())


def _splitk(k, x, w, b, relu):
    M, N, K = x.shape[0], w.shape[0], w.shape[1]
    part = torch.empty(k.lin_splitk_part_size(M, N, K), device=DEV, dtype=F32)
    y = torch.empty(M, N, device=DEV, dtype=BF16)
    k.lin_fwd_splitk(x, w, b, part, y, relu)
    return y


def _conv_fwd(k, x, idx, ws, b, B):
    z = torch.empty(B, FEAT, device=DEV, dtype=BF16)
    k.tfcnn_conv_fwd(x, idx, ws, b, z)
    return z


def _conv_dev(w, b):
    """Kernel-layout master, bias and shadow on the device from the conv tensors in torch's layout."""
    wk = w.reshape(32, 9).to(DEV, F32).contiguous()
    return wk, b.to(DEV, F32).clone(), mnist_tfcnn.conv_shadow(wk)


# ------------------------------------------------------------------------------ lin_fwd_splitk
@functools.lru_cache(maxsize=None)
def _lin_refs(M, N, K, exact):
    """Operands and the unrounded product in fp32 and fp64, computed once per shape."""
    x, w, b = O.lin_case(M, N, K, 7 * M + N, exact)
    return x, w, b, x @ w.t(), x.double() @ w.double().t()


def _epi(pre, b, bias, relu):
    y = pre + b.to(pre.dtype) if bias else pre
    return (torch.relu(y) if relu else y).to(BF16).to(pre.dtype)


def _shapes(k):
    ks = k.LIN_SPLITK_KS
    return [(3, 16, 8), (17, 72, ks + 8), (65, 128, 2 * ks + 8), (65, 128, FEAT)]


@pytest.mark.parametrize("bias,relu", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("shape", range(4))
def test_lin_fwd_splitk(k, shape, bias, relu):
    M, N, K = _shapes(k)[shape]
    assert k.lin_splitk_part_size(M, N, K) == -(-K // k.LIN_SPLITK_KS) * M * N
    fails = []
    for exact in (True, False):
        x, w, b, pre32, pre64 = _lin_refs(M, N, K, exact)
        xd, wd, bd = x.to(DEV, BF16), w.to(DEV, BF16), (b.to(DEV) if bias else None)
        y = _splitk(k, xd, wd, bd, relu)
        r32, r64 = _epi(pre32, b, bias, relu), _epi(pre64, b, bias, relu)
        if exact:
            same = torch.equal(y.cpu().float(), r32)
            print("splitk M%d N%d K%d bias=%d relu=%d exact arm equal: %s (max |y| %.1f)" % (
                M, N, K, bias, relu, same, float(r32.abs().max())))
            assert torch.equal(r32.double(), r64)
            assert same
        else:
            fails += O.held("splitk M%d N%d K%d bias=%d relu=%d" % (M, N, K, bias, relu), y.cpu().float(), r32, r64)
            # a batch's rows equal the rows computed alone: the slab width does not depend on M
            rows = torch.cat([_splitk(k, xd[i:i + 1].contiguous(), wd, bd, relu) for i in range(M)])
            assert torch.equal(rows, y)
    assert fails == []


# ------------------------------------------------------------------------------ exact arm
@pytest.mark.parametrize("B", O.BATCHES)
def test_kernels_exact(k, B):
    c = O.exact_case(B, 20 + B)
    x = c["x"].view(O.ROWS, 784).to(DEV, BF16)
    idx = c["idx"].to(DEV)
    xg = c["x"][c["idx"]]
    if B == 3:
        assert int(idx[0]) == int(idx[1])
    wk, bk, ws = _conv_dev(c["w"], c["b"])
    got, ref = {}, {}

    # conv forward, gathered; and without the gather
    ref["z"] = O.z_rows(O.conv_fwd(xg, c["w"], c["b"], F32, BF16))
    zk = _conv_fwd(k, x, idx, ws, bk, B)
    got["z"] = zk.cpu().float()
    assert torch.equal(_conv_fwd(k, x[c["idx"]].contiguous(), None, ws, bk, B), zk)

    # fc1 forward (split-K) and dgrad on a drawn z
    zin = c["zin"].to(DEV, BF16)
    w16 = c["w1"].to(DEV, BF16)
    ref["h"] = O.lin(c["zin"], c["w1"], c["b1"], True, F32, BF16)
    got["h"] = _splitk(k, zin, w16, c["b1"].to(DEV), True).cpu().float()
    ref["dz"] = O.lin(c["dh"], c["w1"].t(), None, False, F32, BF16) * (c["zin"] > 0)
    dzk = torch.empty(B, FEAT, device=DEV, dtype=BF16)
    k.lin_fwd(c["dh"].to(DEV, BF16), None, w16.t().contiguous(), None, zin, dzk, False)
    got["dz"] = dzk.cpu().float()

    # conv weight gradient + SGD from zero momentum: the buffer is the gradient
    rgw, rgb = O.conv_wgrad(c["dz"], xg, F32, BF16)
    (rw, _, _), (rb, _, _) = O.optimizer_step("sgd", [(c["w"], rgw, torch.zeros_like(rgw), None),
                                                      (c["b"], rgb, torch.zeros_like(rgb), None)], O.EXACT_LR, 0.5)
    wm, bm = torch.zeros_like(wk), torch.zeros_like(bk)
    part = torch.empty(k.tfcnn_part_size(B), device=DEV, dtype=F32)
    k.tfcnn_conv_wgrad_sgd(O.z_rows(c["dz"]).to(DEV, BF16), x, idx, part, wk, wm, bk, bm, ws, _lr(O.EXACT_LR), 0.5)
    got.update({"g.conv.weight": wm.cpu().view(32, 1, 3, 3), "g.conv.bias": bm.cpu(),
                "conv.weight": wk.cpu().view(32, 1, 3, 3), "conv.bias": bk.cpu(), "ws": ws.cpu().float()})
    ref.update({"g.conv.weight": rgw, "g.conv.bias": rgb, "conv.weight": rw, "conv.bias": rb,
                "ws": rw.view(32, 9).t().to(BF16).float()})
    bad = O.exact_mismatches(got, ref, list(ref))
    print("B=%d exact arm: max |z| %.0f, max |h| %.0f, max |dz| %.1f, max |dW| %.0f, mismatches %s" % (
        B, float(ref["z"].max()), float(ref["h"].max()), float(ref["dz"].abs().max()), float(rgw.abs().max()), bad))
    assert bad == []


# ------------------------------------------------------------------------------ generic arm
@pytest.mark.parametrize("B", O.BATCHES)
def test_kernels_generic(k, B):
    x, y, idx, net = O.generic_case(B, 40 + B)
    p = O.params_from_module(net)
    g = torch.Generator().manual_seed(90 + B)
    xd, idxd, xg = x.view(O.ROWS, 784).to(DEV, BF16), idx.to(DEV), x[idx]
    wk, bk, ws = _conv_dev(p["conv.weight"], p["conv.bias"])
    print("B=%d generic arm (figure/bar)" % B)
    fails = []

    # conv forward
    z32 = O.z_rows(O.conv_fwd(xg, p["conv.weight"], p["conv.bias"], F32, BF16))
    z64 = O.z_rows(O.conv_fwd(xg, p["conv.weight"], p["conv.bias"], F64, BF16))
    fails += O.held("z", _conv_fwd(k, xd, idxd, ws, bk, B).cpu().float(), z32, z64)

    # fc1 forward on the split-K kernel, fed the fp32 oracle's z
    zd = z32.to(DEV, BF16)
    w16 = p["fc1.weight"].to(DEV, BF16)
    b1 = 0.1 * torch.randn(HID, generator=g)  # Keras starts the bias at zero: draw one, the epilogue adds it
    h32, h64 = (O.lin(z32, p["fc1.weight"], b1, True, gd, BF16) for gd in (F32, F64))
    fails += O.held("h (split-K)", _splitk(k, zd, w16, b1.to(DEV), True).cpu().float(), h32, h64)

    # fc1 dgrad: dz already masked
    dh = ((0.1 * torch.randn(B, HID, generator=g)) * (h32 > 0)).to(BF16).float()
    dz32, dz64 = (O.lin(dh, p["fc1.weight"].t(), None, False, gd, BF16) * (z32 > 0) for gd in (F32, F64))
    dzk = torch.empty(B, FEAT, device=DEV, dtype=BF16)
    k.lin_fwd(dh.to(DEV, BF16), None, w16.t().contiguous(), None, zd, dzk, False)
    fails += O.held("dz", dzk.cpu().float(), dz32, dz64)
    assert _zero(dzk.cpu()[z32 <= 0])  # the ReLU mask is exact

    # conv weight gradient with both epilogues, from a carried, drawn state (t = 100 for Adam)
    dzc = O.from_z_rows(dz32)
    part = torch.empty(k.tfcnn_part_size(B), device=DEV, dtype=F32)
    for optimizer, lr in (("sgd", O.LR), ("adam", O.ADAM_LR)):
        st = O.drawn_state({n: p[n] for n in ("conv.weight", "conv.bias")}, optimizer, 300 + B)
        names = O.STATE[optimizer]
        refs = []
        for gd in (F32, F64):
            gw, gb = O.conv_wgrad(dzc, xg, gd, BF16)
            refs.append(O.optimizer_step(optimizer, [
                (p[n], gr.float(), st[names[0]][n], st[names[1]][n] if optimizer == "adam" else None)
                for n, gr in (("conv.weight", gw), ("conv.bias", gb))], lr, O.MOMENTUM, 101))
        w, b, s = wk.clone(), bk.clone(), ws.clone()
        s0w, s0b = st[names[0]]["conv.weight"].reshape(32, 9).to(DEV), st[names[0]]["conv.bias"].to(DEV)
        if optimizer == "adam":
            s1w, s1b = st[names[1]]["conv.weight"].reshape(32, 9).to(DEV), st[names[1]]["conv.bias"].to(DEV)
            step_t = torch.full((1,), 101, device=DEV, dtype=torch.int32)
            k.tfcnn_conv_wgrad_adam(dz32.to(DEV, BF16), xd, idxd, part, w, s0w, s1w, b, s0b, s1b, s, _lr(lr), step_t,
                                    O.ADAM_BETAS[0], O.ADAM_BETAS[1], O.ADAM_EPS)
            assert int(step_t) == 101  # the weight gradient reads the counter, it never advances it
        else:
            k.tfcnn_conv_wgrad_sgd(dz32.to(DEV, BF16), xd, idxd, part, w, s0w, b, s0b, s, _lr(lr), O.MOMENTUM)
        (w32, a32, v32), (b32, ab32, vb32) = refs[0]
        (w64, a64, v64), (b64, ab64, vb64) = refs[1]
        w0, b0 = p["conv.weight"], p["conv.bias"]
        fails += O.held(optimizer + " " + names[0] + " w", s0w.cpu().view(32, 1, 3, 3), a32, a64)
        fails += O.held(optimizer + " " + names[0] + " b", s0b.cpu(), ab32, ab64)
        if optimizer == "adam":
            fails += O.held("adam exp_avg_sq w", s1w.cpu().view(32, 1, 3, 3), v32, v64)
            fails += O.held("adam exp_avg_sq b", s1b.cpu(), vb32, vb64)
        fails += O.held(optimizer + " conv upd", w.cpu().view(32, 1, 3, 3) - w0, w32 - w0, w64 - w0)
        fails += O.held(optimizer + " conv bias upd", b.cpu() - b0, b32 - b0, b64 - b0)
        assert torch.equal(s, mnist_tfcnn.conv_shadow(w))  # the shadow is the new master, rounded
    assert fails == []


# ------------------------------------------------------------------------------ model level
def _cpu(sd):
    return {n: t.detach().cpu().clone() for n, t in sd.items()}


def _pads_zero(hip):
    for d in (hip.p, hip.s0) + ((hip.s1,) if hip.s1 is not None else ()):
        assert _zero(d["fc2.weight"][10:], d["fc2.bias"][10:])
    assert _zero(hip.fc[1]["w16"][10:], hip.fc[1]["w16t"][:, 10:])


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
def test_hiptfcnn_steps_like_the_oracle_eager_and_replayed(optimizer):
    x, y, idx, net = O.generic_case(17, 3)
    xg, yg = x[idx], y[idx]
    lr = O.LR if optimizer == "sgd" else O.ADAM_LR
    p0 = O.params_from_module(net)
    # SGD starts from zero momentum; Adam from a loaded, well-conditioned state (its first step from zero
    # is ill-conditioned: test_adam_from_the_zero_state)
    st0 = O.zero_state(p0, optimizer) if optimizer == "sgd" else O.drawn_state(p0, optimizer, 77)
    start = O.state_dict(p0, st0, optimizer)
    refs, losses = [], []
    for gd in (F32, F64):
        p = {n: t.clone() for n, t in p0.items()}
        st = {s: ({n: t.clone() for n, t in v.items()} if isinstance(v, dict) else v) for s, v in st0.items()}
        losses.append(sum(O.train_step(p, st, xg, yg, lr, optimizer, O.MOMENTUM, gd, BF16)["loss"]
                          for _ in range(O.STEPS)))
        refs.append(O.state_dict(p, st, optimizer))
    xd, yd, idxd = x.view(O.ROWS, 784).to(DEV, BF16), y.to(DEV), idx.to(DEV)

    def run(captured):
        hip = mnist_tfcnn.HipTFCNN(net, lr, O.MOMENTUM, DEV, optimizer)
        hip.load_optim_state(start)
        step = CapturedStep(lambda: hip.train_step(xd, yd, idxd), enabled=captured, warmup=0)
        for _ in range(O.STEPS):
            step()
        torch.cuda.synchronize()
        assert (step.graph is not None) == captured
        return hip, _cpu(hip.state_dict()), hip.stats.cpu()

    hip, got, stats = run(False)
    assert set(got) == set(refs[0])
    assert all(got[n].shape == refs[0][n].shape and got[n].dtype == (torch.int64 if n == "step" else F32) for n in got)
    loss_bar = max(1e-2, 4 * abs(losses[0] - losses[1]) / losses[1])
    print("%s: summed loss hip %.5f oracle fp32 %.5f fp64 %.5f; correct %d" % (
        optimizer, float(stats[0]), losses[0], losses[1], int(stats[1])))
    fails = O.state_failures(got, refs[0], refs[1], start, optimizer, "model " + optimizer)
    assert fails == []
    assert abs(float(stats[0]) - losses[0]) / losses[0] < loss_bar
    if optimizer == "adam":
        assert int(got["step"]) == 100 + O.STEPS
    _pads_zero(hip)
    for n, t in got.items():
        assert bool(torch.isfinite(t.float()).all()), n
    _, again, stats2 = run(False)
    hip_g, replayed, stats3 = run(True)
    for n in got:  # the state and, for Adam, the step counter
        assert torch.equal(got[n], again[n]), ("second eager run", n)
        assert torch.equal(got[n], replayed[n]), ("replayed", n)
    assert torch.equal(stats, stats2) and torch.equal(stats, stats3)
    _pads_zero(hip_g)


def test_adam_from_the_zero_state():
    """At t = 1 every element's update is lr g / (|g| + c eps): its sign rests on the last bits of the
    gradient, so no value is compared. B = 3 with a repeated row: a quarter of the z columns are zero for
    the whole batch, so there are fc1 weights whose gradient is exactly zero."""
    x, y, idx, net = O.generic_case(3, 9)
    p = O.params_from_module(net)
    out = O.train_step({n: t.clone() for n, t in p.items()}, O.zero_state(p, "adam"), x[idx], y[idx], O.ADAM_LR,
                       "adam", 0.0, F32, BF16)
    hip = mnist_tfcnn.HipTFCNN(net, O.ADAM_LR, 0.0, DEV, "adam")
    hip.train_step(x.view(O.ROWS, 784).to(DEV, BF16), y.to(DEV), idx.to(DEV))
    torch.cuda.synchronize()
    got = _cpu(hip.state_dict())
    assert int(got["step"]) == 1
    for n in O.PARAMS:
        d = (got[n] - p[n]).abs()
        zero_g = out["g." + n] == 0
        moved = int((d[zero_g] != 0).sum())
        print("adam t=1 %-11s max |upd| / lr %.6f; oracle gradient exactly zero on %d of %d elements, moved %d" % (
            n, float(d.max()) / O.ADAM_LR, int(zero_g.sum()), zero_g.numel(), moved))
        assert bool(torch.isfinite(got[n]).all()) and bool(torch.isfinite(got["exp_avg." + n]).all())
        assert bool(torch.isfinite(got["exp_avg_sq." + n]).all())
        assert float(d.max()) <= O.ADAM_LR * (1 + 1e-3)
        assert moved == 0
    assert int((out["g.fc1.weight"] == 0).sum()) > 1000  # the zero-gradient check is not vacuous
    _pads_zero(hip)


def test_forward_of_a_batch_equals_the_rows_alone():
    x, y, idx, net = O.generic_case(1, 7)
    g = torch.Generator().manual_seed(8)
    x70 = torch.randn(70, 784, generator=g).to(DEV, BF16)
    hip = mnist_tfcnn.HipTFCNN(net, O.LR, O.MOMENTUM, DEV, "sgd")
    whole = hip.forward(x70)
    rows = torch.cat([hip.forward(x70[i:i + 1]) for i in range(70)])
    gathered = hip.forward(x70, torch.arange(69, -1, -1, device=DEV)).flip(0)
    ref = net(x70.float().cpu().view(70, 1, 28, 28)).detach()
    print("forward B=70: logits against the fp32 module %.2e; padded logits max %.1f" % (
        O.rel(whole[:, :10].float(), ref), float(whole[:, 10:].float().abs().max())))
    assert whole.shape == (70, 16) and whole.dtype == BF16
    assert torch.equal(whole, rows) and torch.equal(whole, gathered)
    assert _zero(whole[:, 10:])
    assert O.rel(whole[:, :10].float(), ref) < 5e-2  # bf16 operands against fp32: a plumbing bound


# ------------------------------------------------------------------------------ trial level
TRAIN = re.compile(r"^Train Epoch: 1 \[(\d+)/1280 \((\d+)%\)\]\tloss=(\d+\.\d{4}), accuracy=(\d+\.\d{4})$", re.M)
TEST = re.compile(r"^Test Loss: (\d+\.\d{4}), Test Accuracy: (\d+\.\d{4})$", re.M)
METRICS = ["test/accuracy", "test/loss", "train/accuracy", "train/loss"]


@pytest.mark.parametrize("optimizer,lr", [("adam", "0.001"), ("sgd", "0.05")])
def test_trial_hip_prints_the_lines_writes_the_summaries_and_learns(optimizer, lr, capsys, tmp_path, monkeypatch):
    monkeypatch.delenv("TF_CONFIG", raising=False)
    common = ["--epochs", "1", "--num-train", "1280", "--num-test", "500", "--batch-size", "64", "--optimizer",
              optimizer, "--learning-rate", lr, "--log-interval", "5"]
    a_hip = mnist_tfcnn.main(common + ["--impl", "hip", "--log-path", str(tmp_path / "hip")])
    out_hip = capsys.readouterr().out
    a_mod = mnist_tfcnn.main(common + ["--impl", "module", "--log-path", str(tmp_path / "mod")])
    out_mod = capsys.readouterr().out
    print(out_hip)
    print("trial accuracy %s: hip %.4f module %.4f (chance 0.1)" % (optimizer, a_hip, a_mod))
    th, tm = TRAIN.findall(out_hip), TRAIN.findall(out_mod)
    assert [t[:2] for t in th] == [t[:2] for t in tm] and len(th) == 4
    assert len(TEST.findall(out_hip)) == 1 and len(TEST.findall(out_mod)) == 1
    assert all(math.isfinite(float(t[2])) for t in th)
    assert abs(float(th[0][2]) - float(tm[0][2])) < 0.05  # the first batch, before any update: the same loss
    for d, acc in (("hip", a_hip), ("mod", a_mod)):
        got = tfevent.collect(str(tmp_path / d), METRICS)
        assert sorted(name for _, name, _ in got) == METRICS
        vals = {name: float(v) for _, name, v in got}
        assert all(math.isfinite(v) for v in vals.values())
        assert vals["test/accuracy"] == pytest.approx(acc, rel=1e-5)
    assert a_hip >= 0.1 + 0.5 * (a_mod - 0.1), (a_hip, a_mod)


# ------------------------------------------------------------------------------ experiment level
def test_example_runs_through_the_scheduler_with_the_tfevent_collector(tmp_path):
    from katib_amd.controller.manager import Manager

    e = load_experiment(os.path.join(ROOT, "examples", "kubeflow-training-operator", "tfjob-mnist-with-summaries.yaml"))
    e.spec.max_trial_count = e.spec.parallel_trial_count = 2
    e.spec.max_failed_trial_count = 1
    c =e.spec.trial_template.trial_spec["spec"]["tfReplicaSpecs"]["Worker"]["template"]["spec"]["containers"][0]
    c["command"][0] = sys.executable
    c["command"] += ["--num-train=6400", "--num-test=1000"]  # a short trial: what is tested is the plumbing
    m = Manager(state_dir=str(tmp_path / "state"), num_devices=1, journal=False)
    m.config.amd.slots_per_device = 2
    m.slots = m.N.SlotPool(1, 2)
    try:
        m.create_experiment(e)
        done = m.run_until_complete(e.metadata.name, namespace=e.metadata.namespace, timeout=240)
        assert EC.is_succeeded(done), done.status.conditions
        assert done.status.trials_succeeded == 2
        best = {mt.name: mt for mt in done.status.current_optimal_trial.observation.metrics}
        print("optimal trial %s: %s" % (done.status.current_optimal_trial.best_trial_name,
                                        {n: mt.latest for n, mt in best.items()}))
        assert set(best) == set(METRICS)  # named after the writers' directories: the TFEvent collector read them
        assert 0.0 <= float(best["test/accuracy"].latest) <= 1.0
    finally:
        m.shutdown()
    files = glob.glob(os.path.join(str(tmp_path), "**", "events.out.tfevents*"), recursive=True)
    roots = {f.split("/mnist-with-summaries-logs/")[0] for f in files}
    print("event files:", sorted(os.path.relpath(f, str(tmp_path)) for f in files))
    assert len(files) == 4 and all("/mnist-with-summaries-logs/" in f for f in files)
    assert len(roots) == 2  # each trial wrote under its own directory
