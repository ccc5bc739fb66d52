"""tests/mnist_tfcnn_oracle.py and katib_amd/workloads/mnist_tfcnn.py checked without a GPU: the oracle
against autograd and the torch optimizers, the exact arm's exactness, the checkers of
tests/test_gpu_mnist_tfcnn.py against wrong steps they must reject, the layout and optimizer-state round
trips, the trial's lines and summaries on the module path, the notebook's objective, and the example.

Every test prints the figures it measured (``pytest -s``) before it asserts.
"""
import inspect
import os
import re

import pytest
import torch
import torch.nn.functional as F

import mnist_tfcnn_oracle as O
from katib_amd.api.defaults import set_default
from katib_amd.api.validation import validate_experiment
from katib_amd.api.yaml_io import load_experiment
from katib_amd.controller.jobs import make_plan
from katib_amd.metricscollector import tfevent
from katib_amd.workloads import mnist_tfcnn

F32, F64, BF16 = O.F32, O.F64, O.BF16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# fp64 against fp64 on the same graph: the two differ by summation order alone, 1e-16 per term over sums of
# up to 1.1e4 terms. SGD is linear in the gradient; Adam's first step divides by |g| + eps, which magnifies
# an absolute gradient error by at most lr / eps = 1e4
@pytest.mark.parametrize("optimizer,lr,bar", [("sgd", O.LR, 1e-12), ("adam", O.ADAM_LR, 1e-9)])
def test_oracle_equals_autograd_over_three_steps(optimizer, lr, bar):
    x, y, idx, net = O.generic_case(17, 5)
    net = net.double()
    p = O.params_from_module(net, F64)
    st = O.zero_state(p, optimizer)
    opt = (torch.optim.SGD(net.parameters(), lr=lr, momentum=O.MOMENTUM) if optimizer == "sgd"
           else torch.optim.Adam(net.parameters(), lr=lr, eps=O.ADAM_EPS))
    xg, yg = x[idx].double(), y[idx]
    for _ in range(O.STEPS):
        out = O.train_step(p, st, xg, yg, lr, optimizer, O.MOMENTUM, F64, None)
        loss = F.cross_entropy(net(xg), yg)
        opt.zero_grad()
        loss.backward()
        opt.step()
        assert abs(out["loss"] - loss.item()) < 1e-12 * max(1.0, abs(loss.item()))
    worst = 0.0
    for n, t in net.named_parameters():
        pairs = [(p[n], t.detach())]
        for s in O.STATE[optimizer]:
            pairs.append((st[s][n], opt.state[t][s]))
        for got, ref in pairs:
            assert got.dtype == F64 and got.shape == ref.shape
            worst = max(worst, O.rel(got, ref))
    print("oracle vs autograd, %s, 3 steps: worst relative distance %.2e / %.0e" % (optimizer, worst, bar))
    assert worst < bar
    assert st["t"] == O.STEPS


@pytest.mark.parametrize("B", O.BATCHES)
def test_exact_case_sums_are_exact_in_fp32(B):
    """What the exact arm rests on: the fp32 oracle equals the fp64 one bit for bit on these operands."""
    c = O.exact_case(B, 20 + B)
    x = c["x"][c["idx"]]
    for gd in (F32, F64):
        z = O.conv_fwd(x, c["w"], c["b"], gd, BF16)
        h = O.lin(c["zin"], c["w1"], c["b1"], True, gd, BF16)
        hpre = c["zin"].to(gd) @ c["w1"].to(gd).t()
        dz = O.lin(c["dh"], c["w1"].t(), None, False, gd, BF16) * (c["zin"] > 0)
        gw, gb = O.conv_wgrad(c["dz"], x, gd, BF16)
        got = [z, h, hpre, dz, gw, gb]
        if gd == F32:
            first = got
    worst = max(float(t.abs().max()) for t in got)
    print("B=%d exact case: largest magnitude %.1f (fp32 holds multiples of 0.5 to 2^23); max |z| %.0f" % (
        B, worst, float(z.max())))
    assert worst < 2 ** 23 / 4
    for a, b in zip(first, got):
        assert torch.equal(a.double(), b.double())
    assert float(z.max()) <= 256  # z is an integer bf16 holds exactly
    assert 0.2 < float((h > 0).float().mean()) < 0.8  # the ReLU of the split-K epilogue is exercised both ways


@pytest.mark.parametrize("exact", [True, False])
def test_lin_case_shapes(exact):
    x, w, b = O.lin_case(17, 72, 520, 3, exact)
    assert x.shape == (17, 520) and w.shape == (72, 520) and b.shape == (72,)
    assert torch.equal(x, x.to(BF16).float()) and torch.equal(w, w.to(BF16).float())


def _steps(net, xg, yg, optimizer, gd, mutant=None):
    p = O.params_from_module(net)
    st = O.zero_state(p, optimizer) if optimizer == "sgd" else O.drawn_state(p, optimizer, 77)
    lr = O.LR if optimizer == "sgd" else O.ADAM_LR
    for _ in range(O.STEPS):
        O.train_step(p, st, xg, yg, lr, optimizer, O.MOMENTUM, gd, BF16, mutant)
    return O.state_dict(p, st, optimizer)


@pytest.fixture(scope="module")
def model_refs():
    x, y, idx, net = O.generic_case(17, 3)
    xg, yg = x[idx], y[idx]
    before = {n: t.clone() for n, t in O.params_from_module(net).items()}
    refs = {o: (_steps(net, xg, yg, o, F32), _steps(net, xg, yg, o, F64)) for o in ("sgd", "adam")}
    return net, xg, yg, before, refs


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
def test_state_checker_accepts_the_oracle_itself(model_refs, optimizer):
    net, xg, yg, before, refs = model_refs
    r32, r64 = refs[optimizer]
    assert O.state_failures(r32, r32, r64, before, optimizer, "self") == []
    assert set(r32) == set(mnist_tfcnn.PARAMS) | {s + "." + n for s in O.STATE[optimizer] for n in mnist_tfcnn.PARAMS} | (
        {"step"} if optimizer == "adam" else set())


@pytest.mark.parametrize("optimizer,mutant", [("sgd", "nchw_flatten"), ("sgd", "post_update_dgrad"),
                                              ("sgd", "relu_mask_ge"), ("sgd", "no_db"),
                                              ("adam", "adam_no_bias_correction"), ("adam", "nchw_flatten"),
                                              ("adam", "no_db")])
def test_state_checker_rejects(model_refs, optimizer, mutant):
    net, xg, yg, before, refs = model_refs
    r32, r64 = refs[optimizer]
    fails = O.state_failures(_steps(net, xg, yg, optimizer, F32, mutant), r32, r64, before, optimizer, mutant,
                             out=lambda s: None)
    print(optimizer, mutant, "rejected on", [f[0] for f in fails])
    assert fails


def test_exact_checker_rejects_a_wrong_mask_and_a_missing_bias_gradient():
    """The exact arm compares dz and the conv gradients bit for bit: a mask ``>= 0`` and a missing db show."""
    c = O.exact_case(3, 11)
    x = c["x"][c["idx"]]
    dz = O.lin(c["dh"], c["w1"].t(), None, False, F32, BF16)
    good = {"dz": dz * (c["zin"] > 0)}
    bad = {"dz": dz * (c["zin"] >= 0)}
    assert O.exact_mismatches(good, good, ["dz"]) == [] and O.exact_mismatches(bad, good, ["dz"]) == ["dz"]
    gw, gb = O.conv_wgrad(c["dz"], x, F32, BF16)
    ref = {"g.conv.weight": gw, "g.conv.bias": gb}
    assert O.exact_mismatches({"g.conv.weight": gw, "g.conv.bias": torch.zeros_like(gb)}, ref, list(ref)) == ["g.conv.bias"]
    # ... and the NCHW flatten order is another z
    z = O.conv_fwd(x, c["w"], c["b"], F32, BF16)
    assert O.exact_mismatches({"z": z.flatten(1)}, {"z": O.z_rows(z)}, ["z"]) == ["z"]


def test_layout_round_trip_is_exact():
    torch.manual_seed(3)
    sd = {n: torch.randn_like(t) for n, t in mnist_tfcnn.TFNet().state_dict().items()}
    k = mnist_tfcnn.pack_state(sd)
    assert {n: tuple(t.shape) for n, t in k.items()} == {
        "conv.weight": (32, 9), "conv.bias": (32,), "fc1.weight": (128, 21632), "fc1.bias": (128,),
        "fc2.weight": (16, 128), "fc2.bias": (16,)}
    back = mnist_tfcnn.unpack_state(k)
    for n in O.PARAMS:
        assert back[n].shape == sd[n].shape and torch.equal(back[n], sd[n]), n
    assert float(k["fc2.weight"][10:].abs().max()) == 0 and float(k["fc2.bias"][10:].abs().max()) == 0
    assert k["conv.weight"][7, 2 * 3 + 1] == sd["conv.weight"][7, 0, 2, 1]
    ws = mnist_tfcnn.conv_shadow(k["conv.weight"])
    assert ws.shape == (9, 32) and ws.dtype == BF16 and ws[2 * 3 + 1, 7] == sd["conv.weight"][7, 0, 2, 1].to(BF16)


def test_tfnet_is_keras_model_in_keras_order():
    torch.manual_seed(0)
    net = mnist_tfcnn.TFNet()
    assert all(float(m.bias.detach().abs().max()) == 0 for m in (net.conv, net.fc1, net.fc2))
    for m, fan in ((net.conv, 9 + 9 * 32), (net.fc1, 21632 + 128), (net.fc2, 128 + 10)):
        lim, top = (6.0 / fan) ** 0.5, float(m.weight.detach().abs().max())  # glorot_uniform
        assert 0.9 * lim < top <= lim
    x = torch.randn(2, 1, 28, 28)
    z = F.relu(net.conv(x))
    ref = F.relu(z.permute(0, 2, 3, 1).reshape(2, -1) @ net.fc1.weight.t()) @ net.fc2.weight.t()
    assert torch.allclose(net(x), ref, atol=1e-5)
    # column (pixel p, channel c) of fc1 multiplies z[c] at pixel p
    assert torch.equal(O.z_rows(z)[:, 5 * 32 + 7], z[:, 7, 0, 5])


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
def test_optimizer_state_round_trip(optimizer):
    torch.manual_seed(4)
    net = mnist_tfcnn.TFNet()
    hip = mnist_tfcnn.HipTFCNN(net, 0.01, 0.5, "cpu", optimizer)
    sd0 = hip.state_dict()
    want = {"momentum_buffer." + n for n in O.PARAMS} if optimizer == "sgd" else (
        {s + n for s in ("exp_avg.", "exp_avg_sq.") for n in O.PARAMS} | {"step"})
    assert set(sd0) == set(O.PARAMS) | want
    for n, t in net.state_dict().items():
        assert torch.equal(sd0[n], t) and sd0[n].dtype == F32
    st = O.drawn_state(O.params_from_module(net), optimizer, 5, t=100)
    hip.load_optim_state(O.state_dict(O.params_from_module(net), st, optimizer))
    sd1 = hip.state_dict()
    for s in O.STATE[optimizer]:
        for n in O.PARAMS:
            assert torch.equal(sd1[s + "." + n], st[s][n]), (s, n)
        assert float(getattr(hip, "s0" if s != "exp_avg_sq" else "s1")["fc2.weight"][10:].abs().max()) == 0
    if optimizer == "adam":
        assert int(sd1["step"]) == 100 and int(hip.step_t) == 100


# ------------------------------------------------------------------------------ the trial, module path
TRAIN = re.compile(r"^Train Epoch: (\d+) \[(\d+)/256 \((\d+)%\)\]\tloss=(\d+\.\d{4}), accuracy=(\d+\.\d{4})$", re.M)
TEST = re.compile(r"^Test Loss: (\d+\.\d{4}), Test Accuracy: (\d+\.\d{4})$", re.M)


@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_trial_module_lines_summaries_and_running_means(optimizer, tmp_path, capsys, monkeypatch):
    monkeypatch.delenv("TF_CONFIG", raising=False)
    seen = {"test": [], "train": []}
    real_logits, real_step = mnist_tfcnn._Trainer.test_logits, mnist_tfcnn._Trainer.step

    def test_logits(self, *a, **kw):
        out = real_logits(self, *a, **kw)
        seen["test"].append((out.clone(), self.vy.clone()))
        return out

    def step(self, idx):
        before = self.stats.clone()
        real_step(self, idx)
        seen["train"].append((self.stats - before).tolist())

    monkeypatch.setattr(mnist_tfcnn._Trainer, "test_logits", test_logits)
    monkeypatch.setattr(mnist_tfcnn._Trainer, "step", step)
    log = str(tmp_path / "logs")
    acc = mnist_tfcnn.main(["--impl", "module", "--optimizer", optimizer, "--epochs", "3", "--num-train", "256",
                            "--num-test", "100", "--batch-size", "32", "--log-interval", "3",
                            "--learning-rate", "0.001" if optimizer == "adam" else "0.05", "--log-path", log])
    out = capsys.readouterr().out
    print(out)
    tr, te = TRAIN.findall(out), TEST.findall(out)
    assert len(tr) == 9 and len(te) == 3  # 8 steps per epoch, logged at 0, 3, 6
    assert [(t[0], t[1], t[2]) for t in tr[:3]] == [("1", "0", "0"), ("1", "96", "38"), ("1", "192", "75")]
    got = tfevent.collect(log, ["test/accuracy", "test/loss", "train/accuracy", "train/loss"])
    series = {m: [float(v) for _, name, v in got if name == m] for m in
              ("test/accuracy", "test/loss", "train/accuracy", "train/loss")}
    assert all(len(v) == 3 for v in series.values()), series  # one point per epoch
    steps = sorted(parsed[1] for d in ("train", "test") for fn in os.listdir(os.path.join(log, d))
                   for parsed in map(tfevent.parse_event, tfevent.read_records(os.path.join(log, d, fn))))
    assert steps == [0] * 4 + [1] * 4 + [2] * 4  # step = epoch, as the reference writes it
    # running means since the start of the trial, not per-epoch values
    bs, n = 32, 100
    tl_sum = tb = tc = 0
    for e, (logits, vy) in enumerate(seen["test"]):
        per = F.cross_entropy(logits, vy, reduction="none")
        means = [float(c.mean()) for c in per.split(bs)]
        tl_sum, tb, tc = tl_sum + sum(means), tb + len(means), tc + int((logits.argmax(1) == vy).sum())
        assert series["test/loss"][e] == pytest.approx(tl_sum / tb, rel=1e-5)
        assert series["test/accuracy"][e] == pytest.approx(tc / ((e + 1) * n), rel=1e-5)
        assert float(te[e][0]) == pytest.approx(tl_sum / tb, abs=6e-5)
        assert float(te[e][1]) == pytest.approx(100 * tc / ((e + 1) * n), abs=6e-5)  # the lines: x 100
        k = 8 * (e + 1)
        assert series["train/loss"][e] == pytest.approx(sum(s[0] for s in seen["train"][:k]) / k, rel=1e-5)
        assert series["train/accuracy"][e] == pytest.approx(sum(s[1] for s in seen["train"][:k]) / (k * bs), rel=1e-5)
    per_epoch = [sum(s[0] for s in seen["train"][8 * e:8 * e + 8]) / 8 for e in range(3)]
    print("train loss per epoch %s, reported (running) %s" % (per_epoch, series["train/loss"]))
    assert abs(per_epoch[2] - series["train/loss"][2]) > 1e-3  # the two differ on this run: the check can tell
    assert acc == pytest.approx(series["test/accuracy"][-1], rel=1e-5)


def test_only_task_zero_writes_and_prints(tmp_path, capsys, monkeypatch):
    monkeypatch.setenv("TF_CONFIG", '{"cluster": {"worker": ["a:1", "b:2"]}, "task": {"type": "worker", "index": 1}}')
    log = str(tmp_path / "logs")
    mnist_tfcnn.main(["--epochs", "1", "--num-train", "64", "--num-test", "32", "--batch-size", "32", "--log-path", log])
    assert capsys.readouterr().out == "" and not os.path.exists(log)


def test_impl_defaults_and_hip_exit_without_a_gpu(monkeypatch):
    a = mnist_tfcnn.parse_args([])
    assert (a.impl, a.capture, a.optimizer, a.batch_size, a.learning_rate, a.epochs, a.log_interval) == (
        "module", 1, "adam", 64, 0.001, 10, 100)
    assert a.momentum == 0 and a.steps_per_epoch == 0
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit) as e:
        mnist_tfcnn.main(["--impl", "hip", "--num-train", "64", "--num-test", "64"])
    assert "--impl hip needs a GPU" in str(e.value) and "\n" not in str(e.value)


def test_train_mnist_model_prints_the_notebook_line(capsys, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)  # the module path, wherever this runs
    ns = {}
    exec(inspect.getsource(mnist_tfcnn.train_mnist_model), ns)  # as KatibClient.tune() ships it: source alone
    ns["train_mnist_model"]({"lr": "0.1", "num_epoch": "2", "num_train": "4480"})
    out = capsys.readouterr().out
    print(out)
    lines = re.findall(r"^Epoch (\d)/2\. accuracy=(\d\.\d{4}) - loss=(\d+\.\d{4})$", out, re.M)
    assert [l[0] for l in lines] == ["1", "2"]
    assert float(lines[1][2]) < float(lines[0][2])  # 140 SGD steps at lr 0.1 on the teacher task: the loss falls


# ------------------------------------------------------------------------------ the example
def test_example_loads_validates_and_plans_one_replica():
    e = load_experiment(os.path.join(ROOT, "examples", "kubeflow-training-operator", "tfjob-mnist-with-summaries.yaml"))
    set_default(e)
    validate_experiment(e)
    assert e.spec.objective.objective_metric_name == "test/accuracy" and e.spec.objective.goal is None
    src = e.spec.metrics_collector_spec.source.file_system_path
    assert e.spec.metrics_collector_spec.collector.kind == "TensorFlowEvent" and src.path == "/mnist-with-summaries-logs"
    plan = make_plan(e.spec.trial_template.trial_spec, "tensorflow", e.spec.trial_template.primary_pod_labels)
    assert plan.kind == "TFJob" and len(plan.replicas) == 1 and plan.replicas[0].primary
    argv = plan.replicas[0].argv
    assert argv[:4] == ["python3", "-m", "katib_amd.workloads.mnist_tfcnn", "--impl=hip"]
    assert "--log-path=" + src.path in argv  # the argument contains the collector path: the scheduler remaps it
    assert plan.replicas[0].gpus == 1
