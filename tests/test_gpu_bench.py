"""bench.py's plain run and ``--dump-outputs``: a plain ``--gpus 1 --steps K --warmup W`` run times the
headline only (everything behind ``--full`` stays null) and writes what the timed step computes from the
seeded initial state on the first batch; two runs with the same arguments write the same arrays."""
import importlib.util
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ["trials_per_hour", "b1_trials_per_hour", "b5_experiment_wall_s", "torch_eager_ms_per_step",
             "torch_graph_ms_per_step", "module_eager_ms_per_step", "measured_search_wall_s", "per_rank_floor_ms"]
NAMES = {"loss": (1,), "logits": (128, 10), "weights": None, "alphas": None, "bn_running_mean": None,
         "bn_running_var": None}


def _bench_module():
    spec = importlib.util.spec_from_file_location("_bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_caps_large_arrays_with_a_fixed_sample(tmp_path, monkeypatch):
    bench = _bench_module()
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 6 * 4 * 50)  # 50 elements per array
    w = torch.arange(1000, dtype=torch.float64)
    search = types.SimpleNamespace(loss_out=torch.tensor(2.5), logits_out=torch.ones(4, 10), W=w, A=torch.zeros(7),
                                   bn=types.SimpleNamespace(mean=torch.zeros(3), var=torch.ones(3)))
    bench.dump_outputs(str(tmp_path / "a"), search)
    bench.dump_outputs(str(tmp_path / "b"), search)
    got = {f[:-4]: np.load(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a"))}
    assert set(got) == set(NAMES) and all(a.dtype == np.float32 for a in got.values())
    assert got["logits"].shape == (4, 10) and float(got["loss"].reshape(-1)[0]) == 2.5
    ws = got["weights"]  # over its share: a sorted sample of distinct elements, the same in every run
    assert ws.shape == (50,) and np.all(np.diff(ws) > 0) and set(ws) <= set(range(1000))
    assert np.array_equal(ws, np.load(str(tmp_path / "b" / "weights.npy")))
    assert sum(a.nbytes for a in got.values()) <= 6 * 4 * 50


def _plain_runs(out_dirs):
    """One plain run per directory, side by side (each is mostly set-up)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
                               "--warmup", "1", "--dump-outputs", d], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                              text=True, env=env, cwd=ROOT) for d in out_dirs]
    res = []
    for p, d in zip(procs, out_dirs):
        stdout, stderr = p.communicate(timeout=120)
        assert p.returncode == 0, stderr[-3000:]
        lines = [ln for ln in stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, stdout[-2000:]
        res.append((json.loads(lines[0]), {n: np.load(os.path.join(d, n + ".npy")) for n in NAMES}))
    return res


@pytest.mark.gpu
def test_plain_run_is_headline_only_and_dumps_its_last_step(tmp_path):
    (r, a), (_, b) = _plain_runs([str(tmp_path / "a"), str(tmp_path / "b")])
    assert r["metric"] == "darts_cifar10_search_wall_clock_s" and r["unit"] == "s" and r["higher_is_better"] is False
    assert r["dtype"] == "fp32" and r["steps"] == 3 and r["warmup"] == 1 and r["full"] is False
    assert r["config"]["ops"] == "hip" and r["config"]["hip_graph"] is True
    assert r["ms_per_step"] > 0
    c = r["config"]
    want = c["epochs"] * c["steps_per_epoch"] * (r["ms_per_step"] + r["ms_valid_batch"]) / 1000.0
    assert abs(r["value"] - want) <= 0.01 * want
    assert all(r[k] is None for k in FULL_ONLY), {k: r[k] for k in FULL_ONLY}
    assert sorted(os.listdir(str(tmp_path / "a"))) == sorted(n + ".npy" for n in NAMES)
    for n, shape in NAMES.items():
        assert a[n].dtype == np.float32 and np.isfinite(a[n]).all() and a[n].size > 0, n
        assert shape is None or a[n].shape == shape, (n, a[n].shape)
    assert sum(x.nbytes for x in a.values()) <= 64 * 1000 * 1000
    assert 1.5 < float(a["loss"][0]) < 3.5  # 10 classes, random-init weights: near ln 10
    # same arguments, same inputs, one step from the same state: a second run repeats the first up to the
    # order of the kernels' fp32 atomic sums. A sum of n <= 128 * 32 * 32 terms moves by ~sqrt(n) eps = 4e-5
    # of its size when reordered; every array here is O(1) or smaller -> 1e-4 absolute
    for n in NAMES:
        d = float(np.abs(a[n].astype(np.float64) - b[n]).max())
        print("%s: max |run a - run b| = %.3g (max |a| = %.3g)" % (n, d, float(np.abs(a[n]).max())))
    for n in NAMES:
        assert a[n].shape == b[n].shape and np.abs(a[n].astype(np.float64) - b[n]).max() <= 1e-4, n
