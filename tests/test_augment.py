"""Device-side random crop + flip (ops/augment.py) and CIFAR-10 loading from disk
(workloads/data.py), on the CPU: the Philox-keyed draw contract against known answers and a
per-pixel Python transcription, the draw statistics, the loader, the batch iterator and the two
workloads' new flags."""
import math
import os

import numpy as np
import pytest
import torch

from katib_amd.ops.augment import PLAIN, AugSpec, augment_gather, augment_reference, cifar_lut, draws

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = (3 << 32) | 77
M32 = 0xFFFFFFFF


# ---------------------------------------------------------------- the contract, in plain Python
def _philox(counter, key):
    c, (k0, k1) = list(counter), key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & M32, (p0 >> 32) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c


def _draw(i, spec):
    i64 = i & 0xFFFFFFFFFFFFFFFF  # two's complement of the int64 index
    w = _philox((i64 & M32, i64 >> 32, spec.stream & M32, int(spec.epoch) & M32),
                (spec.seed & M32, (spec.seed >> 32) & M32))
    k = 2 * spec.pad + 1
    return (w[0] * k) >> 32, (w[1] * k) >> 32, int(spec.flip and (w[2] >> 31))


def _loop(value, fill, N, C, H, W, idx, spec):
    """out[b, c, y, x] by the contract, one pixel at a time; ``value(i, c, sy, sx)`` reads the source."""
    out = torch.empty(len(idx), C, H, W)
    for b, i in enumerate(idx):
        dx, dy, flip = _draw(i, spec)
        for c in range(C):
            for y in range(H):
                for x in range(W):
                    sy = y + dy - spec.pad
                    sx = (W - 1 - x if flip else x) + dx - spec.pad
                    inside = 0 <= i < N and 0 <= sy < H and 0 <= sx < W
                    out[b, c, y, x] = value(i, c, sy, sx) if inside else fill[c]
    return out


def _sources(N, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    u8 = torch.zeros(N, H, W, 4, dtype=torch.uint8)
    u8[..., :C] = torch.randint(0, 256, (N, H, W, C), generator=g, dtype=torch.uint8)
    lut = cifar_lut(torch.rand(C, generator=g), 0.2 + torch.rand(C, generator=g))
    f32 = torch.randn(N, C, H, W, generator=g)
    bf16 = torch.randn(N, H, W, C, generator=g).to(torch.bfloat16)
    return u8, lut, f32, bf16


def _expected(kind, srcs, N, C, H, W, idx, spec):
    u8, lut, f32, bf16 = srcs
    if kind == "u8":
        return _loop(lambda i, c, y, x: float(lut[c, int(u8[i, y, x, c])]), [float(lut[c, 0]) for c in range(C)],
                     N, C, H, W, idx, spec)
    if kind == "f32":
        return _loop(lambda i, c, y, x: float(f32[i, c, y, x]), [0.0] * C, N, C, H, W, idx, spec)
    return _loop(lambda i, c, y, x: float(bf16[i, y, x, c]), [0.0] * C, N, C, H, W, idx, spec)


def _src_of(kind, srcs):
    u8, lut, f32, bf16 = srcs
    return {"u8": (u8, lut), "f32": (f32, None), "bf16": (bf16, None)}[kind]


def _c8_of(nchw, c8):
    B, C, H, W = nchw.shape
    o = torch.zeros(B, H, W, c8, dtype=torch.bfloat16)
    o[..., :C] = nchw.permute(0, 2, 3, 1).to(torch.bfloat16)
    return o


# ---------------------------------------------------------------- 1. known answers
@pytest.mark.parametrize("i,want", [(0, (6, 8, 0)), (1, (3, 6, 1)), (49999, (2, 5, 1)), ((1 << 32) + 5, (0, 8, 0))])
def test_known_answers(i, want):
    spec = AugSpec(pad=4, flip=True, seed=SEED, stream=0, epoch=0)
    dx, dy, flip = draws(torch.tensor([i], dtype=torch.int64), spec)
    assert (int(dx), int(dy), int(flip)) == want
    assert _draw(i, spec) == want  # the test's own transcription agrees
    # a device-style epoch tensor draws the same
    dx, dy, flip = draws(torch.tensor([i]), spec.replace(epoch=torch.zeros(1, dtype=torch.int32)))
    assert (int(dx), int(dy), int(flip)) == want


# ---------------------------------------------------------------- 2. oracle == per-pixel loop
GEOMS = [(3, 8, 8, 2, True), (3, 10, 6, 3, True), (1, 28, 28, 2, True), (3, 8, 8, 0, True), (3, 8, 8, 4, False)]
FORMS = [("u8", None), ("f32", None), ("u8", 8), ("bf16", 8), ("bf16", None), ("f32", 8)]


@pytest.mark.parametrize("C,H,W,pad,flip", GEOMS, ids=lambda v: str(v))
def test_reference_matches_pixel_loop(C, H, W, pad, flip):
    N, idx = 7, [3, 0, 3, 6, 1]
    srcs = _sources(N, C, H, W, seed=C * 100 + H)
    spec = AugSpec(pad=pad, flip=flip, seed=SEED, stream=1, epoch=2)
    want = {k: _expected(k, srcs, N, C, H, W, idx, spec) for k in ("u8", "f32", "bf16")}
    if pad:  # the geometry does crop: some sample is shifted
        assert any(_draw(i, spec)[:2] != (pad, pad) for i in idx)
    for kind, c8 in FORMS:
        src, lut = _src_of(kind, srcs)
        got = augment_reference(src, torch.tensor(idx), spec, lut, c8=c8)
        if c8 is None:
            assert got.dtype == torch.float32 and got.shape == (5, C, H, W)
            assert torch.equal(got, want[kind]), (kind, c8)
        else:
            assert got.dtype == torch.bfloat16 and got.shape == (5, H, W, 8)
            assert torch.equal(got, _c8_of(want[kind], 8)), (kind, c8)
            assert (got[..., C:] == 0).all()  # pad channels exactly zero
        assert torch.equal(augment_gather(src, torch.tensor(idx), spec, lut, c8=c8), got)  # CPU dispatch


def test_out_of_range_index_gives_fill_image():
    N, C, H, W = 7, 3, 8, 8
    srcs = _sources(N, C, H, W, seed=5)
    spec = AugSpec(pad=2, flip=True, seed=SEED)
    idx = [-1, N, 2]
    for kind, c8 in FORMS:
        src, lut = _src_of(kind, srcs)
        got = augment_reference(src, torch.tensor(idx), spec, lut, c8=c8)
        fill = lut[:, 0] if kind == "u8" else torch.zeros(C)
        img = fill.view(1, C, 1, 1).expand(2, C, H, W)
        want = _expected(kind, srcs, N, C, H, W, idx, spec)
        assert torch.equal(want[:2], img)
        assert torch.equal(got, want if c8 is None else _c8_of(want, c8)), (kind, c8)


def test_pad0_noflip_is_a_plain_gather():
    N, C, H, W = 7, 3, 8, 8
    u8, lut, f32, bf16 = _sources(N, C, H, W, seed=9)
    idx = torch.tensor([6, 0, 0, 4])
    assert torch.equal(augment_reference(f32, idx, PLAIN), f32.index_select(0, idx))
    norm = torch.stack([lut[c][u8[..., c].long()] for c in range(C)], 1)
    assert torch.equal(augment_reference(u8, idx, PLAIN, lut), norm.index_select(0, idx))


def test_spec_is_validated():
    with pytest.raises(ValueError):
        AugSpec(pad=17)
    with pytest.raises(ValueError):
        AugSpec(pad=-1)
    with pytest.raises(ValueError):
        AugSpec(epoch=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError):
        augment_reference(torch.zeros(2, 8, 8, 4, dtype=torch.uint8), torch.tensor([0]), PLAIN)  # no lut


# ---------------------------------------------------------------- 3. draw statistics
@pytest.mark.parametrize("n,stream,epoch,pad", [(81000, 0, 0, 4), (81000, 1, 7, 4), (25000, 2, 3, 2)])
def test_draw_statistics(n, stream, epoch, pad):
    spec = AugSpec(pad=pad, flip=True, seed=SEED, stream=stream, epoch=epoch)
    dx, dy, flip = draws(torch.arange(n), spec)
    k = 2 * pad + 1
    assert int(dx.min()) == 0 and int(dx.max()) == k - 1 and int(dy.min()) == 0 and int(dy.max()) == k - 1
    cells = torch.bincount(dy * k + dx, minlength=k * k).double()
    p = 1.0 / (k * k)
    z = (cells - n * p).abs() / math.sqrt(n * p * (1 - p))
    zf = abs(int(flip.sum()) - n / 2) / math.sqrt(n / 4)
    print("cells worst %.2f sigma, flip %.2f sigma" % (float(z.max()), zf))
    assert float(z.max()) <= 4.0
    assert zf <= 4.0


# ---------------------------------------------------------------- 4. what the draw depends on
def test_draw_depends_on_index_stream_epoch_only():
    spec = AugSpec(pad=4, flip=True, seed=SEED, stream=0, epoch=0)
    idx = torch.arange(512)
    base = torch.stack(draws(idx, spec))
    assert not torch.equal(base, torch.stack(draws(idx, spec.replace(stream=1))))
    assert not torch.equal(base, torch.stack(draws(idx, spec.replace(epoch=1))))
    assert not torch.equal(base, torch.stack(draws(idx, spec.replace(seed=SEED + 1))))
    assert not torch.equal(base, torch.stack(draws(idx, spec.replace(seed=SEED + (1 << 32)))))
    assert torch.equal(base, torch.stack(draws(idx, spec.replace(epoch=torch.zeros(1, dtype=torch.int32)))))
    # batch position, batch size, order: the same image whatever batch it arrives in
    f32 = torch.randn(40, 3, 8, 8, generator=torch.Generator().manual_seed(3))
    spec = spec.replace(pad=2)
    whole = augment_reference(f32, torch.arange(40), spec)
    perm = torch.randperm(40, generator=torch.Generator().manual_seed(4))
    assert torch.equal(augment_reference(f32, perm, spec), whole[perm])
    assert torch.equal(augment_reference(f32, perm[5:12], spec), whole[perm[5:12]])
    assert torch.equal(augment_reference(f32, torch.tensor([17]), spec), whole[17:18])


# ---------------------------------------------------------------- 5. the loader
TRAIN_COUNTS = (7, 5, 30, 30, 28)  # records per data_batch_N.bin
TEST_COUNT = 40


def _write_cifar(base, seed=11, train_counts=TRAIN_COUNTS, test_count=TEST_COUNT):
    """Tiny CIFAR-10 binary files from a seed -> (train records, test records) as uint8 arrays."""
    os.makedirs(base, exist_ok=True)
    rng = np.random.RandomState(seed)

    def records(n):
        r = rng.randint(0, 256, size=(n, 3073)).astype(np.uint8)
        r[:, 0] = rng.randint(0, 10, size=n)
        return r

    train = [records(n) for n in train_counts]
    for j, r in enumerate(train):
        r.tofile(os.path.join(base, "data_batch_%d.bin" % (j + 1)))
    test = records(test_count)
    test.tofile(os.path.join(base, "test_batch.bin"))
    return np.concatenate(train), test


@pytest.fixture(scope="module")
def cifar_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("cifar")
    _write_cifar(str(d / "cifar-10-batches-bin"))
    return str(d)


@pytest.mark.parametrize("nested", [False, True])
def test_loader_reads_binary_version(tmp_path, nested):
    from katib_amd.workloads.data import CIFAR10_MEAN, CIFAR10_STD, cifar10_from_dir

    base = tmp_path / "cifar-10-batches-bin" if nested else tmp_path
    train, test = _write_cifar(str(base))
    for split, rec in (("train", train), ("test", test)):
        ds = cifar10_from_dir(str(tmp_path), "cpu", split)
        n = rec.shape[0]
        assert ds.n == n and ds.x.shape == (n, 32, 32, 4) and ds.x.dtype == torch.uint8
        assert ds.y.dtype == torch.int64 and np.array_equal(ds.y.numpy(), rec[:, 0].astype(np.int64))
        planar = rec[:, 1:].reshape(n, 3, 32, 32)
        assert np.array_equal(ds.x[..., :3].numpy(), planar.transpose(0, 2, 3, 1))
        assert (ds.x[..., 3] == 0).all()
        v = np.arange(256, dtype=np.float32) / np.float32(255)
        for c in range(3):
            want = (v - np.float32(CIFAR10_MEAN[c])) / np.float32(CIFAR10_STD[c])
            assert ds.lut.shape == (3, 256) and np.array_equal(ds.lut[c].numpy(), want)
    assert cifar10_from_dir(str(tmp_path), "cpu", "train", limit=9).n == 9
    # the first two files hold 7 and 5 records: record 7 is the first of data_batch_2.bin
    ds = cifar10_from_dir(str(tmp_path), "cpu", "train")
    assert int(ds.y[7]) == int(train[7, 0]) and sum(TRAIN_COUNTS[:2]) == 12


def test_loader_rejects_truncated_and_missing(tmp_path):
    from katib_amd.workloads.data import cifar10_from_dir

    with pytest.raises(ValueError, match="3073"):
        cifar10_from_dir(str(tmp_path), "cpu", "train")  # nothing there
    _write_cifar(str(tmp_path))
    os.remove(str(tmp_path / "data_batch_4.bin"))
    with pytest.raises(ValueError, match="data_batch_4.bin"):
        cifar10_from_dir(str(tmp_path), "cpu", "train")
    with open(str(tmp_path / "test_batch.bin"), "r+b") as f:
        f.truncate(3073 * 3 - 1)
    with pytest.raises(ValueError, match="3073"):
        cifar10_from_dir(str(tmp_path), "cpu", "test")
    with pytest.raises(ValueError):
        cifar10_from_dir(str(tmp_path), "cpu", "valid")


# ---------------------------------------------------------------- 6. the batch iterator
def test_batches_without_augment_is_index_select():
    from katib_amd.workloads.data import cifar10

    ds = cifar10("cpu", n=64)
    sub = ds.subset(8, 56)
    g = torch.Generator(device="cpu").manual_seed(3)
    perm = torch.randperm(48, generator=g) + 8
    got = list(sub.batches(16, seed=3, drop_last=True))
    assert len(got) == 3
    for s, (x, y) in enumerate(got):
        idx = perm[s * 16:(s + 1) * 16]
        assert torch.equal(x, ds.x.index_select(0, idx)) and torch.equal(y, ds.y.index_select(0, idx))


def test_batches_with_augment_matches_oracle_and_sharding():
    from katib_amd.workloads.data import cifar10

    ds = cifar10("cpu", n=64)
    sub = ds.subset(0, 64)
    spec = AugSpec(pad=4, flip=True, seed=2, stream=1, epoch=3)
    perm = torch.randperm(64, generator=torch.Generator(device="cpu").manual_seed(5))
    one = list(sub.batches(16, seed=5, drop_last=True, augment=spec))
    plain = list(sub.batches(16, seed=5, drop_last=True))
    assert len(one) == 4
    for s, ((x, y), (_, y0)) in enumerate(zip(one, plain)):
        idx = perm[s * 16:(s + 1) * 16]
        assert torch.equal(y, y0) and torch.equal(y, ds.y.index_select(0, idx))
        assert torch.equal(x, augment_reference(ds.x, idx, spec))
    assert not torch.equal(one[0][0], plain[0][0])
    shards = [list(sub.batches(8, seed=5, shard=r, num_shards=2, drop_last=True, augment=spec)) for r in (0, 1)]
    for s, (x, y) in enumerate(one):
        assert torch.equal(torch.cat([shards[0][s][0], shards[1][s][0]]), x)
        assert torch.equal(torch.cat([shards[0][s][1], shards[1][s][1]]), y)


def test_batches_on_u8_dataset_normalise(cifar_dir):
    from katib_amd.workloads.data import cifar10_from_dir

    ds = cifar10_from_dir(cifar_dir, "cpu", "train")
    x, y = next(ds.subset(0, 32).batches(8, seed=1))
    assert x.shape == (8, 3, 32, 32) and x.dtype == torch.float32
    idx = torch.randperm(32, generator=torch.Generator(device="cpu").manual_seed(1))[:8]
    want = torch.stack([ds.lut[c][ds.x[idx][..., c].long()] for c in range(3)], 1)
    assert torch.equal(x, want) and torch.equal(y, ds.y[idx])


# ---------------------------------------------------------------- 7, 8. the workloads on the CPU
RESNET_ARGS = ["--augment", "1", "--epochs", "1", "--num-train", "64", "--num-valid", "32", "--batch-size", "16",
               "--width", "8", "--step", "module"]


def test_resnet_trial_runs_augmented_on_cpu(capsys, cifar_dir):
    import re

    from katib_amd.workloads import resnet_cifar

    for extra in ([], ["--data-dir", cifar_dir]):
        acc = resnet_cifar.main(RESNET_ARGS + extra)
        out = capsys.readouterr().out
        losses = [float(m) for m in re.findall(r"loss=([^\s]+)", out)]
        assert len(losses) == 1 and math.isfinite(losses[0]), out
        assert 0.0 <= acc <= 1.0


def test_darts_trial_runs_on_fixture_on_cpu(capsys, cifar_dir):
    from katib_amd.workloads import darts_cifar10

    settings = '{"num_epochs": 1, "init_channels": 4, "num_nodes": 2, "batch_size": 8, "stem_multiplier": 1}'
    darts_cifar10.main(["--algorithm-settings", settings, "--num-layers", "1", "--max-steps", "1",
                        "--data-dir", cifar_dir, "--num-train", "96"])
    out = capsys.readouterr().out
    assert "Best-Genotype=Genotype(" in out, out


def test_darts_augment_flag_defaults():
    from katib_amd.workloads import darts_cifar10

    a = darts_cifar10.parse_args([])
    assert a.data_dir == "" and a.augment == "auto"
    assert darts_cifar10.parse_args(["--augment", "1"]).augment == "1"
    with pytest.raises(SystemExit):
        darts_cifar10.parse_args(["--augment", "2"])


# ---------------------------------------------------------------- 9. the example
def test_augment_example_loads_and_validates():
    from katib_amd.api.defaults import set_default
    from katib_amd.api.validation import validate_experiment
    from katib_amd.api.yaml_io import load_experiment

    e = set_default(load_experiment(os.path.join(ROOT, "examples", "nas", "darts-cifar10-augment.yaml")))
    validate_experiment(e)
    cmd = e.spec.trial_template.trial_spec["spec"]["template"]["spec"]["containers"][0]["command"]
    assert "--augment=1" in cmd and any(c.startswith("--data-dir=") for c in cmd)
    assert e.spec.algorithm.algorithm_name == "darts"
