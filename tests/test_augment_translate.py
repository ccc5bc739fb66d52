"""Translation mode of the augmenting gather (ops/augment.py: flip + fractional translation,
bilinear taps, reflected borders), its unpadded channels-last destination and the ENAS child's
``--data-dir`` / ``--augment`` flags, on the CPU: the oracle against a per-pixel transcription of
the contract in plain ints and numpy.float32 scalars, direction and exactness on a ramp, the draw's
properties, argument validation, and the child trial on a seeded fixture directory."""
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from katib_amd.ops.augment import AugSpec, augment_gather, augment_reference, cifar_lut, draws_translate

SEED = (3 << 32) | 77
M32 = 0xFFFFFFFF
F = np.float32


# ---------------------------------------------------------------- the contract, in plain Python
def _philox(counter, key):
    c, (k0, k1) = list(counter), key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & M32, (p0 >> 32) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c


def _draw(i, spec, H, W):
    i64 = i & 0xFFFFFFFFFFFFFFFF  # two's complement of the int64 index
    w = _philox((i64 & M32, i64 >> 32, spec.stream & M32, int(spec.epoch) & M32),
                (spec.seed & M32, (spec.seed >> 32) & M32))
    rx, ry = math.floor(spec.translate * W * 256), math.floor(spec.translate * H * 256)
    return ((w[0] * (2 * rx + 1)) >> 32) - rx, ((w[1] * (2 * ry + 1)) >> 32) - ry, int(spec.flip and (w[2] >> 31))


def _refl(k, n):
    return -1 - k if k < 0 else (2 * n - 1 - k if k >= n else k)


def _loop(value, fill, N, C, H, W, idx, spec):
    """out[b, c, y, x] by the contract, one pixel at a time, every * and + one numpy.float32
    operation; ``value(i, c, row, col)`` reads the source as a numpy.float32."""
    out = np.empty((len(idx), C, H, W), dtype=np.float32)
    for b, i in enumerate(idx):
        tx, ty, flip = _draw(i, spec, H, W)
        for c in range(C):
            for y in range(H):
                for x in range(W):
                    if not 0 <= i < N:
                        out[b, c, y, x] = fill[c]
                        continue
                    u, v = 256 * x - tx, 256 * y - ty
                    x0, fx, y0, fy = u >> 8, u & 255, v >> 8, v & 255
                    col = (lambda k: W - 1 - _refl(k, W)) if flip else (lambda k: _refl(k, W))
                    a, bb = value(i, c, _refl(y0, H), col(x0)), value(i, c, _refl(y0, H), col(x0 + 1))
                    e, d = value(i, c, _refl(y0 + 1, H), col(x0)), value(i, c, _refl(y0 + 1, H), col(x0 + 1))
                    top = F(F((256 - fy) * (256 - fx)) * a) + F(F((256 - fy) * fx) * bb)
                    bot = F(F(fy * (256 - fx)) * e) + F(F(fy * fx) * d)
                    out[b, c, y, x] = F(F(top) + F(bot)) * F(2.0 ** -16)
    return torch.from_numpy(out)


def _sources(N, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    u8 = torch.zeros(N, H, W, 4, dtype=torch.uint8)
    u8[..., :C] = torch.randint(0, 256, (N, H, W, C), generator=g, dtype=torch.uint8)
    lut = cifar_lut(torch.rand(C, generator=g), 0.2 + torch.rand(C, generator=g))
    bf16 = torch.randn(N, H, W, C, generator=g).to(torch.bfloat16)
    return {"u8": (u8, lut), "bf16": (bf16, None)}


def _expected(kind, srcs, N, C, H, W, idx, spec):
    src, lut = srcs[kind]
    if kind == "u8":
        ln = lut.numpy()
        return _loop(lambda i, c, y, x: ln[c, int(src[i, y, x, c])], [ln[c, 0] for c in range(C)], N, C, H, W, idx, spec)
    sf = src.float().numpy()
    return _loop(lambda i, c, y, x: sf[i, y, x, c], [F(0)] * C, N, C, H, W, idx, spec)


def _c8_of(nchw, c8):
    B, C, H, W = nchw.shape
    o = torch.zeros(B, H, W, c8, dtype=torch.bfloat16)
    o[..., :C] = nchw.permute(0, 2, 3, 1).to(torch.bfloat16)
    return o


# ---------------------------------------------------------------- 1. oracle == per-pixel loop
GEOMS = [(3, 8, 8, 0.1, True), (1, 5, 7, 0.5, True), (3, 6, 4, 0.25, False)]


@pytest.mark.parametrize("C,H,W,translate,flip", GEOMS, ids=lambda v: str(v))
def test_reference_matches_pixel_loop(C, H, W, translate, flip):
    N, idx = 7, [3, 0, 3, 6, 1, 5]
    srcs = _sources(N, C, H, W, seed=C * 100 + H)
    spec = AugSpec(pad=0, flip=flip, translate=translate, seed=SEED, stream=1, epoch=2)
    dr = [_draw(i, spec, H, W) for i in idx]
    assert any(t[0] & 255 and t[1] & 255 for t in dr)  # some sample interpolates in both directions
    for kind in ("u8", "bf16"):
        src, lut = srcs[kind]
        want = _expected(kind, srcs, N, C, H, W, idx, spec)
        it = torch.tensor(idx)
        got = augment_reference(src, it, spec, lut)
        assert got.dtype == torch.float32 and got.shape == (len(idx), C, H, W)
        assert torch.equal(got, want), kind
        got8 = augment_reference(src, it, spec, lut, c8=8)
        assert got8.dtype == torch.bfloat16 and torch.equal(got8, _c8_of(want, 8)), kind
        goth = augment_reference(src, it, spec, lut, nhwc=True)
        assert goth.dtype == torch.bfloat16 and goth.shape == (len(idx), H, W, C) and goth.is_contiguous()
        assert torch.equal(goth, want.permute(0, 2, 3, 1).to(torch.bfloat16)), kind
        for kw in ({}, {"c8": 8}, {"nhwc": True}):  # CPU dispatch, with and without a static buffer
            ref = augment_reference(src, it, spec, lut, **kw)
            assert torch.equal(augment_gather(src, it, spec, lut, **kw), ref)
            buf = torch.empty_like(ref)
            assert augment_gather(src, it, spec, lut, out=buf, **kw) is buf and torch.equal(buf, ref)


def test_nhwc_destination_in_crop_and_plain_mode():
    """nhwc is the NCHW result, channels last, rounded to bf16 - for every source, crop and plain."""
    N, C, H, W = 7, 3, 8, 8
    g = torch.Generator().manual_seed(9)
    srcs = dict(_sources(N, C, H, W, seed=4), f32=(torch.randn(N, C, H, W, generator=g), None))
    idx = torch.tensor([6, 0, 2, 2, -1, N])
    for spec in (AugSpec(pad=2, flip=True, seed=SEED, epoch=3), AugSpec(pad=0, flip=False)):
        for kind, (src, lut) in srcs.items():
            nchw = augment_reference(src, idx, spec, lut)
            got = augment_reference(src, idx, spec, lut, nhwc=True)
            assert got.shape == (6, H, W, C) and got.dtype == torch.bfloat16
            assert torch.equal(got, nchw.permute(0, 2, 3, 1).to(torch.bfloat16)), kind
            assert torch.equal(augment_gather(src, idx, spec, lut, nhwc=True), got)
    # the child's view of it: the channels-last NCHW tensor index_select gives today
    src = srcs["bf16"][0]
    got = augment_reference(src, idx[:4], AugSpec(pad=0, flip=False), nhwc=True).permute(0, 3, 1, 2)
    assert torch.equal(got, src.permute(0, 3, 1, 2).index_select(0, idx[:4]))
    assert got.is_contiguous(memory_format=torch.channels_last)


# ---------------------------------------------------------------- 2. direction and exactness
def test_ramp_moves_by_tx_and_mirrors_exactly():
    """byte = 4 x in every row and lut[c][v] = v: away from reflected taps the output is exactly
    4 x - tx / 64 (flip = 0) or the mirrored ramp 4 (W - 1 - x) + tx / 64 (flip = 1); every sum is
    an integer below 2^24, so fp32 is exact."""
    N, C, H, W = 64, 3, 4, 32
    u8 = torch.zeros(N, H, W, 4, dtype=torch.uint8)
    u8[..., :C] = (4 * torch.arange(W, dtype=torch.uint8)).view(1, 1, W, 1)
    lut = torch.arange(256, dtype=torch.float32).repeat(C, 1)
    spec = AugSpec(pad=0, flip=True, translate=0.1, seed=SEED, stream=0, epoch=1)
    idx = torch.arange(N)
    tx, ty, flip = draws_translate(idx, spec, H, W)
    out = augment_reference(u8, idx, spec, lut)
    flips, signs, checked = set(), set(), 0
    for b in range(N):
        t, f = int(tx[b]), int(flip[b])
        flips.add(f)
        signs.add((t > 0) - (t < 0))
        for x in range(W):
            x0 = (256 * x - t) >> 8
            if x0 < 0 or x0 + 1 > W - 1:
                continue  # a reflected tap
            want = 4 * (W - 1 - x) + t / 64 if f else 4 * x - t / 64
            assert (out[b, :, :, x] == want).all(), (b, x, t, f)
            checked += 1
    assert flips == {0, 1} and {-1, 1} <= signs and checked > N * (W - 8)


def test_constant_image_stays_constant():
    N, C, H, W = 40, 3, 6, 10
    u8 = torch.zeros(N, H, W, 4, dtype=torch.uint8)
    u8[..., :C] = torch.tensor([200, 3, 255], dtype=torch.uint8)
    lut = torch.arange(256, dtype=torch.float32).repeat(C, 1)
    bf = torch.full((N, H, W, C), 1.5, dtype=torch.bfloat16)
    for tr in (0.1, 0.5):
        spec = AugSpec(pad=0, flip=True, translate=tr, seed=SEED, stream=3, epoch=4)
        out = augment_reference(u8, torch.arange(N), spec, lut)
        assert torch.equal(out, torch.tensor([200.0, 3.0, 255.0]).view(1, C, 1, 1).expand(N, C, H, W))
        assert (augment_reference(bf, torch.arange(N), spec, nhwc=True) == 1.5).all()


def test_whole_pixel_draw_returns_the_tap_exactly():
    """translate so small that rx = ry = 0: tx = ty = 0, fx = fy = 0, the result is the (flipped) image."""
    N, C, H, W = 16, 3, 8, 8
    src, lut = _sources(N, C, H, W, seed=2)["u8"]
    idx = torch.arange(N)
    tiny = AugSpec(pad=0, flip=True, translate=1e-4, seed=SEED)
    tx, ty, flip = draws_translate(idx, tiny, H, W)
    assert not tx.any() and not ty.any() and flip.any()
    assert torch.equal(augment_reference(src, idx, tiny, lut), augment_reference(src, idx, tiny.replace(translate=0.0), lut))


# ---------------------------------------------------------------- 3. the draw
def test_draws_translate_properties():
    spec = AugSpec(pad=0, flip=True, translate=0.1, seed=SEED, stream=0, epoch=0)
    idx = torch.arange(4096)
    tx, ty, flip = draws_translate(idx, spec)  # 32 x 32 by default
    rx = ry = 819  # floor(0.1 * 32 * 256)
    assert int(tx.min()) >= -rx and int(tx.max()) <= rx and int(ty.min()) >= -ry and int(ty.max()) <= ry
    assert int(tx.min()) < -rx // 2 and int(tx.max()) > rx // 2 and int(ty.min()) < -ry // 2 and int(ty.max()) > ry // 2
    assert 0.4 < float(flip.float().mean()) < 0.6
    for b in (0, 1, 4095):  # the test's own transcription agrees
        assert (int(tx[b]), int(ty[b]), int(flip[b])) == _draw(b, spec, 32, 32)
    # a rectangular image scales each range by its own size
    txr, tyr, _ = draws_translate(idx, spec.replace(translate=0.5), 5, 7)
    assert int(txr.abs().max()) <= 128 * 7 and int(tyr.abs().max()) <= 128 * 5 and int(txr.abs().max()) > 128 * 5
    # a function of the data-set index only: batch order and duplicates do not matter
    perm = torch.randperm(4096, generator=torch.Generator().manual_seed(1))
    pick = torch.cat([perm[:100], perm[:100]])
    for got, full in zip(draws_translate(pick, spec), (tx, ty, flip)):
        assert torch.equal(got, full[pick])
    # epochs and streams draw differently; a device-style epoch tensor draws what the int draws
    assert not torch.equal(draws_translate(idx, spec.replace(epoch=1))[0], tx)
    assert not torch.equal(draws_translate(idx, spec.replace(stream=1))[0], tx)
    et = torch.full((1,), 1, dtype=torch.int32)
    assert torch.equal(draws_translate(idx, spec.replace(epoch=et))[0], draws_translate(idx, spec.replace(epoch=1))[0])
    assert not draws_translate(idx, spec.replace(flip=False))[2].any()


def test_spec_and_destination_are_validated():
    for kw in ({"translate": 0.1, "pad": 4}, {"translate": 0.1, "pad": 1}, {"translate": 0.51, "pad": 0},
               {"translate": -0.1, "pad": 0}):
        with pytest.raises(ValueError):
            AugSpec(**kw)
    AugSpec(pad=0, translate=0.5)
    assert AugSpec().translate == 0.0  # crop mode stays the default
    src = torch.zeros(2, 4, 4, 3, dtype=torch.bfloat16)
    for fn in (augment_reference, augment_gather):
        with pytest.raises(ValueError):
            fn(src, torch.tensor([0]), AugSpec(pad=0), c8=8, nhwc=True)


def test_out_of_range_index_gives_fill_image():
    N, C, H, W = 7, 3, 8, 8
    srcs = _sources(N, C, H, W, seed=5)
    spec = AugSpec(pad=0, flip=True, translate=0.25, seed=SEED)
    idx = torch.tensor([-1, N, 2])
    for kind, (src, lut) in srcs.items():
        fill = lut[:, 0] if kind == "u8" else torch.zeros(C)
        img = fill.view(1, C, 1, 1).expand(2, C, H, W)
        got = augment_reference(src, idx, spec, lut)
        assert torch.equal(got[:2], img) and not torch.equal(got[2], img[0])
        assert torch.equal(augment_reference(src, idx, spec, lut, nhwc=True)[:2],
                           img.permute(0, 2, 3, 1).to(torch.bfloat16))
        assert torch.equal(augment_reference(src, idx, spec, lut, c8=8)[:2], _c8_of(img, 8))


# ---------------------------------------------------------------- 4. the ENAS child
@pytest.fixture(scope="module")
def cifar_dir(tmp_path_factory):
    """A tiny CIFAR-10 binary version from a seed: 5 x 24 train records, 40 test records."""
    d = tmp_path_factory.mktemp("cifar") / "cifar-10-batches-bin"
    os.makedirs(str(d))
    rng = np.random.RandomState(11)
    for name, n in [("data_batch_%d.bin" % j, 24) for j in range(1, 6)] + [("test_batch.bin", 40)]:
        r = rng.randint(0, 256, size=(n, 3073)).astype(np.uint8)
        r[:, 0] = rng.randint(0, 10, size=n)
        r.tofile(str(d / name))
    return str(d.parent)


EMB = {"0": {"opt_type": "convolution", "opt_id": 0, "filter_size": "3", "num_filter": "8", "stride": "2"},
       "1": {"opt_type": "separable_convolution", "opt_id": 1, "filter_size": "3", "num_filter": "8", "stride": "1",
             "depth_multiplier": "1"}}
NN_CONFIG = {"num_layers": 2, "input_sizes": [32, 32, 3], "output_sizes": [10], "embedding": EMB}
ARCH = [[0], [1, 0]]  # a convolution first, then a separable convolution without a skip


@pytest.mark.parametrize("augment", ["1", "0"])
def test_enas_child_runs_on_fixture(capsys, cifar_dir, augment):
    from katib_amd.workloads import enas_child

    va = enas_child.main(["--architecture", json.dumps(ARCH), "--nn_config", json.dumps(NN_CONFIG), "--num_epochs", "1",
                          "--batch-size", "16", "--num-train", "96", "--num-valid", "32", "--data-dir", cifar_dir,
                          "--augment", augment])
    out = capsys.readouterr().out
    for name in ("Training-Accuracy", "Training-Loss", "Validation-Accuracy", "Validation-Loss"):
        vals = [float(m) for m in re.findall(r"^%s=(\S+)$" % name, out, flags=re.M)]
        assert len(vals) == 1 and math.isfinite(vals[0]), (name, out)
    assert 0.0 <= va <= 1.0


def test_enas_child_flags_select_the_gather(cifar_dir):
    from katib_amd.ops.augment import PLAIN
    from katib_amd.workloads.enas_child import ChildTrainer, parse_args

    a = parse_args([])
    assert a.data_dir == "" and a.augment == "auto"
    plain = ChildTrainer(ARCH, NN_CONFIG, num_train=64, num_valid=32, batch_size=16)
    assert not hasattr(plain, "xb") and plain.epoch_t is None  # today's index_select step
    # synthetic data, augmentation on: the static buffer holds the oracle's batch of the last step
    tr = ChildTrainer(ARCH, NN_CONFIG, num_train=64, num_valid=32, batch_size=16, seed=5, augment=True)
    assert tr.xb.shape == (16, 32, 32, 3) and tr.xb.dtype == torch.bfloat16
    assert tr.epoch_t.dtype == torch.int32 and tr.epoch_t.numel() == 1
    tr.epoch_t.fill_(2)
    idx = torch.arange(16) * 3
    tr.step(idx)
    spec = AugSpec(pad=0, flip=True, translate=0.1, seed=5, stream=0, epoch=2)
    assert torch.equal(tr.xb, augment_reference(tr.src, idx, spec, nhwc=True))
    assert not torch.equal(tr.xb, augment_reference(tr.src, idx, PLAIN, nhwc=True))
    assert math.isfinite(float(tr.acc_buf[0]))
    # the fixture directory without augmentation: bytes / 255 through the table, test split for validation
    td = ChildTrainer(ARCH, NN_CONFIG, num_train=96, num_valid=32, batch_size=16, data_dir=cifar_dir, augment=False)
    assert td.epoch_t is None and td.ty.numel() == 96 and td.vy.numel() == 32
    td.step(idx)
    want = (td.src[idx][..., :3].float() / 255.0).to(torch.bfloat16)
    assert torch.equal(td.xb, want)
    vl, va = td.validate(32)
    assert math.isfinite(vl) and 0.0 <= va <= 1.0


# ---------------------------------------------------------------- 5. the example
def test_augment_example_loads_and_validates():
    from katib_amd.api.defaults import set_default
    from katib_amd.api.validation import validate_experiment
    from katib_amd.api.yaml_io import load_experiment

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = set_default(load_experiment(os.path.join(root, "examples", "nas", "enas-cifar10-augment.yaml")))
    validate_experiment(e)
    spec = e.spec.trial_template.trial_spec["spec"]
    assert spec["entrypoint"] == "katib_amd.workloads.enas_child:main"
    assert "--augment=1" in spec["args"] and "--data-dir=/data" in spec["args"]
    assert e.spec.algorithm.algorithm_name == "enas"
