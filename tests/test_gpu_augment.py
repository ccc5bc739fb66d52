"""The augmenting batch gather kernel (csrc/hip/augment.hip) against the torch oracle
(ops/augment.py: augment_reference, computed on the CPU), bit for bit; graph replay with a device
epoch; the fused ResNet step's augmented first launch; both workloads with the new flags."""
import math
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, B = 37, 9
IDX = [0, N - 1, 5, 5, 36, 17, 0, 23, 8]  # first, last, repeats
SEEDS = [(3 << 32) | 77, (0x9E3779B9 << 32) | 0x85EBCA6B]  # both key words non-zero
PAIRS = [(0, 0), (2, 5)]  # (stream, epoch)
GEOMS = [(3, 32, 32, 4, True), (1, 28, 28, 2, True), (3, 10, 6, 3, True), (3, 32, 32, 0, True), (3, 32, 32, 4, False)]
FORMS = [("u8", None), ("f32", None), ("u8", 8), ("bf16", 8)]


def _dev():
    return torch.device("cuda", 0)


def _sources(C, H, W, seed):
    from katib_amd.ops.augment import cifar_lut

    g = torch.Generator().manual_seed(seed)
    u8 = torch.zeros(N, H, W, 4, dtype=torch.uint8)
    u8[..., :C] = torch.randint(0, 256, (N, H, W, C), generator=g, dtype=torch.uint8)
    lut = cifar_lut(torch.rand(C, generator=g), 0.2 + torch.rand(C, generator=g))  # random means / stds
    f32 = torch.randn(N, C, H, W, generator=g)
    bf16 = torch.randn(N, H, W, C, generator=g).to(torch.bfloat16)
    return {"u8": (u8, lut), "f32": (f32, None), "bf16": (bf16, None)}


# ---------------------------------------------------------------- 1. kernel == oracle
@pytest.mark.parametrize("C,H,W,pad,flip", GEOMS, ids=lambda v: str(v))
def test_kernel_equals_oracle(C, H, W, pad, flip):
    from katib_amd.ops.augment import AugSpec, augment_gather, augment_reference, hip_supported

    dev = _dev()
    srcs = _sources(C, H, W, seed=7 * H + C)
    idx = torch.tensor(IDX)
    for seed, (stream, epoch) in zip(SEEDS, PAIRS):
        spec = AugSpec(pad=pad, flip=flip, seed=seed, stream=stream, epoch=epoch)
        for kind, c8 in FORMS:
            src, lut = srcs[kind]
            want = augment_reference(src, idx, spec, lut, c8=c8)
            dsrc, dlut = src.to(dev), None if lut is None else lut.to(dev)
            assert hip_supported(dsrc, c8)
            got = augment_gather(dsrc, idx.to(dev), spec, dlut, c8=c8)
            assert got.is_cuda and got.dtype == want.dtype and got.shape == want.shape
            assert torch.equal(got.cpu(), want), (kind, c8, seed, stream, epoch)
            # a device epoch tensor draws what the integer draws
            et = torch.full((1,), epoch, dtype=torch.int32, device=dev)
            got = augment_gather(dsrc, idx.to(dev), spec.replace(epoch=et), dlut, c8=c8)
            assert torch.equal(got.cpu(), want), (kind, c8, "device epoch")
    if pad:  # and the crop really moves pixels
        plain = augment_reference(srcs["f32"][0], idx, AugSpec(pad=0, flip=False))
        assert not torch.equal(plain, augment_reference(srcs["f32"][0], idx, spec))


def test_binding_rejects_bad_arguments():
    from katib_amd import _hipload

    k = _hipload.hipkern()
    dev = _dev()
    src = torch.zeros(4, 3, 8, 8, device=dev)
    idx = torch.zeros(2, dtype=torch.long, device=dev)
    out = torch.empty(2, 3, 8, 8, device=dev)
    k.augment_gather(src, None, idx, out, 2, True, 1, 2, 0, 0, None)
    with pytest.raises(RuntimeError, match="pad"):
        k.augment_gather(src, None, idx, out, 17, True, 1, 2, 0, 0, None)
    with pytest.raises(RuntimeError):
        k.augment_gather(src, None, idx, torch.empty(2, 3, 8, 9, device=dev), 2, True, 1, 2, 0, 0, None)
    with pytest.raises(RuntimeError, match="C8"):
        k.augment_gather(src.to(torch.bfloat16), None, idx, torch.empty(2, 4, 8, 12, device=dev, dtype=torch.bfloat16),
                         2, True, 1, 2, 0, 0, None)
    with pytest.raises(RuntimeError, match="aligned"):
        k.augment_gather(src, None, idx, torch.empty(2 * 3 * 8 * 8 + 1, device=dev)[1:].view(2, 3, 8, 8), 2, True,
                         1, 2, 0, 0, None)
    with pytest.raises(RuntimeError, match="lut"):
        k.augment_gather(torch.zeros(4, 8, 8, 4, dtype=torch.uint8, device=dev), None, idx, out, 2, True, 1, 2, 0, 0,
                         None)
    with pytest.raises(RuntimeError):
        k.augment_gather(src, None, idx.int(), out, 2, True, 1, 2, 0, 0, None)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 2. graph replay
def test_graph_replays_with_new_epoch_and_indices():
    from katib_amd.ops.augment import AugSpec, augment_gather, augment_reference

    dev = _dev()
    src, _ = _sources(3, 32, 32, seed=3)["f32"]
    dsrc = src.to(dev)
    epoch_t = torch.zeros(1, dtype=torch.int32, device=dev)
    idx = torch.zeros(B, dtype=torch.long, device=dev)
    out = torch.empty(B, 3, 32, 32, device=dev)
    spec = AugSpec(pad=4, flip=True, seed=SEEDS[1], stream=1, epoch=epoch_t)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        augment_gather(dsrc, idx, spec, out=out)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        augment_gather(dsrc, idx, spec, out=out)
    outs = {}
    same_idx = torch.tensor(IDX)
    for e, batch in ((0, same_idx), (1, same_idx), (5, torch.arange(B) * 4)):
        epoch_t.fill_(e)
        idx.copy_(batch)
        graph.replay()
        outs[e] = out.cpu().clone()
        assert torch.equal(outs[e], augment_reference(src, batch, spec.replace(epoch=e))), e
    assert not torch.equal(outs[0], outs[1])


# ---------------------------------------------------------------- 3. the fused ResNet step
def _model(width, dev):
    from katib_amd.ops import batchnorm as hbn
    from katib_amd.ops import conv as hconv
    from katib_amd.workloads import resnet_cifar as rc

    torch.manual_seed(0)
    rc.Conv, rc.BN = hconv.Conv2d, hbn.BatchNorm2d
    return rc.ResNet18(width).to(dev).to(memory_format=torch.channels_last).train()


@pytest.mark.parametrize("kind", ["bf16", "u8"])
def test_fused_resnet_step_augments_its_first_launch(kind):
    import copy

    from katib_amd.ops.augment import AugSpec, augment_reference, cifar_lut
    from katib_amd.ops.resnet_step import FusedResNetStep
    from katib_amd.workloads.common import CapturedStep

    dev = _dev()
    n = 24
    g = torch.Generator().manual_seed(1)
    ty = torch.randint(0, 10, (n,), generator=g).to(dev)
    if kind == "bf16":
        tx = torch.randn(n, 3, 32, 32, generator=g).to(dev).to(torch.bfloat16).contiguous(
            memory_format=torch.channels_last)
        src, lut, kw = tx.permute(0, 2, 3, 1), None, {}
    else:
        tx = None
        src = torch.zeros(n, 32, 32, 4, dtype=torch.uint8)
        src[..., :3] = torch.randint(0, 256, (n, 32, 32, 3), generator=g, dtype=torch.uint8)
        src, lut = src.to(dev), cifar_lut((0.49, 0.48, 0.45), (0.25, 0.24, 0.26)).to(dev)
        kw = {"src": (src, lut)}
    epoch_t = torch.zeros(1, dtype=torch.int32, device=dev)
    spec = AugSpec(pad=4, flip=True, seed=(5 << 32) | 9, stream=0, epoch=epoch_t)
    ours = _model(16, dev)
    twin = copy.deepcopy(ours)
    idx = torch.tensor([3, 0, 23, 7, 7, 12, 19, 1], device=dev)
    loss_buf = torch.zeros((), device=dev)
    fused = FusedResNetStep(ours, tx, ty, idx, loss_buf, 0.05, 0.9, 5e-4, aug=spec, **kw)
    fused.step()
    want_x0 = augment_reference(src, idx, spec, lut, c8=8)
    assert torch.equal(fused.x0, want_x0)
    # the same step without aug on a data set the oracle augmented beforehand (the draw is keyed by
    # data-set index, so image i of that set is what the augmented step reads for index i)
    pre = augment_reference(src, torch.arange(n, device=dev), spec, lut).to(torch.bfloat16).contiguous(
        memory_format=torch.channels_last)
    loss_twin = torch.zeros((), device=dev)
    plain = FusedResNetStep(twin, pre, ty, idx, loss_twin, 0.05, 0.9, 5e-4)
    plain.step()
    assert torch.equal(plain.x0, fused.x0)
    a, b = float(loss_buf), float(loss_twin)
    print("loss augmented step %.9g, pre-augmented twin %.9g" % (a, b))
    # identical inputs and weights, but not compared bitwise: the head's pooled sums add through LDS
    # float atomics (rn_head), whose order is not fixed from launch to launch; the bound is the loss
    # tolerance of tests/test_gpu_resnet_step.py
    assert math.isfinite(a) and abs(a - b) < 0.03 * abs(b) + 1e-3, (a, b)
    # captured: one eager warm-up, then three replays at epochs 0, 0, 1 with fresh indices
    step = CapturedStep(fused.step, warmup=1)
    step()
    batches = [torch.arange(8), torch.arange(8, 16), torch.tensor([23, 22, 0, 5, 5, 9, 16, 2])]
    for e, batch in zip((0, 0, 1), batches):
        epoch_t.fill_(e)
        idx.copy_(batch.to(dev))
        before = float(loss_buf)
        step()
        assert math.isfinite(float(loss_buf) - before)
    assert step.graph is not None
    assert torch.equal(fused.x0, augment_reference(src, idx, spec.replace(epoch=1), lut, c8=8))
    assert not torch.equal(fused.x0, augment_reference(src, idx, spec.replace(epoch=0), lut, c8=8))


def test_fused_resnet_step_u8_needs_aug():
    from katib_amd.ops.resnet_step import FusedResNetStep

    dev = _dev()
    src = torch.zeros(8, 32, 32, 4, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError):
        FusedResNetStep(_model(8, dev), None, torch.zeros(8, dtype=torch.long, device=dev),
                        torch.arange(8, device=dev), torch.zeros((), device=dev), 0.1, 0.9, 0.0,
                        src=(src, torch.zeros(3, 256, device=dev)))


# ---------------------------------------------------------------- 4, 5. the workloads
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


@pytest.mark.parametrize("augment", ["1", "0"])
def test_darts_trial_on_fixture_hip_backend(capsys, cifar_dir, augment):
    from katib_amd.ops import darts as dops
    from katib_amd.workloads import darts_cifar10

    settings = '{"num_epochs": 1, "init_channels": 4, "num_nodes": 3, "batch_size": 16, "stem_multiplier": 1}'
    before = dops.backend()
    try:
        darts_cifar10.main(["--algorithm-settings", settings, "--num-layers", "2", "--max-steps", "2",
                            "--data-dir", cifar_dir, "--augment", augment, "--ops", "hip"])
    finally:
        dops.set_backend(before)
    out = capsys.readouterr().out
    assert "Best-Genotype=Genotype(" in out, out


def test_resnet_trial_augmented_fused_step(capsys, cifar_dir):
    from katib_amd.workloads import resnet_cifar

    args = ["--augment", "1", "--step", "fused", "--epochs", "1", "--max-steps", "3", "--width", "16",
            "--batch-size", "32", "--num-train", "96", "--num-valid", "32"]
    for extra in ([], ["--data-dir", cifar_dir]):
        resnet_cifar.main(args + extra)
        out = capsys.readouterr().out
        losses = [float(m) for m in re.findall(r"loss=([^\s]+)", out)]
        assert len(losses) == 1 and math.isfinite(losses[0]), out


def test_resnet_trial_augmented_module_step_captures(capsys):
    """--step module draws through the torch oracle inside the captured step (device epoch)."""
    from katib_amd.workloads import resnet_cifar

    resnet_cifar.main(["--augment", "1", "--step", "module", "--epochs", "2", "--max-steps", "5", "--width", "8",
                       "--batch-size", "16", "--num-train", "96", "--num-valid", "32"])
    out = capsys.readouterr().out
    losses = [float(m) for m in re.findall(r"loss=([^\s]+)", out)]
    assert len(losses) == 2 and all(math.isfinite(v) for v in losses), out
