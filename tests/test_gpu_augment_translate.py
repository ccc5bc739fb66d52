"""The augmenting gather's NHWC kernels (csrc/hip/augment.hip: augment_nhwc_k, plain / crop and
translation mode) against the torch oracle computed on the CPU, bit for bit; the translate forms
without a kernel; graph replay with a device epoch; the binding's new arguments; the ENAS child's
captured step with the augmentation inside it."""
import json
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
# (3, 10, 6): H * W * C = 180 is no multiple of 8, the per-pixel path; 0.5: the deepest reflection
GEOMS = [(3, 32, 32, 0.1, True), (1, 28, 28, 0.1, True), (3, 10, 6, 0.25, True), (3, 32, 32, 0.5, True),
         (3, 32, 32, 0.1, False)]


def _dev():
    return torch.device("cuda", 0)


def _sources(C, H, W, seed):
    from katib_amd.ops.augment import cifar_lut

    g = torch.Generator().manual_seed(seed)
    u8 = torch.zeros(N, H, W, 4, dtype=torch.uint8)
    u8[..., :C] = torch.randint(0, 256, (N, H, W, C), generator=g, dtype=torch.uint8)
    lut = cifar_lut(torch.rand(C, generator=g), 0.2 + torch.rand(C, generator=g))  # random means / stds
    bf16 = torch.randn(N, H, W, C, generator=g).to(torch.bfloat16)
    return {"u8": (u8, lut), "bf16": (bf16, None)}


# ---------------------------------------------------------------- 1. kernel == oracle
@pytest.mark.parametrize("C,H,W,translate,flip", GEOMS, ids=lambda v: str(v))
def test_kernel_equals_oracle(C, H, W, translate, flip):
    from katib_amd.ops.augment import AugSpec, augment_gather, augment_reference, hip_supported

    dev = _dev()
    srcs = _sources(C, H, W, seed=7 * H + C)
    idx = torch.tensor(IDX + [-1, N])  # and two indices outside the set: the fill image
    for seed, (stream, epoch) in zip(SEEDS, PAIRS):
        specs = [AugSpec(pad=0, flip=flip, translate=translate, seed=seed, stream=stream, epoch=epoch),
                 AugSpec(pad=4, flip=flip, seed=seed, stream=stream, epoch=epoch),  # crop and plain into NHWC
                 AugSpec(pad=0, flip=flip, seed=seed, stream=stream, epoch=epoch)]
        for spec in specs:
            for kind, (src, lut) in srcs.items():
                want = augment_reference(src, idx, spec, lut, nhwc=True)
                dsrc, dlut = src.to(dev), None if lut is None else lut.to(dev)
                assert hip_supported(dsrc, None, True, spec)
                got = augment_gather(dsrc, idx.to(dev), spec, dlut, nhwc=True)
                assert got.is_cuda and got.dtype == torch.bfloat16 and got.shape == (len(idx), H, W, C)
                bad = (got.cpu() != want).sum().item()
                print("%s translate %.2f pad %d seed %x: %d of %d elements differ" % (kind, spec.translate, spec.pad,
                                                                                      seed, bad, want.numel()))
                assert torch.equal(got.cpu(), want), (kind, spec)
                # a device epoch tensor draws what the integer draws
                et = torch.full((1,), epoch, dtype=torch.int32, device=dev)
                got = augment_gather(dsrc, idx.to(dev), spec.replace(epoch=et), dlut, nhwc=True)
                assert torch.equal(got.cpu(), want), (kind, spec, "device epoch")
    # and the translation really moves pixels
    src, lut = srcs["u8"]
    assert not torch.equal(augment_reference(src, idx, specs[0], lut, nhwc=True),
                           augment_reference(src, idx, specs[2].replace(flip=False), lut, nhwc=True))


@pytest.mark.parametrize("C,H,W", [(2, 4, 8), (4, 6, 6), (5, 8, 8), (8, 5, 3), (16, 3, 3)], ids=lambda v: str(v))
def test_kernel_equals_oracle_other_channel_counts(C, H, W):
    """H * W * C a multiple of 8 with 2, 4 and more channels: an 8-element span covers from 5 pixels
    down to a part of one, and the last span ends at the last pixel. u8 holds at most 4 channels."""
    from katib_amd.ops.augment import AugSpec, augment_gather, augment_reference

    dev = _dev()
    g = torch.Generator().manual_seed(C)
    srcs = _sources(C, H, W, seed=C) if C <= 4 else {
        "bf16": (torch.randn(N, H, W, C, generator=g).to(torch.bfloat16), None)}
    idx = torch.tensor(IDX)
    for spec in (AugSpec(pad=0, flip=True, translate=0.25, seed=SEEDS[0], stream=1, epoch=2),
                 AugSpec(pad=1, flip=True, seed=SEEDS[0], stream=1, epoch=2)):
        for kind, (src, lut) in srcs.items():
            want = augment_reference(src, idx, spec, lut, nhwc=True)
            got = augment_gather(src.to(dev), idx.to(dev), spec, None if lut is None else lut.to(dev), nhwc=True)
            assert torch.equal(got.cpu(), want), (kind, spec)


def test_translate_forms_without_a_kernel_return_the_reference():
    from katib_amd.ops.augment import AugSpec, augment_gather, augment_reference, hip_supported

    dev = _dev()
    srcs = _sources(3, 32, 32, seed=11)
    idx = torch.tensor(IDX)
    spec = AugSpec(pad=0, flip=True, translate=0.1, seed=SEEDS[0], stream=1, epoch=3)
    for kind, (src, lut) in srcs.items():
        dsrc, dlut = src.to(dev), None if lut is None else lut.to(dev)
        for c8 in (None, 8):
            assert not hip_supported(dsrc, c8, False, spec)
            got = augment_gather(dsrc, idx.to(dev), spec, dlut, c8=c8)
            assert got.is_cuda
            assert torch.equal(got.cpu(), augment_reference(src, idx, spec, lut, c8=c8)), (kind, c8)


# ---------------------------------------------------------------- 2. graph replay
def test_graph_replays_with_new_epoch_and_indices():
    from katib_amd.ops.augment import AugSpec, augment_gather, augment_reference

    dev = _dev()
    src, lut = _sources(3, 32, 32, seed=3)["u8"]
    dsrc, dlut = src.to(dev), lut.to(dev)
    epoch_t = torch.zeros(1, dtype=torch.int32, device=dev)
    idx = torch.zeros(B, dtype=torch.long, device=dev)
    out = torch.empty(B, 32, 32, 3, device=dev, dtype=torch.bfloat16)
    spec = AugSpec(pad=0, flip=True, translate=0.1, seed=SEEDS[1], stream=1, epoch=epoch_t)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        augment_gather(dsrc, idx, spec, dlut, out=out, nhwc=True)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        augment_gather(dsrc, idx, spec, dlut, out=out, nhwc=True)
    outs = {}
    same_idx = torch.tensor(IDX)
    for e, batch in ((0, same_idx), (1, same_idx), (5, torch.arange(B) * 4)):
        epoch_t.fill_(e)
        idx.copy_(batch)
        graph.replay()
        outs[e] = out.cpu().clone()
        assert torch.equal(outs[e], augment_reference(src, batch, spec.replace(epoch=e), lut, nhwc=True)), e
    assert not torch.equal(outs[0], outs[1])


# ---------------------------------------------------------------- 3. the binding
def test_binding_rejects_bad_arguments_and_keeps_the_old_call():
    from katib_amd import _hipload

    k = _hipload.hipkern()
    dev = _dev()
    idx = torch.zeros(2, dtype=torch.long, device=dev)
    f32 = torch.zeros(4, 3, 8, 8, device=dev)
    k.augment_gather(f32, None, idx, torch.empty(2, 3, 8, 8, device=dev), 2, True, 1, 2, 0, 0, None)  # 11 arguments
    src = torch.zeros(4, 8, 8, 3, device=dev, dtype=torch.bfloat16)  # [N, H, W, C]
    out = torch.empty(2, 8, 8, 3, device=dev, dtype=torch.bfloat16)
    NHWC = 2
    k.augment_gather(src, None, idx, out, 0, True, 1, 2, 0, 0, None, 128 * 8, 128 * 8, NHWC)  # the largest range
    k.augment_gather(src, None, idx, out, 2, True, 1, 2, 0, 0, None, 0, 0, NHWC)  # crop into NHWC
    k.augment_gather(src, None, idx, out, 0, True, 1, 2, 0, 0, None, rx=204, ry=204, dst=NHWC)
    for rx, ry, name in ((-1, 0, "rx"), (128 * 8 + 1, 0, "rx"), (0, -1, "ry"), (0, 128 * 8 + 1, "ry")):
        with pytest.raises(RuntimeError, match=name):
            k.augment_gather(src, None, idx, out, 0, True, 1, 2, 0, 0, None, rx, ry, NHWC)
    with pytest.raises(RuntimeError, match="pad"):
        k.augment_gather(src, None, idx, out, 2, True, 1, 2, 0, 0, None, 204, 204, NHWC)
    for bad in (torch.empty(2, 8, 8, 4, device=dev, dtype=torch.bfloat16),  # not C channels
                torch.empty(2, 8, 9, 3, device=dev, dtype=torch.bfloat16),
                torch.empty(3, 8, 8, 3, device=dev, dtype=torch.bfloat16),
                torch.empty(2, 8, 8, 3, device=dev)):  # not bf16
        with pytest.raises(RuntimeError, match="out"):
            k.augment_gather(src, None, idx, bad, 0, True, 1, 2, 0, 0, None, 204, 204, NHWC)
    with pytest.raises(RuntimeError, match="aligned"):
        k.augment_gather(src, None, idx, torch.empty(2 * 8 * 8 * 3 + 1, device=dev, dtype=torch.bfloat16)[1:].view(
            2, 8, 8, 3), 0, True, 1, 2, 0, 0, None, 204, 204, NHWC)
    with pytest.raises(RuntimeError, match="dst"):  # translation has no NCHW / C8 kernel
        k.augment_gather(f32, None, idx, torch.empty(2, 3, 8, 8, device=dev), 0, True, 1, 2, 0, 0, None, 204, 204)
    with pytest.raises(RuntimeError):  # an fp32 source has no NHWC kernel
        k.augment_gather(torch.zeros(4, 3, 8, 8, device=dev), None, idx, out, 0, True, 1, 2, 0, 0, None, 0, 0, NHWC)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 4. the ENAS child
EMB = {"0": {"opt_type": "convolution", "opt_id": 0, "filter_size": "3", "num_filter": "32", "stride": "1"},
       "1": {"opt_type": "separable_convolution", "opt_id": 1, "filter_size": "3", "num_filter": "32", "stride": "2",
             "depth_multiplier": "1"}}
NN_CONFIG = {"num_layers": 2, "input_sizes": [32, 32, 3], "output_sizes": [10], "embedding": EMB}
ARCH = [[0], [1, 0]]  # a convolution first, then a separable convolution without a skip


def test_child_trainer_augments_inside_the_captured_step():
    from katib_amd.ops.augment import AugSpec, augment_reference
    from katib_amd.workloads.enas_child import ChildTrainer

    tr = ChildTrainer(ARCH, NN_CONFIG, num_train=512, num_valid=64, batch_size=32, capture=True, seed=7, augment=True)
    assert tr.xb.shape == (32, 32, 32, 3) and tr.xb.dtype == torch.bfloat16 and tr.xb.is_cuda
    g = torch.Generator().manual_seed(2)
    for _ in range(tr.step_fn.warmup):  # eager warm-up runs
        tr.step(torch.randint(0, 512, (32,), generator=g).to(tr.dev))
    assert tr.step_fn.graph is None
    src = tr.src.cpu()
    spec = AugSpec(pad=0, flip=True, translate=0.1, seed=7, stream=0)
    for e in (0, 1):  # the capture and a replay, then a replay at the next epoch
        tr.epoch_t.fill_(e)
        for _ in range(2):
            batch = torch.randint(0, 512, (32,), generator=g)
            tr.step(batch.to(tr.dev))
        assert tr.step_fn.graph is not None
        assert torch.equal(tr.xb.cpu(), augment_reference(src, batch, spec.replace(epoch=e), nhwc=True)), e
    assert not torch.equal(tr.xb.cpu(), augment_reference(src, batch, spec.replace(epoch=0), nhwc=True))
    assert math.isfinite(float(tr.acc_buf[0]))
    vl, va = tr.validate()
    assert math.isfinite(vl) and 0.0 <= va <= 1.0


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


def test_child_trainer_on_fixture_directory(cifar_dir):
    """u8 source: the captured step's batch is the oracle's; validation reads the test split."""
    from katib_amd.ops.augment import AugSpec, augment_reference
    from katib_amd.workloads.enas_child import ChildTrainer

    tr = ChildTrainer(ARCH, NN_CONFIG, num_train=96, num_valid=32, batch_size=16, capture=True, seed=9,
                      data_dir=cifar_dir, augment=True)
    g = torch.Generator().manual_seed(4)
    tr.epoch_t.fill_(1)
    for _ in range(tr.step_fn.warmup + 2):
        batch = torch.randint(0, 96, (16,), generator=g)
        tr.step(batch.to(tr.dev))
    assert tr.step_fn.graph is not None
    spec = AugSpec(pad=0, flip=True, translate=0.1, seed=9, stream=0, epoch=1)
    assert torch.equal(tr.xb.cpu(), augment_reference(tr.src.cpu(), batch, spec, tr.lut.cpu(), nhwc=True))
    assert math.isfinite(float(tr.acc_buf[0]))
    vl, va = tr.validate(32)
    assert math.isfinite(vl) and 0.0 <= va <= 1.0


@pytest.mark.parametrize("augment", ["1", "0"])
def test_enas_child_main_on_fixture(capsys, cifar_dir, augment):
    from katib_amd.workloads import enas_child

    enas_child.main(["--architecture", json.dumps(ARCH), "--nn_config", json.dumps(NN_CONFIG), "--num_epochs", "1",
                     "--batch-size", "16", "--num-train", "96", "--num-valid", "32", "--data-dir", cifar_dir,
                     "--augment", augment])
    out = capsys.readouterr().out
    for name in ("Training-Accuracy", "Training-Loss", "Validation-Accuracy", "Validation-Loss"):
        vals = [float(m) for m in re.findall(r"^%s=(\S+)$" % name, out, flags=re.M)]
        assert len(vals) == 1 and math.isfinite(vals[0]), (name, out)
