"""Datasets resident in device memory: synthetic by default, CIFAR-10 from disk on request.

There is no network access for CIFAR-10 / MNIST downloads, so workloads train on
synthetic tensors of the real shapes (documented as ``data: synthetic`` in every
benchmark line). The MI355X-first data path keeps the *whole* dataset in HBM
(CIFAR-10 train: 50k x 3 x 32 x 32 fp32 = 614 MB, trivial against 288 GB) and
draws batches with an on-device gather of a per-epoch permutation - no host
loader, no H2D copy per step. The labels are a fixed random linear function of
the images so that training makes measurable progress.

``cifar10_from_dir`` reads the CIFAR-10 binary version from a local directory instead and keeps
the raw bytes in HBM (packed ``[N, 32, 32, 4]`` uint8, 205 MB for the train split); the batch
gather normalises through a 256-entry table per channel (``ops/augment.py``). With an ``AugSpec``
the same gather also crops and flips - the reference trial's ``train_transform`` - or, in
translation mode, flips and translates: the ENAS reference child's Keras augmentation.
"""

from __future__ import annotations

import math
import os
from typing import Iterator, Optional, Tuple

import numpy as np
import torch

from ..ops.augment import PLAIN, AugSpec, augment_gather, cifar_lut


class DeviceDataset:
    def __init__(self, n: int, shape: Tuple[int, ...], num_classes: int, device, seed: int = 0,
                 dtype=torch.float32, learnable: bool = True):
        g = torch.Generator(device="cpu").manual_seed(seed)
        x = torch.randn((n,) + tuple(shape), generator=g, dtype=torch.float32)
        if learnable:
            proj = torch.randn(int(math.prod(shape)), num_classes, generator=g)
            y = (x.flatten(1) @ proj).argmax(1)
        else:
            y = torch.randint(0, num_classes, (n,), generator=g)
        self.x = x.to(device=device, dtype=dtype)
        self.y = y.to(device)
        self.n = n
        self.device = torch.device(device)
        self.num_classes = num_classes

    def subset(self, start: int, end: int) -> "DeviceSubset":
        return DeviceSubset(self, start, end)


class DeviceSubset:
    def __init__(self, ds: DeviceDataset, start: int, end: int):
        self.ds, self.start, self.end = ds, start, end

    def __len__(self):
        return self.end - self.start

    def batches(self, batch_size: int, seed: int = 0, shard: int = 0, num_shards: int = 1,
                drop_last: bool = False,
                augment: Optional[AugSpec] = None) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        """Random permutation each epoch (SubsetRandomSampler); each rank takes its own
        ``batch_size`` slice of every global batch of ``batch_size * num_shards``. With
        ``augment`` (or on a packed u8 data set, which has to be normalised) the images come from
        ``augment_gather``; the draws are keyed by data-set index, so every sharding sees the same
        crops. Labels are never touched."""
        lut = getattr(self.ds, "lut", None)
        if augment is None and lut is not None:
            augment = PLAIN
        g = torch.Generator(device="cpu").manual_seed(seed)
        perm = (torch.randperm(len(self), generator=g) + self.start).to(self.ds.device)
        gb = batch_size * num_shards
        n = len(self)
        steps = n // gb if drop_last else math.ceil(n / gb)
        for s in range(steps):
            idx = perm[s * gb + shard * batch_size: s * gb + (shard + 1) * batch_size]
            if idx.numel() == 0:
                idx = perm[:batch_size]
            if augment is not None:
                yield augment_gather(self.ds.x, idx, augment, lut), self.ds.y.index_select(0, idx)
                continue
            yield self.ds.x.index_select(0, idx), self.ds.y.index_select(0, idx)

    def steps_per_epoch(self, batch_size: int, num_shards: int = 1) -> int:
        return math.ceil(len(self) / (batch_size * num_shards))


def cifar10(device, n: int = 50000, seed: int = 0) -> DeviceDataset:
    return DeviceDataset(n, (3, 32, 32), 10, device, seed)


def mnist(device, n: int = 60000, seed: int = 0) -> DeviceDataset:
    return DeviceDataset(n, (1, 28, 28), 10, device, seed)


# ---------------------------------------------------------------- CIFAR-10 from disk
# Per-channel statistics of the CIFAR-10 train split, the constants the reference's DARTS trial
# normalises with (published values).
CIFAR10_MEAN = (0.49139968, 0.48215827, 0.44653124)
CIFAR10_STD = (0.24703233, 0.24348505, 0.26158768)
CIFAR10_RECORD = 1 + 3 * 32 * 32  # label byte + planar RGB
CIFAR10_FILES = {"train": tuple("data_batch_%d.bin" % i for i in range(1, 6)), "test": ("test_batch.bin",)}
_LAYOUT = ("the CIFAR-10 binary version: %s directly under the directory or under its cifar-10-batches-bin/, "
           "each a whole number of %d-byte records (1 label byte + 3072 planar RGB bytes)")


class PackedU8Dataset:
    """Images as packed ``[N, H, W, 4]`` uint8 (channels in bytes 0..C-1), int64 labels and the
    normalisation table ``lut [C, 256]``; batches are drawn by ``augment_gather``."""

    def __init__(self, x: torch.Tensor, y: torch.Tensor, lut: torch.Tensor, num_classes: int):
        self.x, self.y, self.lut = x, y, lut
        self.n = x.shape[0]
        self.device = x.device
        self.num_classes = num_classes

    def subset(self, start: int, end: int) -> "DeviceSubset":
        return DeviceSubset(self, start, end)


def cifar10_from_dir(root: str, device, split: str = "train", limit: int = 0,
                     lut: Optional[torch.Tensor] = None) -> PackedU8Dataset:
    """The CIFAR-10 binary version under ``root`` (numpy / torch only: no pickle, no torchvision).
    ``limit`` keeps the first ``limit`` images. ``lut [3, 256]`` replaces the default table (the
    per-channel mean / std normalisation of the DARTS and ResNet trials); the ENAS child passes
    ``byte / 255``."""
    if split not in CIFAR10_FILES:
        raise ValueError("cifar10_from_dir: split must be 'train' or 'test', got %r" % (split,))
    names = CIFAR10_FILES[split]
    layout = _LAYOUT % (", ".join(names), CIFAR10_RECORD)
    base = next((d for d in (root, os.path.join(root, "cifar-10-batches-bin"))
                 if os.path.isfile(os.path.join(d, names[0]))), None)
    if base is None:
        raise ValueError("cifar10_from_dir: %s not found under %r; expected %s" % (names[0], root, layout))
    parts = []
    for name in names:
        path = os.path.join(base, name)
        if not os.path.isfile(path):
            raise ValueError("cifar10_from_dir: %s is missing; expected %s" % (path, layout))
        raw = np.fromfile(path, dtype=np.uint8)
        if raw.size == 0 or raw.size % CIFAR10_RECORD:
            raise ValueError("cifar10_from_dir: %s has %d bytes; expected %s" % (path, raw.size, layout))
        parts.append(raw.reshape(-1, CIFAR10_RECORD))
    rec = torch.from_numpy(np.concatenate(parts, 0))
    if limit:
        rec = rec[:limit]
    n = rec.shape[0]
    packed = torch.zeros(n, 32, 32, 4, dtype=torch.uint8)
    packed[..., :3] = rec[:, 1:].view(n, 3, 32, 32).permute(0, 2, 3, 1)
    dev = torch.device(device)
    if lut is None:
        lut = cifar_lut(CIFAR10_MEAN, CIFAR10_STD)
    return PackedU8Dataset(packed.to(dev), rec[:, 0].to(torch.int64).to(dev), lut.to(dev), 10)
