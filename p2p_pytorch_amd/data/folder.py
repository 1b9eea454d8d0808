"""Paired image folders: ``<root>/{train,test}/{a,b}/<same filename>``.

``DatasetFromFolder`` is the reference dataset (dataset.py:12-54, data.py:6-15): PIL RGB ->
[-1, 1] CHW float, no resize / crop / flip, ``a2b`` returns (a, b), ``b2a`` (the default)
returns (b, a).

``DevicePairCache`` is the MI355X path: the whole paired set is decoded ONCE into two
uint8 NHWC tensors that live in HBM (288 GB per GPU holds ~1.4 M 256x256 pairs), and a
training batch is a device-side gather + uint8->bf16 normalise -- no DataLoader worker
processes, no per-step host->device copies (the reference's only concurrency was
DataLoader workers, train.py:174-175).  Each rank of a data-parallel job draws its own
disjoint slice of a shared per-epoch permutation.  With ``load_size`` / ``crop_size`` /
``flip`` it also applies pix2pix's augmentation (resize to the load size, one random crop,
one random horizontal flip, the same for both images of a pair) in the same single pass
over the cache (``ops.augment_pairs``).
"""
from __future__ import annotations

import os
from os.path import join

import numpy as np
import torch
import torch.utils.data as data
from PIL import Image

from .. import ops
from .image_io import is_image_file, normalize, to_tensor


class DatasetFromFolder(data.Dataset):
    def __init__(self, image_dir, direction="b2a"):
        super().__init__()
        self.direction = direction
        self.a_path = join(image_dir, "a")
        self.b_path = join(image_dir, "b")
        self.image_filenames = sorted(x for x in os.listdir(self.a_path) if is_image_file(x))

    def __getitem__(self, index):
        name = self.image_filenames[index]
        a = normalize(to_tensor(Image.open(join(self.a_path, name)).convert("RGB")))
        b = normalize(to_tensor(Image.open(join(self.b_path, name)).convert("RGB")))
        return (a, b) if self.direction == "a2b" else (b, a)

    def __len__(self):
        return len(self.image_filenames)


def get_training_set(root_dir, direction="b2a"):
    return DatasetFromFolder(join(root_dir, "train"), direction)


def get_test_set(root_dir, direction="b2a"):
    return DatasetFromFolder(join(root_dir, "test"), direction)


class DevicePairCache:
    """All pairs of a folder split as uint8 [N, H, W, 3] on ``device``; images must share
    one size (the generator's crops do).

    ``load_size`` (int or (h, w), at least the image size), ``crop_size`` (int or (h, w),
    default the load size) and ``flip`` switch the augmentation on: every epoch draws one
    (y0, x0, flip) per sample next to the permutation, uniform over 0 .. load - crop and
    {0, 1}.  With all three at their defaults a batch is the plain gather + normalise.
    ``antialias`` makes the resize PIL's (and upstream pix2pix's) bicubic, and lets
    ``load_size`` be smaller than the images, down to a quarter of them; on its own it is not
    augmentation."""

    def __init__(self, dataset: DatasetFromFolder, device, rank: int = 0, world: int = 1,
                 seed: int = 123, load_size=None, crop_size=None, flip: bool = False,
                 antialias: bool = False):
        a_list, b_list = [], []
        for name in dataset.image_filenames:
            a_list.append(np.asarray(Image.open(join(dataset.a_path, name)).convert("RGB")))
            b_list.append(np.asarray(Image.open(join(dataset.b_path, name)).convert("RGB")))
        if not a_list:
            raise ValueError(f"no images in {dataset.a_path}")
        shapes = {x.shape for x in a_list + b_list}
        if len(shapes) != 1:
            raise ValueError(f"DevicePairCache needs equally sized images, got {sorted(shapes)[:4]}")
        a = torch.from_numpy(np.stack(a_list))
        b = torch.from_numpy(np.stack(b_list))
        if dataset.direction != "a2b":
            a, b = b, a
        self.a = a.to(device)
        self.b = b.to(device)
        self.n = self.a.shape[0]
        self.device = torch.device(device)
        self.rank, self.world = rank, world
        self.gen = torch.Generator(device="cpu").manual_seed(seed)
        self._perm = None
        self._pos = 0
        self.augment = load_size is not None or crop_size is not None or bool(flip)
        self.flip = bool(flip)
        self.antialias = bool(antialias)
        size = tuple(self.a.shape[1:3])
        self.load = size if load_size is None else self._hw(load_size)
        self.crop = self.load if crop_size is None else self._hw(crop_size)
        if self.antialias:
            if min(self.load) < 1 or size[0] > 4 * self.load[0] or size[1] > 4 * self.load[1]:
                raise ValueError(f"load_size {self.load} is less than a quarter of the images {size}")
        elif self.load[0] < size[0] or self.load[1] < size[1]:
            raise ValueError(f"load_size {self.load} is smaller than the images {size} (needs antialias)")
        if not (1 <= self.crop[0] <= self.load[0] and 1 <= self.crop[1] <= self.load[1]):
            raise ValueError(f"crop_size {self.crop} does not fit load_size {self.load}")
        self._table = None   # int32 [n, 4] on the device: (index, y0, x0, flip) of this epoch

    @staticmethod
    def _hw(v):
        return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))

    def __len__(self):
        return self.n

    def batches_per_epoch(self, batch_size: int) -> int:
        return self.n // (batch_size * self.world)

    @staticmethod
    def _to_model(x_u8: torch.Tensor, dtype) -> torch.Tensor:
        # uint8 NHWC -> [-1, 1] NCHW-shaped, channels_last memory (no layout copy)
        return x_u8.permute(0, 3, 1, 2).to(dtype).mul_(2.0 / 255.0).sub_(1.0).contiguous(
            memory_format=torch.channels_last)

    def new_epoch(self):
        perm = torch.randperm(self.n, generator=self.gen)
        self._perm = perm.to(self.device)
        self._pos = 0
        if self.augment:
            # every rank draws the same table from the same generator and takes its slice
            def draw(high):
                return torch.randint(0, high, (self.n,), generator=self.gen)

            y0 = draw(self.load[0] - self.crop[0] + 1)
            x0 = draw(self.load[1] - self.crop[1] + 1)
            fl = draw(2) if self.flip else torch.zeros(self.n, dtype=torch.long)
            self._table = torch.stack([perm, y0, x0, fl], 1).to(torch.int32).to(self.device)

    def next_batch(self, batch_size: int, dtype=torch.bfloat16):
        """Next (input, target) batch of this rank; None at the end of the epoch."""
        if self._perm is None:
            self.new_epoch()
        span = batch_size * self.world
        if self._pos + span > self.n:
            return None
        lo = self._pos + self.rank * batch_size
        self._pos += span
        if self.augment:   # one pass over the cache, one rounding
            return ops.augment_pairs(self.a, self.b, self._table[lo:lo + batch_size], self.load, self.crop, dtype,
                                     self.antialias)
        idx = self._perm[lo:lo + batch_size]
        return self._to_model(self.a.index_select(0, idx), dtype), self._to_model(
            self.b.index_select(0, idx), dtype)
