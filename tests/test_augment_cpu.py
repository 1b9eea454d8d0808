"""The augmentation oracle (ops/reference.py ``augment_pairs``), the cache's per-epoch table and
the trainer flags, on the CPU."""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from p2p_pytorch_amd.data.folder import DatasetFromFolder, DevicePairCache  # noqa: E402
from p2p_pytorch_amd.ops import reference as ref  # noqa: E402


def test_oracle_at_source_size_is_the_normalised_image_or_its_mirror():
    g = torch.Generator().manual_seed(0)
    a = torch.randint(0, 256, (2, 6, 9, 3), generator=g, dtype=torch.uint8)
    b = torch.randint(0, 256, (2, 6, 9, 3), generator=g, dtype=torch.uint8)
    params = torch.tensor([[1, 0, 0, 0], [0, 0, 0, 1]], dtype=torch.int32)
    got = ref.augment_pairs(a, b, params, (6, 9), (6, 9), torch.float64)
    for src, out in zip((a, b), got):
        plain = src.permute(0, 3, 1, 2).double() * (2.0 / 255.0) - 1.0
        assert torch.equal(out[0], plain[1]) and torch.equal(out[1], torch.flip(plain[0], dims=(2,)))


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    root = tmp_path_factory.mktemp("pairs")
    g = torch.Generator().manual_seed(2)
    for side in "ab":
        (root / side).mkdir()
        for i in range(8):
            px = torch.randint(0, 256, (12, 12, 3), generator=g, dtype=torch.uint8).numpy()
            Image.fromarray(np.ascontiguousarray(px)).save(root / side / f"{i}.png")
    return DatasetFromFolder(str(root), "a2b")


def _epoch(cache, batch=2):
    cache.new_epoch()
    table = cache._table.clone()
    return table, [cache.next_batch(batch, torch.float32) for _ in range(cache.batches_per_epoch(batch))]


def test_cache_table_is_seeded_shared_by_the_ranks_and_redrawn_every_epoch(folder):
    kw = dict(seed=5, load_size=15, crop_size=(10, 12), flip=True)
    t0, b0 = _epoch(DevicePairCache(folder, "cpu", **kw))
    again = DevicePairCache(folder, "cpu", **kw)
    t1, b1 = _epoch(again)
    assert torch.equal(t0, t1) and all(torch.equal(x, y) for p, q in zip(b0, b1) for x, y in zip(p, q))
    assert b0[0][0].shape == (2, 3, 10, 12) and b0[0][0].is_contiguous(memory_format=torch.channels_last)
    assert sorted(t0[:, 0].tolist()) == list(range(8)) and t0.dtype == torch.int32
    assert 0 <= t0[:, 1].min() and t0[:, 1].max() <= 5 and 0 <= t0[:, 2].min() and t0[:, 2].max() <= 3
    assert set(t0[:, 3].tolist()) <= {0, 1}
    t2, _ = _epoch(again)                                   # the second epoch of the same cache
    assert not torch.equal(t1, t2)
    ranks = [DevicePairCache(folder, "cpu", rank=r, world=2, **kw) for r in (0, 1)]
    (ta, ba), (tb, bb) = _epoch(ranks[0]), _epoch(ranks[1])
    assert torch.equal(ta, t0) and torch.equal(tb, t0) and len(ba) == len(bb) == 2
    # rank r's k-th batch is rows [4k + 2r, 4k + 2r + 2) of the one table: disjoint indices
    for r, bs in enumerate((ba, bb)):
        for k, got in enumerate(bs):
            want = ref.augment_pairs(ranks[r].a, ranks[r].b, t0[4 * k + 2 * r:4 * k + 2 * r + 2], (15, 15), (10, 12),
                                     torch.float32)
            assert all(torch.equal(x, y) for x, y in zip(got, want))


def test_cache_without_augmentation_is_the_plain_gather(folder):
    cache = DevicePairCache(folder, "cpu", seed=5)
    cache.new_epoch()
    assert cache._table is None
    idx = cache._perm[:3]
    a, b = cache.next_batch(3, torch.float32)
    assert torch.equal(a, DevicePairCache._to_model(cache.a.index_select(0, idx), torch.float32))
    assert torch.equal(b, DevicePairCache._to_model(cache.b.index_select(0, idx), torch.float32))
    assert torch.equal(cache._perm, torch.randperm(8, generator=torch.Generator().manual_seed(5)))


def test_train_cli_refuses_augmentation_without_the_device_cache():
    import train
    with pytest.raises(SystemExit, match="--device_cache"):
        train.main(["--dataset", "facades", "--load_size", "286"])
