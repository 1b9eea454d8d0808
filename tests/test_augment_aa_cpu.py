"""The antialiased resize in the augmentation oracle, the cache and the trainer flags, on the CPU."""
import numpy as np
import pytest
import torch
from PIL import Image

from p2p_pytorch_amd.data.folder import DatasetFromFolder, DevicePairCache
from p2p_pytorch_amd.ops import reference as ref


def test_oracle_keeps_a_constant_image_through_the_cut_off_edges():
    # weights that did not sum to 1 at the edges would darken the border by whole grey levels;
    # float64 weights sum to 1 within a rounding each: 2 passes x 17 taps x 2^-53 x 2 < 2^-46
    a = torch.full((1, 16, 23, 3), 200, dtype=torch.uint8)
    params = torch.tensor([[0, 0, 0, 0], [0, 0, 0, 1]], dtype=torch.int32)
    for grey, out in zip((200, 22), ref.augment_pairs(a, a // 9, params, (7, 30), (7, 30), torch.float64, True)):
        want = grey * (2.0 / 255.0) - 1.0
        assert out.shape == (2, 3, 7, 30) and (out - want).abs().max().item() <= 2.0 ** -46
    with pytest.raises(ValueError, match="at most 4x"):
        ref.augment_pairs(a, a, params, (3, 30), (3, 30), torch.float64, antialias=True)


def test_cpu_cache_loads_below_the_image_size_only_with_the_flag(tmp_path):
    g = torch.Generator().manual_seed(2)
    for side in "ab":
        (tmp_path / side).mkdir()
        for i in range(4):
            px = torch.randint(0, 256, (12, 12, 3), generator=g, dtype=torch.uint8).numpy()
            Image.fromarray(np.ascontiguousarray(px)).save(tmp_path / side / f"{i}.png")
    folder = DatasetFromFolder(str(tmp_path), "a2b")
    with pytest.raises(ValueError, match="smaller than the images"):
        DevicePairCache(folder, "cpu", load_size=7, crop_size=5, flip=True)
    assert not DevicePairCache(folder, "cpu", antialias=True).augment
    cache = DevicePairCache(folder, "cpu", load_size=7, crop_size=5, flip=True, antialias=True)
    cache.new_epoch()
    for lo in (0, 2):
        got = cache.next_batch(2, torch.float32)
        want = ref.augment_pairs(cache.a, cache.b, cache._table[lo:lo + 2], (7, 7), (5, 5), torch.float32, True)
        assert got[0].shape == (2, 3, 5, 5) and all(torch.equal(x, y) for x, y in zip(got, want))


def test_train_cli_refuses_antialias_without_the_device_cache():
    import train
    with pytest.raises(SystemExit, match="--device_cache"):
        train.main(["--dataset", "facades", "--antialias"])
