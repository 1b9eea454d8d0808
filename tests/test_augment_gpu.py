"""csrc/augment.hip (``ops.augment_pairs``) against the float64 oracle run on the CPU.

Kernel tile: 32 x 64 output pixels.  Inputs are uint8 noise (A and B different), so a wrong tap,
offset or flip is an error of whole grey levels (2/255 each).  fp32 tolerance, per case:
max(10 x E, 2^-22), E = max-abs difference of the oracle run in float32 and in float64 on the
case's own inputs (``FP32_ORACLE_ERR``, measured on the CPU; 2^-22 = four fp32 ulps at magnitude
1).  bf16: 2^-8 = twice the half-ulp of the top binade, a third of a grey level.
"""
import functools

import numpy as np
import pytest
import torch
from PIL import Image

import p2p_pytorch_amd as p2p
from p2p_pytorch_amd import ops
from p2p_pytorch_amd.data.folder import DatasetFromFolder, DevicePairCache
from p2p_pytorch_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

CASES = {   # name: (N, source, load, crop, rows of (index, y0, x0, flip))
    "identity": (2, (8, 8), (8, 8), (8, 8), [[0, 0, 0, 0], [1, 0, 0, 1]]),
    "crop_only": (2, (8, 12), (8, 12), (5, 7), [[0, 0, 0, 0], [1, 3, 5, 1], [1, 0, 0, 1], [0, 3, 5, 0]]),
    # 8 -> 11, offsets 0 and 2 = the maximum: the edge clamp acts on all four sides
    "one_tile": (2, (8, 8), (11, 11), (9, 9), [[0, 0, 0, 0], [1, 2, 2, 1], [1, 0, 0, 1], [0, 2, 2, 0]]),
    # 2 x 2 tiles, ragged last rows and columns, scalar output pass; repeated, unordered indices
    "ragged_tiles": (3, (30, 60), (37, 71), (35, 67), [[2, 0, 0, 0], [0, 2, 4, 1], [2, 2, 4, 0], [1, 0, 0, 1]]),
    # the same resize with a crop width that is a multiple of 4: the vector output pass, 64 + 4 columns
    "vec4_tiles": (3, (30, 60), (37, 71), (34, 68), [[2, 0, 0, 0], [0, 3, 3, 1], [2, 3, 0, 1], [1, 0, 3, 0]]),
}
FP32_ORACLE_ERR = {"identity": 1.487e-7, "crop_only": 1.487e-7, "one_tile": 1.769e-6, "ragged_tiles": 5.217e-6,
                   "vec4_tiles": 5.217e-6}   # (the identity cases are the oracle's fp32 `* 2/255 - 1` alone)
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}


@functools.lru_cache(maxsize=None)
def _case(name):
    N, (H, W), load, crop, rows = CASES[name]
    g = torch.Generator().manual_seed(0)
    a = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8)
    b = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8)
    params = torch.tensor(rows, dtype=torch.int32)
    return a, b, params, load, crop, ref.augment_pairs(a, b, params, load, crop, torch.float64)


def _run(name, dtype, params=None):
    p2p.set_backend("native")
    a, b, p, load, crop, _ = _case(name)
    out = ops.augment_pairs(a.cuda(), b.cuda(), p.cuda() if params is None else params, load, crop, dtype)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("name", list(CASES))
def test_both_images_match_the_fp64_oracle(name, dtype):
    params, (CH, CW), want = _case(name)[2], _case(name)[4], _case(name)[5]
    tol = 2.0 ** -8 if dtype == "bf16" else max(10 * FP32_ORACLE_ERR[name], 2.0 ** -22)
    for img, got, w in zip("AB", _run(name, DTYPES[dtype]), want):
        assert got.shape == (len(params), 3, CH, CW) and got.dtype == DTYPES[dtype]
        assert got.stride() == (3 * CH * CW, 1, 3 * CW, 3)   # channels-last
        err = (got.double().cpu() - w).abs().max().item()
        print(f"augment {name} {dtype} {img}: max-abs {err:.3e} (tol {tol:.3e})")
        assert err <= tol


def test_two_calls_are_bitwise_equal_from_a_host_or_a_device_table():
    first, second = _run("ragged_tiles", torch.bfloat16), _run("ragged_tiles", torch.bfloat16, _case("ragged_tiles")[2])
    assert all(torch.equal(x, y) for x, y in zip(first, second))


def test_table_rows_are_checked_on_the_host_and_clamped_on_the_device():
    a, b, _, load, crop, _ = _case("one_tile")
    for bad in ([[2, 0, 0, 0]], [[0, 3, 0, 0]], [[0, 0, -1, 0]], [[0, 0, 0, 2]]):
        with pytest.raises(RuntimeError, match="out of range"):
            _run("one_tile", torch.float32, torch.tensor(bad, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="smaller than the images"):
        ops.augment_pairs(a.cuda(), b.cuda(), torch.zeros(1, 4, dtype=torch.int32), (7, 11), (7, 7))
    wild = _run("one_tile", torch.float32, torch.tensor([[5, -3, 9, 7]], dtype=torch.int32).cuda())
    tame = _run("one_tile", torch.float32, torch.tensor([[1, 0, 2, 1]], dtype=torch.int32).cuda())
    assert all(torch.equal(x, y) for x, y in zip(wild, tame))


def test_cache_batches_are_the_kernel_applied_to_its_own_table(tmp_path):
    g = torch.Generator().manual_seed(1)
    for side in "ab":
        (tmp_path / side).mkdir()
        for i in range(4):
            px = torch.randint(0, 256, (16, 16, 3), generator=g, dtype=torch.uint8).numpy()
            Image.fromarray(np.ascontiguousarray(px)).save(tmp_path / side / f"{i}.png")
    p2p.set_backend("native")
    cache = DevicePairCache(DatasetFromFolder(str(tmp_path), "a2b"), "cuda", load_size=20, crop_size=16, flip=True)
    cache.new_epoch()
    table = cache._table.cpu()
    assert table.shape == (4, 4) and sorted(table[:, 0].tolist()) == [0, 1, 2, 3]
    for lo in (0, 2):
        got = cache.next_batch(2)
        want = ops.augment_pairs(cache.a, cache.b, cache._table[lo:lo + 2], (20, 20), (16, 16))
        oracle = ref.augment_pairs(cache.a.cpu(), cache.b.cpu(), table[lo:lo + 2], (20, 20), (16, 16), torch.float64)
        for x, y, z in zip(got, want, oracle):
            assert x.shape == (2, 3, 16, 16) and x.dtype == torch.bfloat16
            assert x.is_contiguous(memory_format=torch.channels_last) and torch.equal(x, y)
            assert (x.double().cpu() - z).abs().max().item() <= 2.0 ** -8
    assert cache.next_batch(2) is None
