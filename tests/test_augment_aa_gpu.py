"""``ops.augment_pairs(..., antialias=True)`` (csrc/augment.hip: 16 x 64 tile, 8-row bands) against the
float64 oracle on the CPU.  As in test_augment_gpu.py: uint8 noise, A != B; bf16 2^-8; fp32 max(10 x E,
2^-22), E = the oracle's float32-against-float64 difference on the case's inputs (``FP32_ORACLE_ERR``,
measured on the CPU; the 10 x covers the kernel's other summation order)."""
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
EDGES = [[0, 0, 0, 0], [1, 2, 2, 1], [1, 0, 0, 1], [0, 2, 2, 0]]   # offsets 0 and the maximum, flip 0 / 1
ONES = [[1, 0, 0, 0], [0, 1, 1, 1], [1, 1, 0, 1], [0, 0, 1, 0]]
CASES = {   # name: (N, source, load, crop, rows of (index, y0, x0, flip))
    "down_one_tile": (2, (16, 16), (7, 7), (5, 5), EDGES),   # 10 taps cut off on all four sides; two bands
    # 3 x 2 tiles, ragged last rows and columns, scalar stores, a partial last band; repeated, unordered indices
    "down_ragged": (3, (70, 150), (35, 67), (33, 67), [[2, 0, 0, 0], [0, 2, 0, 1], [2, 1, 0, 1], [1, 0, 0, 0]]),
    "down_vec4": (3, (70, 150), (35, 71), (34, 68), ONES),   # ... on the vector store path, 64 + 4 columns
    "limit_4x": (2, (64, 128), (16, 32), (16, 32), [[0, 0, 0, 0], [1, 0, 0, 1]]),   # 16 taps, the widest staged row
    "mixed_axes": (2, (30, 60), (37, 25), (36, 24), ONES),   # rows magnify (support 2, a = -0.5), columns minify
    "up_only": (2, (8, 8), (11, 11), (9, 9), EDGES),   # both axes magnify: differs from the a = -0.75 path
    "identity": (2, (8, 8), (8, 8), (8, 8), [[0, 0, 0, 0], [1, 0, 0, 1]]),   # the identity kernel with the flag on
}
FP32_ORACLE_ERR = {"down_one_tile": 7.045e-7, "down_ragged": 4.650e-6, "down_vec4": 7.832e-6, "limit_4x": 3.780e-7,
                   "mixed_axes": 2.822e-6, "up_only": 1.069e-6, "identity": 1.487e-7}
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}


@functools.lru_cache(maxsize=None)
def _case(name):
    N, (H, W), load, crop, rows = CASES[name]
    g = torch.Generator().manual_seed(0)
    a = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8)
    b = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8)
    params = torch.tensor(rows, dtype=torch.int32)
    return a, b, params, load, crop, ref.augment_pairs(a, b, params, load, crop, torch.float64, antialias=True)


def _run(name, dtype, params=None):
    p2p.set_backend("native")
    a, b, p, load, crop, _ = _case(name)
    out = ops.augment_pairs(a.cuda(), b.cuda(), p.cuda() if params is None else params, load, crop, dtype, True)
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
        print(f"augment aa {name} {dtype} {img}: max-abs {err:.3e} (tol {tol:.3e})")
        assert err <= tol


def test_two_calls_are_bitwise_equal_from_a_host_or_a_device_table():
    host = _run("down_ragged", torch.bfloat16, _case("down_ragged")[2])
    assert all(torch.equal(x, y) for x, y in zip(_run("down_ragged", torch.bfloat16), host))


def test_the_4x_limit_the_device_table_clamp_and_the_flag_off():
    a, b = (torch.zeros(1, 65, 128, 3, dtype=torch.uint8).cuda() for _ in range(2))
    zero = torch.zeros(1, 4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="at most 4x"):
        ops.augment_pairs(a, b, zero, (16, 32), (16, 32), antialias=True)
    with pytest.raises(RuntimeError, match="smaller than the images"):
        ops.augment_pairs(a, b, zero, (16, 32), (16, 32))
    wild = _run("down_one_tile", torch.float32, torch.tensor([[5, -3, 9, 7]], dtype=torch.int32).cuda())
    tame = _run("down_one_tile", torch.float32, torch.tensor([[1, 0, 2, 1]], dtype=torch.int32).cuda())
    assert all(torch.equal(x, y) for x, y in zip(wild, tame))


def test_cache_batches_are_the_kernel_applied_to_its_own_table(tmp_path):
    g = torch.Generator().manual_seed(1)
    for side in "ab":
        (tmp_path / side).mkdir()
        for i in range(4):
            px = torch.randint(0, 256, (16, 16, 3), generator=g, dtype=torch.uint8).numpy()
            Image.fromarray(np.ascontiguousarray(px)).save(tmp_path / side / f"{i}.png")
    p2p.set_backend("native")
    cache = DevicePairCache(DatasetFromFolder(str(tmp_path), "a2b"), "cuda", load_size=10, crop_size=8, flip=True,
                            antialias=True)
    cache.new_epoch()
    for lo in (0, 2):
        rows, got = cache._table[lo:lo + 2], cache.next_batch(2)
        want = ops.augment_pairs(cache.a, cache.b, rows, (10, 10), (8, 8), antialias=True)
        oracle = ref.augment_pairs(cache.a.cpu(), cache.b.cpu(), rows.cpu(), (10, 10), (8, 8), torch.float64, True)
        for x, y, z in zip(got, want, oracle):
            assert x.shape == (2, 3, 8, 8) and x.dtype == torch.bfloat16 and torch.equal(x, y)
            assert (x.double().cpu() - z).abs().max().item() <= 2.0 ** -8
    assert cache.next_batch(2) is None
