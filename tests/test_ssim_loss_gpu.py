"""csrc/ssim_loss.hip against the float64 oracle, and the trainer term built on it.

Kernel tiles: forward 16 x 64 window origins (th x tw), backward 16 x 32 pixels.  The ragged
shape (th + k + 2, tw + k + 3) has 2 x 2 forward and 2 x 3 backward tiles, windows on every seam.
fp32 tolerance, per case: ten times the difference between the oracle run in fp32 and in fp64
on that case's own inputs (CPU), value (relative) and each gradient (max-abs over max-abs)
separately: ``FP32_ORACLE_ERR``.  bf16 (gradients rounded to bf16): the project's rel_err <
1e-2, and 1e-3 on the value.
"""
import pytest
import torch

import p2p_pytorch_amd as p2p
from p2p_pytorch_amd import ops
from p2p_pytorch_amd.engine.pix2pix import Pix2PixStep
from p2p_pytorch_amd.models import define_D, define_G
from p2p_pytorch_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

K = {"uniform7": 7, "gauss11": 11}
TH, TW = 16, 64          # forward tile (origins); the backward tile is 16 x 32 pixels
FP32_ORACLE_ERR = {   # (window, shape): measured (value, x gradient, y gradient)
    ("uniform7", "one_window"): (3.39e-8, 3.26e-7, 1.66e-7), ("uniform7", "2x3_origins"): (1.09e-7, 1.98e-7, 1.94e-7),
    ("uniform7", "ragged_tiles"): (9.51e-8, 4.61e-7, 3.76e-7), ("uniform7", "c8"): (1.33e-7, 2.68e-7, 2.52e-7),
    ("gauss11", "one_window"): (1.81e-6, 2.83e-6, 6.47e-6), ("gauss11", "2x3_origins"): (8.26e-8, 7.44e-7, 1.71e-7),
    ("gauss11", "ragged_tiles"): (5.56e-8, 5.13e-7, 6.16e-7), ("gauss11", "c8"): (1.28e-7, 2.85e-7, 3.74e-7)}
SHAPES = {"one_window": lambda k: (1, 1, k, k), "2x3_origins": lambda k: (2, 3, k + 1, k + 2),
          "ragged_tiles": lambda k: (2, 3, TH + k + 2, TW + k + 3), "c8": lambda k: (1, 8, k + 3, k + 5)}


def rel_err(a, b):
    return ((a.double().cpu() - b.double().cpu()).abs().max() / b.double().abs().max().clamp_min(1e-12)).item()


def _pair(shape, dtype):
    g = torch.Generator().manual_seed(0)
    x = torch.rand(*shape, generator=g) * 2 - 1
    y = (x + 0.3 * torch.randn(*shape, generator=g)).clamp(-1, 1)
    if dtype == "bf16":
        x, y = x.bfloat16(), y.bfloat16()      # the oracle sees the rounded values
    return x, y


def _dev(t, dtype):
    t = t.cuda()
    return t.contiguous(memory_format=torch.channels_last) if dtype == "bf16" else t.contiguous()


def _native(x, y, window, need_y, dtype):
    p2p.set_backend("native")
    xd, yd = _dev(x, dtype).requires_grad_(True), _dev(y, dtype).requires_grad_(need_y)
    loss = ops.ssim_loss(xd, yd, window)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), xd.grad, yd.grad


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("window", list(K))
def test_value_and_gradients_match_the_fp64_oracle(window, dtype, shape):
    shp = SHAPES[shape](K[window])
    need_y = shape == "2x3_origins"
    x, y = _pair(shp, dtype)
    xr, yr = x.double().requires_grad_(True), y.double().requires_grad_(True)
    want = ref.ssim_loss(xr, yr, window)
    want.backward()
    loss, gx, gy = _native(x, y, window, need_y, dtype)
    assert loss.dtype == torch.float32 and gx.dtype == x.dtype and gx.stride() == _dev(x, dtype).stride()
    tol_v, tol_gx, tol_gy = (1e-3, 1e-2, 1e-2) if dtype == "bf16" else (10 * e for e in FP32_ORACLE_ERR[window, shape])
    ev, egx = abs(loss.item() - want.item()) / abs(want.item()), rel_err(gx, xr.grad)
    egy = rel_err(gy, yr.grad) if need_y else 0.0
    print(f"ssim {window} {dtype} {shp}: value {ev:.3e} (tol {tol_v:.2e}) gx {egx:.3e} (tol {tol_gx:.2e}) "
          f"gy {egy:.3e} (tol {tol_gy:.2e})")
    assert (gy is None) == (not need_y)
    assert ev <= tol_v and egx <= tol_gx and egy <= tol_gy


@pytest.mark.parametrize("window", list(K))
def test_two_calls_are_bitwise_equal(window):
    x, y = _pair(SHAPES["ragged_tiles"](K[window]), "bf16")
    l0, g0, _ = _native(x, y, window, False, "bf16")
    l1, g1, _ = _native(x, y, window, False, "bf16")
    assert torch.equal(l0, l1) and torch.equal(g0, g1)


def _step(lam, **kw):
    p2p.set_backend("native")
    torch.manual_seed(7)
    G = define_G(netG="unet_64", gpu_id="cpu", verbose=False, use_dropout=False).cuda()
    D = define_D(6, 64, norm="instance", netD="basic", gpu_id="cpu", verbose=False).cuda()
    return Pix2PixStep(G, D, lambda_ssim=lam, **kw), G


IMAGES = lambda: [_dev(t, "bf16") for t in _pair((2, 3, 64, 64), "bf16")]  # noqa: E731


def test_pix2pix_step_adds_the_ssim_term():
    a, b = IMAGES()
    # the term takes a default step off the packed-image path, which has no fake_B to read
    assert _step(0.0)[0]._packed_ok(a, b) and not _step(1.0)[0]._packed_ok(a, b)
    runs = {}
    for lam in (0.0, 1.0):
        step, G = _step(lam, lr=0.0, packed=None if lam else False)
        out = step.step(a, b)
        runs[lam] = (out, G.ups[0].weight.grad.detach().clone(), G)   # ups[0]: the last layer
    with torch.no_grad():
        term = ops.ssim_loss(runs[1.0][2](a), b).item()
    out0, out1 = runs[0.0][0], runs[1.0][0]
    assert "G_SSIM" not in out0 and abs(out1["G_SSIM"].item() - term) <= 1e-3 * term
    assert abs((out1["G"].item() - out0["G"].item()) - term) <= 1e-2 * term
    assert not torch.equal(runs[0.0][1], runs[1.0][1])

