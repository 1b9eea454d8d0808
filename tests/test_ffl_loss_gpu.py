"""csrc/ffl_loss.hip against the float64 oracle (``reference.ffl_loss``, method "fft"), and the
trainer term built on it.

Kernel tiles are 32 x 32 (one wave each): (1, 1, 32, 32) is one tile per pass; (2, 3, 64, 32) is
rectangular; (2, 3, 96, 64) has 3 row strips, 3-wave workgroups and a half spectrum of 33
columns (two column strips, the second with one live column); (1, 8, 32, 64) is the
channel-padded image layout; (1, 1, 512, 512) is the largest size, 16-wave workgroups and the
128 KB LDS strip of the column passes (both bf16 only: they cover a layout and a launch path).
fp32 tolerance, per case: ten times the difference between the oracle's "matrix" method run in fp32 and its "fft" method in float64 on that case's own inputs
(CPU), value (relative) and each gradient (max-abs over max-abs): ``FP32_ORACLE_ERR``.  bf16
(gradients rounded to bf16): the project's rel_err < 1e-2, and 1e-3 on the value.
"""
import pytest
import torch

import p2p_pytorch_amd as p2p
from p2p_pytorch_amd import ops
from p2p_pytorch_amd.engine.pix2pix import Pix2PixStep
from p2p_pytorch_amd.models import define_D, define_G
from p2p_pytorch_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

SHAPES = {"one_tile": (1, 1, 32, 32), "rect": (2, 3, 64, 32), "npo2": (2, 3, 96, 64), "c8": (1, 8, 32, 64),
          "max": (1, 1, 512, 512)}
FP32_ORACLE_ERR = {   # (shape, alpha): measured (value, x gradient, y gradient)
    ("one_tile", 0): (1.75e-8, 2.50e-7, 2.50e-7), ("one_tile", 1): (5.56e-8, 2.00e-7, 2.00e-7),
    ("one_tile", 2): (1.60e-7, 2.84e-7, 2.84e-7), ("rect", 0): (1.77e-8, 2.30e-7, 2.30e-7),
    ("rect", 1): (2.56e-8, 2.85e-7, 2.85e-7), ("rect", 2): (4.15e-8, 3.46e-7, 3.46e-7),
    ("npo2", 0): (3.23e-9, 2.60e-7, 2.60e-7), ("npo2", 1): (1.99e-8, 4.01e-7, 4.01e-7),
    ("npo2", 2): (1.95e-8, 4.66e-7, 4.66e-7)}


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


def _oracle(x, y, alpha):
    xr, yr = x.double().requires_grad_(True), y.double().requires_grad_(True)
    want = ref.ffl_loss(xr, yr, alpha, "fft")
    want.backward()
    return want.item(), xr.grad, yr.grad


def _native(x, y, alpha, need_y, dtype):
    p2p.set_backend("native")
    xd, yd = _dev(x, dtype).requires_grad_(True), _dev(y, dtype).requires_grad_(need_y)
    loss = ops.ffl_loss(xd, yd, alpha)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), xd.grad, yd.grad


@pytest.mark.parametrize("alpha", [0, 1, 2])
@pytest.mark.parametrize("dtype,shape", [(d, s) for d in ("bf16", "fp32") for s in SHAPES if d == "bf16" or s not in ("c8", "max")])
def test_value_and_gradients_match_the_fp64_oracle(dtype, shape, alpha):
    need_y = shape == "rect"
    x, y = _pair(SHAPES[shape], dtype)
    want, wgx, wgy = _oracle(x, y, alpha)
    loss, gx, gy = _native(x, y, alpha, need_y, dtype)
    assert loss.dtype == torch.float32 and gx.dtype == x.dtype and gx.stride() == _dev(x, dtype).stride()
    tol_v, tol_gx, tol_gy = (1e-3, 1e-2, 1e-2) if dtype == "bf16" else (10 * e for e in FP32_ORACLE_ERR[shape, alpha])
    ev, egx = abs(loss.item() - want) / abs(want), rel_err(gx, wgx)
    egy = rel_err(gy, wgy) if need_y else 0.0
    print(f"ffl alpha {alpha} {dtype} {shape}: value {ev:.3e} (tol {tol_v:.2e}) gx {egx:.3e} (tol {tol_gx:.2e}) "
          f"gy {egy:.3e} (tol {tol_gy:.2e})")
    assert (gy is None) == (not need_y)
    assert not need_y or (gy.dtype == y.dtype and gy.stride() == _dev(y, dtype).stride())
    assert ev <= tol_v and egx <= tol_gx and egy <= tol_gy


def test_alpha_zero_is_the_mean_squared_difference():
    x, y = _pair(SHAPES["npo2"], "fp32")
    want = ((x.double() - y.double()) ** 2).mean().item()          # Parseval: w = 1
    loss, _, _ = _native(x, y, 0, False, "fp32")
    assert abs(loss.item() - want) <= 10 * FP32_ORACLE_ERR["npo2", 0][0] * want


def test_a_zero_plane_has_a_zero_gradient_and_poisons_nothing():
    x, y = _pair(SHAPES["rect"], "fp32")
    y[1, 2] = x[1, 2]
    want, wgx, _ = _oracle(x, y, 1)
    loss, gx, _ = _native(x, y, 1, False, "fp32")
    tol = FP32_ORACLE_ERR["rect", 1]
    assert not gx[1, 2].any() and torch.isfinite(gx).all() and torch.isfinite(loss)
    assert abs(loss.item() - want) <= 10 * tol[0] * want and rel_err(gx, wgx) <= 10 * tol[1]
    loss, gx, gy = _native(x, x.clone(), 1, True, "fp32")         # x == y everywhere
    assert loss.item() == 0.0 and not gx.any() and not gy.any()


def test_two_calls_are_bitwise_equal():
    x, y = _pair(SHAPES["npo2"], "bf16")
    l0, g0, h0 = _native(x, y, 1, True, "bf16")
    l1, g1, h1 = _native(x, y, 1, True, "bf16")
    assert torch.equal(l0, l1) and torch.equal(g0, g1) and torch.equal(h0, h1)


@pytest.mark.parametrize("shape", [(1, 1, 48, 32), (1, 1, 32, 544)])
def test_the_size_rule_names_the_limit(shape):
    x, y = _pair(shape, "fp32")
    p2p.set_backend("native")
    with pytest.raises(ValueError, match=r"multiple of 32 in \[32, 512\]"):
        ops.ffl_loss(x.cuda(), y.cuda())


def test_pix2pix_step_adds_the_ffl_term():
    a, b = (_dev(t, "bf16") for t in _pair((2, 3, 64, 64), "bf16"))
    outs = {}
    for lam in (0.0, 1.0):
        p2p.set_backend("native")
        torch.manual_seed(7)
        G = define_G(netG="unet_64", gpu_id="cpu", verbose=False, use_dropout=False).cuda()
        D = define_D(6, 64, norm="instance", netD="basic", gpu_id="cpu", verbose=False).cuda()
        step = Pix2PixStep(G, D, lambda_ffl=lam, lr=0.0)
        assert step._packed_ok(a, b) == (lam == 0.0)      # the term needs fake_B as a tensor
        outs[lam] = step.step(a, b)
        with torch.no_grad():
            term = ops.ffl_loss(G(a), b).item()
    assert "G_FFL" not in outs[0.0] and abs(outs[1.0]["G_FFL"].item() - term) <= 1e-3 * term
