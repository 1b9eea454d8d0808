"""csrc/ms_ssim_loss.hip against the float64 oracle, and the trainer term built on it.

Kernel tiles: forward 16 x 64 pixels, backward 24 x 32 pixels.  The cases (k = window size, M
scales; M < 5 uses the first M weights renormalised, ``five_scales`` the default five):
``last_is_one_window`` has one origin at the coarsest scale (S versus cs selection);
``odd_sizes`` drops a trailing row and column in the pool and its adjoint; ``three_scales_ragged``
has several tiles with seams at two scales and an odd scale 2 (75 x 85); ``c8`` is read through
channel-padded strides.  fp32 tolerance, per case: ten times the difference between the oracle
run in fp32 and in fp64 on that case's own inputs (CPU), value (relative) and each gradient
(max-abs over max-abs) separately: ``FP32_ORACLE_ERR``.  bf16 (the oracle sees the rounded
inputs, gradients rounded to bf16): the project's rel_err < 1e-2, and 1e-3 on the value.
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
CASES = {   # name: (shape(k), M)
    "last_is_one_window": (lambda k: (1, 1, 2 * k, 2 * k), 2), "odd_sizes": (lambda k: (2, 3, 2 * k + 3, 2 * k + 5), 2),
    "three_scales_ragged": (lambda k: (2, 3, 150, 171), 3), "five_scales": (lambda k: (1, 3, 16 * k, 16 * k + 4), 5),
    "c8": (lambda k: (1, 8, 2 * k + 2, 2 * k + 6), 2)}
FP32_ORACLE_ERR = {   # (window, case): measured (value, x gradient, y gradient)
    ("uniform7", "last_is_one_window"): (3.57e-07, 5.17e-07, 1.09e-06),
    ("uniform7", "odd_sizes"): (5.16e-08, 5.60e-07, 4.52e-07),
    ("uniform7", "three_scales_ragged"): (3.45e-07, 6.17e-07, 4.82e-07),
    ("uniform7", "five_scales"): (9.52e-08, 4.78e-07, 3.84e-07),
    ("uniform7", "c8"): (2.12e-07, 2.22e-07, 2.75e-07),
    ("gauss11", "last_is_one_window"): (1.95e-07, 3.74e-07, 1.04e-07),
    ("gauss11", "odd_sizes"): (2.09e-07, 6.26e-07, 4.19e-07),
    ("gauss11", "three_scales_ragged"): (3.10e-07, 5.74e-07, 5.98e-07),
    ("gauss11", "five_scales"): (5.03e-07, 2.82e-07, 3.46e-07),
    ("gauss11", "c8"): (2.19e-07, 3.30e-07, 4.87e-07)}


def rel_err(a, b):
    return ((a.double().cpu() - b.double().cpu()).abs().max() / b.double().abs().max().clamp_min(1e-12)).item()


def _pair(window, case, dtype, negate=None):
    shape, M = CASES[case][0](K[window]), CASES[case][1]
    g = torch.Generator().manual_seed(0)
    x = torch.rand(*shape, generator=g) * 2 - 1
    y = (x + 0.3 * torch.randn(*shape, generator=g)).clamp(-1, 1)
    if negate is not None:
        y[:, negate] = -y[:, negate]
    if dtype == "bf16":
        x, y = x.bfloat16(), y.bfloat16()      # the oracle sees the rounded values
    return x, y, (ref.MS_SSIM_WEIGHTS if M == 5 else ref.ms_ssim_weights(M))


def _dev(t, dtype):
    t = t.cuda()
    return t.contiguous(memory_format=torch.channels_last) if dtype == "bf16" else t.contiguous()


def _oracle(x, y, window, w):
    xr, yr = x.double().requires_grad_(True), y.double().requires_grad_(True)
    ms = ref.ms_ssim(xr, yr, window, weights=w)
    (1.0 - ms.mean()).backward()
    return 1.0 - ms.mean().item(), ms.detach(), xr.grad, yr.grad


def _native(x, y, window, w, need_y, dtype):
    p2p.set_backend("native")
    xd, yd = _dev(x, dtype).requires_grad_(True), _dev(y, dtype).requires_grad_(need_y)
    loss = ops.ms_ssim_loss(xd, yd, window, weights=w)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), xd.grad, yd.grad


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("window", list(K))
def test_value_and_gradients_match_the_fp64_oracle(window, dtype, case):
    need_y = case == "odd_sizes"
    x, y, w = _pair(window, case, dtype)
    want, ms, wgx, wgy = _oracle(x, y, window, w)
    assert (ms > 0).all()                          # the <= 0 rule masks nothing in this comparison
    loss, gx, gy = _native(x, y, window, w, need_y, dtype)
    assert loss.dtype == torch.float32 and gx.dtype == x.dtype and gx.stride() == _dev(x, dtype).stride()
    assert (gy is None) == (not need_y) and (gy is None or gy.stride() == gx.stride() and gy.dtype == x.dtype)
    tol_v, tol_gx, tol_gy = (1e-3, 1e-2, 1e-2) if dtype == "bf16" else (10 * e for e in FP32_ORACLE_ERR[window, case])
    ev, egx = abs(loss.item() - want) / abs(want), rel_err(gx, wgx)
    egy = rel_err(gy, wgy) if need_y else 0.0
    print(f"ms_ssim {window} {dtype} {case}: value {ev:.3e} (tol {tol_v:.2e}) gx {egx:.3e} (tol {tol_gx:.2e}) "
          f"gy {egy:.3e} (tol {tol_gy:.2e})")
    assert ev <= tol_v and egx <= tol_gx and egy <= tol_gy


@pytest.mark.parametrize("window", list(K))
def test_a_masked_channel_has_exactly_zero_gradients(window):
    x, y, w = _pair(window, "odd_sizes", "fp32", negate=1)
    want, ms, wgx, wgy = _oracle(x, y, window, w)
    assert not ms[:, 1].any() and (ms[:, [0, 2]] > 0).all()
    loss, gx, gy = _native(x, y, window, w, True, "fp32")
    assert torch.isfinite(loss) and torch.isfinite(gx).all() and torch.isfinite(gy).all()
    assert not gx[:, 1].any() and not gy[:, 1].any()
    tol = [10 * e for e in FP32_ORACLE_ERR[window, "odd_sizes"]]
    assert abs(loss.item() - want) / abs(want) <= tol[0]
    assert rel_err(gx[:, [0, 2]], wgx[:, [0, 2]]) <= tol[1] and rel_err(gy[:, [0, 2]], wgy[:, [0, 2]]) <= tol[2]


def test_two_calls_are_bitwise_equal():
    x, y, w = _pair("gauss11", "three_scales_ragged", "bf16")
    l0, g0, _ = _native(x, y, "gauss11", w, False, "bf16")
    l1, g1, _ = _native(x, y, "gauss11", w, False, "bf16")
    assert torch.equal(l0, l1) and torch.equal(g0, g1)


def test_ms_ssim_returns_the_per_channel_values():
    x, y, w = _pair("gauss11", "three_scales_ragged", "fp32")
    p2p.set_backend("native")
    got = ops.ms_ssim(_dev(x, "fp32"), _dev(y, "fp32"), "gauss11", weights=w)
    want = _oracle(x, y, "gauss11", w)[1]
    assert got.shape == (2, 3) and not got.requires_grad
    assert rel_err(got, want) <= 10 * FP32_ORACLE_ERR["gauss11", "three_scales_ragged"][0]


def _step(lam, **kw):
    p2p.set_backend("native")
    torch.manual_seed(7)
    G = define_G(netG="unet_64", gpu_id="cpu", verbose=False, use_dropout=False).cuda()
    D = define_D(6, 64, norm="instance", netD="basic", gpu_id="cpu", verbose=False).cuda()
    return Pix2PixStep(G, D, lambda_msssim=lam, msssim_scales=2, **kw), G


def test_pix2pix_step_adds_the_msssim_term():
    g = torch.Generator().manual_seed(0)
    a, b = [_dev((torch.rand(2, 3, 64, 64, generator=g) * 2 - 1).bfloat16(), "bf16") for _ in range(2)]
    # the term takes a default step off the packed-image path, which has no fake_B to read
    assert _step(0.0)[0]._packed_ok(a, b) and not _step(1.0)[0]._packed_ok(a, b)
    runs = {}
    for lam in (0.0, 1.0):
        step, G = _step(lam, lr=0.0, packed=None if lam else False)
        out = step.step(a, b)
        runs[lam] = (out, G.ups[0].weight.grad.detach().clone(), G)   # ups[0]: the last layer
    with torch.no_grad():
        term = ops.ms_ssim_loss(runs[1.0][2](a), b, "uniform7", weights=ref.ms_ssim_weights(2)).item()
    out0, out1 = runs[0.0][0], runs[1.0][0]
    assert "G_MSSSIM" not in out0 and abs(out1["G_MSSSIM"].item() - term) <= 1e-3 * term
    assert not torch.equal(runs[0.0][1], runs[1.0][1])
