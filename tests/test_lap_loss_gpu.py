"""csrc/lap_loss.hip against the float64 oracle, and the trainer term built on it.

Kernel tile: 32 x 64 pixels of a level, forward and backward.  ``l1`` (M = 1) is plain L1 with
exact zeros of x - y planted (gradient 0 there); ``sub_tile`` keeps every level inside one tile;
``ragged`` has 3 x 3 tiles at level 0 with seams and partial tiles on both axes, and y needs a
gradient; ``five`` runs five levels; ``c8`` is read through channel-padded strides.

Condition on the inputs: a band value whose sign flips under fp32 rounding moves the gradient by
O(1), so ``SEEDS`` holds, per case and dtype, the smallest seed in 0 .. 63 for which the float64
oracle's smallest ``|b_j|`` is >= 1e-5 (about 50 x the fp32 rounding of a band); the test asserts
that floor from the oracle's bands.  For M = 1 the band x - y has an exact sign in either dtype and
the planted zeros are wanted, so there the floor holds for the nonzero values.

fp32 tolerance, per case: max(10 E, floor).  E is the difference between the oracle run in fp32
and in fp64 on that case's own inputs (CPU), value (relative) and each gradient (max-abs over
max-abs) separately: ``FP32_ORACLE_ERR``.  The floor covers the kernels' own summation order,
which E does not bound: a gradient element is a sum of at most 1 + 25 + 9 = 35 signed terms (its
own sign, the 5 x 5 taps of U^T, the 3 x 3 taps of D^T), each rounded once, so it may differ from
the exact sum by 35 x 2^-24 of the largest element; the value is a sum of positive terms in which
any one term passes through fewer than 35 additions (8 per thread, 6 + 3 per workgroup, the
fixed-order final tree), so the same relative bound holds for it.  bf16 (the oracle sees the rounded inputs,
gradients rounded to bf16): the project's rel_err < 1e-2, and 1e-3 on the value.
"""
import pytest
import torch

import p2p_pytorch_amd as p2p
from p2p_pytorch_amd import ops
from p2p_pytorch_amd.engine.pix2pix import Pix2PixStep
from p2p_pytorch_amd.models import define_D, define_G
from p2p_pytorch_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

CASES = {   # name: (shape, M)
    "l1": ((1, 1, 40, 72), 1), "sub_tile": ((2, 3, 32, 32), 3), "ragged": ((1, 3, 96, 160), 4),
    "five": ((1, 3, 64, 208), 5), "c8": ((1, 8, 24, 40), 2)}
BAND_FLOOR = 1e-5
SUM_FLOOR = 35 * 2.0 ** -24
SEEDS = {   # (case, dtype): seed, and the oracle's smallest |b_j| with it
    ("l1", "bf16"): 0, ("l1", "fp32"): 0,               # 4.88e-04, 7.79e-05 (nonzero values)
    ("sub_tile", "bf16"): 0, ("sub_tile", "fp32"): 0,   # 2.99e-05, 1.42e-05
    ("ragged", "bf16"): 35, ("ragged", "fp32"): 0,      # 1.26e-05, 1.18e-05
    ("five", "bf16"): 61, ("five", "fp32"): 52,         # 1.12e-05, 1.01e-05
    ("c8", "bf16"): 0, ("c8", "fp32"): 0}               # 2.48e-05, 1.43e-04
FP32_ORACLE_ERR = {   # case: measured (value, x gradient, y gradient)
    "l1": (2.21e-08, 2.42e-08, 2.42e-08), "sub_tile": (1.07e-07, 8.38e-08, 8.38e-08),
    "ragged": (2.96e-08, 1.20e-07, 1.20e-07), "five": (1.58e-08, 1.88e-07, 1.88e-07),
    "c8": (1.21e-07, 8.40e-08, 8.40e-08)}


def rel_err(a, b):
    return ((a.double().cpu() - b.double().cpu()).abs().max() / b.double().abs().max().clamp_min(1e-12)).item()


def _pair(case, dtype, seed=None):
    g = torch.Generator().manual_seed(SEEDS[case, dtype] if seed is None else seed)
    shape = CASES[case][0]
    x = torch.rand(*shape, generator=g) * 2 - 1
    y = (x + 0.3 * torch.randn(*shape, generator=g)).clamp(-1, 1)
    if case == "l1":
        y[..., ::5] = x[..., ::5]              # exact zeros of x - y
    if dtype == "bf16":
        x, y = x.bfloat16(), y.bfloat16()      # the oracle sees the rounded values
    return x, y


def _dev(t, dtype, case):
    t = t.cuda()
    t = t.contiguous(memory_format=torch.channels_last) if dtype == "bf16" else t.contiguous()
    return t[:, :3] if case == "c8" else t     # the 3 image channels of a pad-8 tensor


def _oracle(x, y, M, dtype=torch.float64):
    xr, yr = x.to(dtype).requires_grad_(True), y.to(dtype).requires_grad_(True)
    bands = ref.lap_bands(xr, yr, M)
    loss = sum(b.abs().mean() for b in bands)
    loss.backward()
    return loss.item(), xr.grad, yr.grad, [b.detach() for b in bands]


def _native(x, y, M, need_y, dtype, case):
    p2p.set_backend("native")
    xd, yd = _dev(x, dtype, case).detach().requires_grad_(True), _dev(y, dtype, case).detach().requires_grad_(need_y)
    loss = ops.lap_loss(xd, yd, M)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), xd.grad, yd.grad


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_value_and_gradients_match_the_fp64_oracle(dtype, case):
    M, need_y = CASES[case][1], case == "ragged"
    x, y = _pair(case, dtype)
    xo, yo = (x[:, :3], y[:, :3]) if case == "c8" else (x, y)
    want, wgx, wgy, bands = _oracle(xo, yo, M)
    small = torch.cat([b.abs().flatten() for b in bands])
    if M == 1:
        assert (small == 0).any() and not wgx[xo.double() == yo.double()].any()
        small = small[small > 0]
    assert small.min().item() >= BAND_FLOOR            # the condition on the inputs
    if M == 1:
        assert abs(want - (xo.double() - yo.double()).abs().mean().item()) <= 1e-15
    loss, gx, gy = _native(x, y, M, need_y, dtype, case)
    assert loss.dtype == torch.float32 and gx.dtype == x.dtype and gx.shape == xo.shape
    assert (gy is None) == (not need_y) and (gy is None or torch.equal(gy, -gx))
    if M == 1:
        assert not gx.cpu()[xo == yo].any()            # sign(0) = 0
    tol_v, tol_gx, tol_gy = (1e-3, 1e-2, 1e-2) if dtype == "bf16" else \
        (max(10 * e, SUM_FLOOR) for e in FP32_ORACLE_ERR[case])
    ev, egx = abs(loss.item() - want) / abs(want), rel_err(gx, wgx)
    egy = rel_err(gy, wgy) if need_y else 0.0
    print(f"lap {dtype} {case}: value {ev:.3e} (tol {tol_v:.2e}) gx {egx:.3e} (tol {tol_gx:.2e}) "
          f"gy {egy:.3e} (tol {tol_gy:.2e})")
    assert ev <= tol_v and egx <= tol_gx and egy <= tol_gy


def test_two_calls_are_bitwise_equal():
    x, y = _pair("ragged", "bf16")
    l0, g0, _ = _native(x, y, 4, False, "bf16", "ragged")
    l1, g1, _ = _native(x, y, 4, False, "bf16", "ragged")
    assert torch.equal(l0, l1) and torch.equal(g0, g1)


def _step(lam, **kw):
    p2p.set_backend("native")
    torch.manual_seed(7)
    G = define_G(netG="unet_64", gpu_id="cpu", verbose=False, use_dropout=False).cuda()
    D = define_D(6, 64, norm="instance", netD="basic", gpu_id="cpu", verbose=False).cuda()
    return Pix2PixStep(G, D, lambda_lap=lam, lap_levels=3, **kw), G


def _images():
    g = torch.Generator().manual_seed(0)
    return [(torch.rand(2, 3, 64, 64, generator=g) * 2 - 1).bfloat16().cuda()
            .contiguous(memory_format=torch.channels_last) for _ in range(2)]


def test_pix2pix_step_adds_the_lap_term():
    a, b = _images()
    # the term takes a default step off the packed-image path, which has no fake_B to read
    assert _step(0.0)[0]._packed_ok(a, b) and not _step(1.0)[0]._packed_ok(a, b)
    runs = {}
    for lam in (0.0, 1.0):
        step, G = _step(lam, lr=0.0, packed=None if lam else False)
        out = step.step(a, b)
        runs[lam] = (out, G.ups[0].weight.grad.detach().clone(), G)   # ups[0]: the last layer
    with torch.no_grad():
        term = ops.lap_loss(runs[1.0][2](a), b, 3).item()
    out0, out1 = runs[0.0][0], runs[1.0][0]
    assert "G_LAP" not in out0 and abs(out1["G_LAP"].item() - term) <= 1e-3 * term
    assert not torch.equal(runs[0.0][1], runs[1.0][1])
