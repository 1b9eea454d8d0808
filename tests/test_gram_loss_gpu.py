"""csrc/gram_loss.hip against the float64 oracle (``reference.gram_loss``) on the same bf16-rounded
features, and the trainer term built on it.

Forward: pixels go through LDS in strips (stages) of 64 rows.  Split rule: with
stages = ceil(N / 64) and pairs = the macro tile pairs of C (1 up to C = 128), a split takes
sps = max(4, ceil(stages / ceil(1024 / (2 B pairs)))) stages and there are ceil(stages / sps)
splits.  (1, 64, 4, 4): one k16 step of live rows, two 32-blocks, three tile pairs;
(2, 64, 5, 7): 35 pixels, a ragged strip, the fx / fy halves of a 2B = 4 image launch;
(1, 128, 16, 16): off-diagonal tiles and their mirror on the 128-wide panel; (1, 512, 8, 8): the
widest C, off-diagonal macro pairs with two panels, the backward's K loop of 8 chunks of D;
(1, 64, 23, 23): 529 pixels = 9 stages = 3 splits of 4, 4 and 1 stages, the last stage with 17
live rows -- the smallest C = 64 shape with three splits and a ragged last one; (1, 192, 3, 3): C no
multiple of the 128 panel (channel tails read as zero in both kernels).

Tolerances: the project's bf16 bounds, value within 1e-3 relative, gradient rel_err < 1e-2
(max-abs over max-abs).  The backward takes D as one bf16 image.  Emulated on the CPU (D
rounded to bf16, fp32 product, result rounded to bf16) the gradient's rel_err per shape, in the
order above: 2.38e-3, 3.35e-3, 3.40e-3, 2.80e-3, 3.42e-3, 2.51e-3 (a hi + lo pair: 2.38e-3,
3.24e-3, 2.80e-3, 2.58e-3, 2.83e-3, 2.27e-3): every shape keeps more than 2x under 1e-2.
"""
import pytest
import torch

import p2p_pytorch_amd as p2p
from p2p_pytorch_amd import ops
from p2p_pytorch_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

SHAPES = [(1, 64, 4, 4), (2, 64, 5, 7), (1, 128, 16, 16), (1, 512, 8, 8), (1, 64, 23, 23), (1, 192, 3, 3)]
MULTI_SPLIT = (1, 64, 23, 23)


def _feats(shape):
    g = torch.Generator().manual_seed(0)
    x = torch.relu(torch.randn(*shape, generator=g))
    y = torch.relu(x + 0.3 * torch.randn(*shape, generator=g))
    return x.bfloat16(), y.bfloat16()          # the oracle sees the rounded values


def _dev(t):
    return t.cuda().contiguous(memory_format=torch.channels_last)


def _native(x, y):
    p2p.set_backend("native")
    xd = _dev(x).requires_grad_(True)
    loss = ops.gram_loss(xd, _dev(y))
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), xd.grad, xd


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_value_and_gradient_match_the_fp64_oracle(shape):
    x, y = _feats(shape)
    xr = x.double().requires_grad_(True)
    want = ref.gram_loss(xr, y.double())
    want.backward()
    loss, gx, xd = _native(x, y)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    assert gx.dtype == xd.dtype and gx.stride() == xd.stride() and torch.isfinite(gx).all()
    ev = abs(loss.item() - want.item()) / want.item()
    eg = ((gx.double().cpu() - xr.grad).abs().max() / xr.grad.abs().max()).item()
    print(f"gram {shape}: value {want.item():.4e} err {ev:.3e} (tol 1e-3)  gradient rel_err {eg:.3e} (tol 1e-2)")
    assert ev <= 1e-3 and eg < 1e-2


def test_equal_features_give_zero_loss_and_zero_gradient():
    x, _ = _feats((2, 64, 5, 7))
    loss, gx, _ = _native(x, x.clone())
    assert loss.item() == 0.0 and torch.isfinite(gx).all() and not gx.any()


def test_two_calls_are_bitwise_equal():
    x, y = _feats(MULTI_SPLIT)
    l0, g0, _ = _native(x, y)
    l1, g1, _ = _native(x, y)
    assert torch.equal(l0, l1) and torch.equal(g0, g1)


def test_violations_raise():
    x, y = _feats((1, 64, 4, 4))
    p2p.set_backend("native")
    with pytest.raises(TypeError, match="bf16 channels_last"):
        ops.gram_loss(_dev(x).float(), _dev(y).float())                  # dtype: no silent upcast
    with pytest.raises(TypeError, match="bf16 channels_last"):
        ops.gram_loss(x.cuda().contiguous(), _dev(y))                    # layout: NCHW
    x, y = _feats((1, 96, 4, 4))
    with pytest.raises(ValueError, match=r"multiple of 64 in \[64, 512\]"):
        ops.gram_loss(_dev(x), _dev(y))


def test_family_r_step_adds_the_style_term():
    from p2p_pytorch_amd.engine.compress_gan import CompressGANStep
    from p2p_pytorch_amd.models import StyleLoss, VGGLoss, define_C, define_D, define_G
    p2p.set_backend("native")
    g = torch.Generator().manual_seed(5)
    a, b = (_dev((torch.rand(2, 3, 64, 64, generator=g) * 2 - 1).bfloat16()) for _ in range(2))
    outs = {}
    for lam in (0.0, 1.0):
        torch.manual_seed(11)
        G = define_G(gpu_id="cpu", verbose=False).cuda()
        D = define_D(6, 64, gpu_id="cpu", verbose=False).cuda()
        C = define_C(gpu_id="cpu", verbose=False).cuda()
        vgg = VGGLoss().cuda()
        step = CompressGANStep(G, D, C, lr=0.0, vgg=vgg, lambda_style=lam)
        outs[lam] = step.step(a, b)
        with torch.no_grad():
            term = StyleLoss(vgg)(G(step._quant(C(b)).detach()), b).item()
    torch.cuda.synchronize()
    assert "Style" not in outs[0.0] and (step.criterionStyle is not None)
    assert term > 0 and abs(outs[1.0]["Style"].item() - term) <= 1e-3 * term
