"""The order in which the optional image terms (SSIM, MS-SSIM, focal frequency, style) enter the
generator loss of both steps, and the log keys they add: torch path, fp32, CPU."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import p2p_pytorch_amd as p2p  # noqa: E402
from p2p_pytorch_amd.engine.compress_gan import CompressGANStep  # noqa: E402
from p2p_pytorch_amd.engine.pix2pix import Pix2PixStep  # noqa: E402
from p2p_pytorch_amd.models import VGGLoss, define_C, define_D, define_G  # noqa: E402

# distinct, non-round weights: a swapped pair or a regrouped sum changes the fp32 bits
L_SSIM, L_MSSSIM, L_FFL, L_STYLE = 0.37, 1.9, 2.3, 0.71
TERMS = dict(lambda_ssim=L_SSIM, lambda_msssim=L_MSSSIM, msssim_scales=2, ssim_window="uniform7", lambda_ffl=L_FFL)


@pytest.fixture(autouse=True)
def _torch_backend():
    prev = p2p.get_backend()
    p2p.set_backend("torch")
    yield
    p2p.set_backend(prev)


def _images():
    # 32 x 32: the smallest size the focal frequency loss takes, and >= 14 (two uniform7 scales)
    g = torch.Generator().manual_seed(3)
    return (torch.rand(2, 3, 32, 32, generator=g) * 2 - 1 for _ in range(2))


def _pix2pix(**terms):
    torch.manual_seed(7)
    G = define_G(netG="unet_4", ngf=8, gpu_id="cpu", verbose=False)
    D = define_D(6, 8, netD="pixel", gpu_id="cpu", verbose=False)
    return Pix2PixStep(G, D, **terms).step(*_images())


def _family_r(**terms):
    torch.manual_seed(7)
    G = define_G(gpu_id="cpu", verbose=False)
    D = define_D(6, 64, gpu_id="cpu", verbose=False)
    C = define_C(gpu_id="cpu", verbose=False)
    step = CompressGANStep(G, D, C, vgg=VGGLoss(), **terms)
    return step, step.step(*_images())


def test_pix2pix_adds_the_terms_in_table_order():
    out = _pix2pix(**TERMS)
    assert list(out) == ["D", "G_GAN", "G_L1", "G", "G_SSIM", "G_MSSSIM", "G_FFL"]
    want = (((out["G_GAN"] + out["G_L1"]) + out["G_SSIM"] * L_SSIM) + out["G_MSSSIM"] * L_MSSSIM) \
        + out["G_FFL"] * L_FFL
    assert out["G"].dtype == torch.float32 and torch.equal(out["G"], want)
    assert list(_pix2pix()) == ["D", "G_GAN", "G_L1", "G"]


def test_family_r_adds_the_terms_in_table_order():
    step, out = _family_r(lambda_style=L_STYLE, **TERMS)
    assert list(out) == ["D", "G_GAN", "C", "G_GAN_Feat", "VGG", "TV", "G", "SSIM", "MSSSIM", "FFL", "Style"]
    want = out["G_GAN"] + out["G_GAN_Feat"] + out["VGG"] + out["TV"] * step.lambda_tv
    for key, lam in (("SSIM", L_SSIM), ("MSSSIM", L_MSSSIM), ("FFL", L_FFL), ("Style", L_STYLE)):
        want = want + out[key] * lam
    assert out["G"].dtype == torch.float32 and torch.equal(out["G"], want)
    assert list(_family_r()[1]) == ["D", "G_GAN", "C", "G_GAN_Feat", "VGG", "TV", "G"]
