"""The SSIM loss oracle (ops/reference.py ``ssim_loss``) and its trainer flag, on the CPU."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from p2p_pytorch_amd.engine.metrics import _ssim_torch, to_uint8_levels  # noqa: E402
from p2p_pytorch_amd.ops import reference as ref  # noqa: E402


def _pair(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1
    y = (x + 0.3 * torch.randn(*shape, generator=g, dtype=torch.float64)).clamp(-1, 1)
    return x, y


@pytest.mark.parametrize("window", ["uniform7", "gauss11"])
def test_identical_images_have_zero_loss(window):
    x, _ = _pair((2, 3, 16, 19))
    assert abs(ref.ssim_loss(x, x, window).item()) <= 1e-12


def test_uniform7_is_the_printed_metric_on_uint8_levels():
    """On exact uint8 levels the continuous definition is the metric the trainer prints.

    ``_ssim_torch(ref_compat=False)`` evaluates the levels 0..255 with data_range 255.  SSIM
    is invariant to a common scale of images and data_range (not to a shift: the luminance
    term sees the means), so the oracle gets the same non-negative image at scale 2 / 255
    with the matching data_range 2.0."""
    g = torch.Generator().manual_seed(3)
    lev = torch.randint(0, 256, (2, 3, 12, 15), generator=g).double()
    noisy = (lev + torch.randint(-40, 41, lev.shape, generator=g)).clamp(0, 255)
    # model-range images that land on those levels (a quarter level above the floor)
    xm, ym = (lev + 0.25) / 127.5 - 1, (noisy + 0.25) / 127.5 - 1
    assert torch.equal(to_uint8_levels(xm, False).double(), lev)
    want = _ssim_torch(xm, ym, ref_compat=False, data_range=255.0).double().mean()
    got = 1.0 - ref.ssim_loss(lev * (2.0 / 255.0), noisy * (2.0 / 255.0), "uniform7", 2.0)
    assert abs(got.item() - want.item()) <= 1e-6


@pytest.mark.parametrize("window,k", [("uniform7", 7), ("gauss11", 11)])
def test_oracle_gradcheck(window, k):
    x, y = _pair((1, 1, k + 1, k + 1), seed=5)
    x, y = x.requires_grad_(True), y.requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: ref.ssim_loss(a, b, window), (x, y))


@pytest.mark.parametrize("family,parts", [
    (["--netG", "unet_4", "--netD", "pixel", "--ngf", "8", "--ndf", "8"], ["G_GAN", "G_L1", "G_SSIM"]),
    ([], ["G_GAN", "G_GAN_Feat", "VGG", "TV", "SSIM"])], ids=["pix2pix", "reference"])   # lambda_tv = 1
def test_train_cli_logs_the_ssim_term(tmp_path, monkeypatch, family, parts):
    monkeypatch.chdir(tmp_path)
    import train
    train.main(["--synthetic", "--image_size", "32", "--steps_per_epoch", "2", "--nepoch", "1", "--epochsave", "1",
                "--no_eval", "--log_every", "1", "--name", "s", "--threads", "0", "--lambda_ssim", "1",
                "--ssim_window", "gauss11", "--log_json", "s.jsonl"] + family)
    with open("s.jsonl") as f:
        rows = [d for d in map(json.loads, f) if parts[-1] in d]
    assert len(rows) == 2
    for d in rows:
        assert 0.0 < d[parts[-1]] < 2.0 and abs(d["G"]) < 1e6
        assert d["G"] == pytest.approx(sum(d[k] for k in parts), rel=1e-5)
