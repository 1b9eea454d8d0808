"""The MS-SSIM loss oracle (ops/reference.py ``ms_ssim_loss``) and its trainer flags, on the CPU."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from p2p_pytorch_amd.ops import reference as ref  # noqa: E402

K = {"uniform7": 7, "gauss11": 11}


def _pair(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1
    y = (x + 0.3 * torch.randn(*shape, generator=g, dtype=torch.float64)).clamp(-1, 1)
    return x, y


@pytest.mark.parametrize("window", list(K))
def test_identical_images_have_zero_loss(window):
    x, _ = _pair((2, 3, 4 * K[window] + 1, 4 * K[window] + 6))
    assert abs(ref.ms_ssim_loss(x, x, window, weights=ref.ms_ssim_weights(3)).item()) <= 1e-12


@pytest.mark.parametrize("window", list(K))
def test_oracle_gradcheck(window):
    k = K[window]
    x, y = _pair((1, 1, 2 * k + 2, 2 * k + 4), seed=5)
    x, y = x.requires_grad_(True), y.requires_grad_(True)
    w = ref.ms_ssim_weights(2)
    assert torch.autograd.gradcheck(lambda a, b: ref.ms_ssim_loss(a, b, window, weights=w), (x, y))


@pytest.mark.parametrize("window", list(K))
def test_one_scale_is_the_single_scale_ssim(window):
    """Every (n, c) has the same origin count, so the mean of the per-(n, c) means is ``ssim_loss``."""
    x, y = _pair((2, 3, K[window] + 5, K[window] + 8))
    assert abs(ref.ms_ssim_loss(x, y, window, weights=(1.0,)).item() - ref.ssim_loss(x, y, window).item()) <= 1e-12


def test_a_nonpositive_factor_zeroes_value_and_gradient():
    x, y = _pair((2, 3, 30, 33))
    y[:, 1] = -y[:, 1]          # channel 1: negative covariance, cs < 0 on average
    x, y = x.requires_grad_(True), y.requires_grad_(True)
    w = ref.ms_ssim_weights(2)
    ms = ref.ms_ssim(x, y, "gauss11", weights=w)
    (1.0 - ms.mean()).backward()
    assert torch.equal(ms[:, 1], torch.zeros(2, dtype=ms.dtype)) and (ms[:, [0, 2]] > 0).all()
    for g in (x.grad, y.grad):
        assert torch.isfinite(g).all() and not g[:, 1].any() and g[:, [0, 2]].abs().max() > 0


def test_the_size_rule_names_the_limit():
    x, y = _pair((1, 1, 43, 60))
    with pytest.raises(ValueError, match="at least 44 pixels"):
        ref.ms_ssim_loss(x, y, "gauss11", weights=ref.ms_ssim_weights(3))


@pytest.mark.parametrize("family,parts", [
    (["--netG", "unet_4", "--netD", "pixel", "--ngf", "8", "--ndf", "8"], ["G_GAN", "G_L1", "G_MSSSIM"]),
    ([], ["G_GAN", "G_GAN_Feat", "VGG", "TV", "MSSSIM"])], ids=["pix2pix", "reference"])   # lambda_tv = 1
def test_train_cli_logs_the_msssim_term(tmp_path, monkeypatch, family, parts):
    monkeypatch.chdir(tmp_path)
    import train
    train.main(["--synthetic", "--image_size", "32", "--steps_per_epoch", "2", "--nepoch", "1", "--epochsave", "1",
                "--no_eval", "--log_every", "1", "--name", "s", "--threads", "0", "--lambda_msssim", "1",
                "--msssim_scales", "2", "--ssim_window", "gauss11", "--log_json", "s.jsonl"] + family)
    with open("s.jsonl") as f:
        rows = [d for d in map(json.loads, f) if parts[-1] in d]
    assert len(rows) == 2
    for d in rows:
        assert 0.0 < d[parts[-1]] < 2.0 and abs(d["G"]) < 1e6
        assert d["G"] == pytest.approx(sum(d[k] for k in parts), rel=1e-5)
