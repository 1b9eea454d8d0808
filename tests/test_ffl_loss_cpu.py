"""The focal frequency loss oracle (ops/reference.py ``ffl_loss``) and its trainer flags, on the CPU."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from p2p_pytorch_amd.ops import reference as ref  # noqa: E402


def _pair(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1
    y = (x + 0.3 * torch.randn(*shape, generator=g, dtype=torch.float64)).clamp(-1, 1)
    return x, y


@pytest.mark.parametrize("alpha", [0.0, 1.0, 2.0, 0.5])
def test_matrix_and_fft_methods_agree_and_the_gradient_is_the_closed_form(alpha):
    x, y = _pair((2, 3, 96, 64))
    y[1, 2] = x[1, 2]                       # a zero plane: w = 0 there, nothing is NaN
    x, y = x.requires_grad_(True), y.requires_grad_(True)
    want = ref.ffl_loss(x, y, alpha, "fft")
    gx, gy = torch.autograd.grad(want, (x, y))
    assert abs(ref.ffl_loss(x, y, alpha, "matrix").item() - want.item()) <= 1e-13 * want.item()
    mx, my = torch.autograd.grad(ref.ffl_loss(x, y, alpha, "matrix"), (x, y))
    # dL/dx = 2 / (N C H W) Re(IDFT2_ortho(w . F)),  dL/dy = -dL/dx
    f = torch.fft.fft2((x - y).detach(), norm="ortho")
    m = f.abs() ** alpha
    mmax = m.amax(dim=(2, 3), keepdim=True)
    w = torch.where(mmax > 0, m / mmax.clamp_min(1e-300), torch.zeros_like(m))
    closed = 2.0 / x.numel() * torch.fft.ifft2(w * f, norm="ortho")
    scale = closed.real.abs().max()
    assert closed.imag.abs().max() <= 1e-15 * scale and not gx[1, 2].any() and torch.isfinite(gx).all()
    for g, sign in ((gx, 1), (gy, -1), (mx, 1), (my, -1)):
        assert (g - sign * closed.real).abs().max() <= 1e-13 * scale
    if alpha == 0.0:                        # Parseval: w = 1 (0 on the zero plane, which adds nothing)
        assert abs(want.item() - ((x - y) ** 2).mean().item()) <= 1e-13 * want.item()


@pytest.mark.parametrize("shape", [(1, 1, 48, 32), (1, 1, 32, 544), (1, 1, 16, 32)])
def test_the_size_rule_names_the_limit(shape):
    x, y = _pair(shape)
    with pytest.raises(ValueError, match=r"multiple of 32 in \[32, 512\]"):
        ref.ffl_loss(x, y)


@pytest.mark.parametrize("family,parts", [
    (["--netG", "unet_4", "--netD", "pixel", "--ngf", "8", "--ndf", "8"], ["G_GAN", "G_L1", "G_FFL"]),
    ([], ["G_GAN", "G_GAN_Feat", "VGG", "TV", "FFL"])], ids=["pix2pix", "reference"])   # lambda_tv = 1
def test_train_cli_logs_the_ffl_term(tmp_path, monkeypatch, family, parts):
    monkeypatch.chdir(tmp_path)
    import train
    train.main(["--synthetic", "--image_size", "32", "--steps_per_epoch", "2", "--nepoch", "1", "--epochsave", "1",
                "--no_eval", "--log_every", "1", "--name", "s", "--threads", "0", "--lambda_ffl", "1",
                "--ffl_alpha", "1", "--log_json", "s.jsonl"] + family)
    with open("s.jsonl") as f:
        rows = [d for d in map(json.loads, f) if parts[-1] in d]
    assert len(rows) == 2
    for d in rows:
        assert 0.0 < d[parts[-1]] < 4.0 and abs(d["G"]) < 1e6
        assert d["G"] == pytest.approx(sum(d[k] for k in parts), rel=1e-5)
