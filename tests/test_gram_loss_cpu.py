"""The Gram-matrix style loss oracle (ops/reference.py ``gram_loss``) and its trainer flag, on the CPU."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from p2p_pytorch_amd import ops  # noqa: E402
from p2p_pytorch_amd.ops import reference as ref  # noqa: E402

CLI = ["--synthetic", "--image_size", "32", "--steps_per_epoch", "2", "--nepoch", "1", "--epochsave", "1",
       "--no_eval", "--log_every", "1", "--name", "s", "--threads", "0", "--lambda_style", "1",
       "--log_json", "s.jsonl"]


def test_the_oracle_gradient_is_the_closed_form():
    B, C, H, W = 2, 64, 5, 7
    g = torch.Generator().manual_seed(0)
    x = torch.relu(torch.randn(B, C, H, W, generator=g, dtype=torch.float64)).requires_grad_(True)
    y = torch.relu(x.detach() + 0.3 * torch.randn(B, C, H, W, generator=g, dtype=torch.float64))
    gx, = torch.autograd.grad(ops.gram_loss(x, y), x)
    fx, fy = x.detach().reshape(B, C, -1), y.reshape(B, C, -1)
    d = (fx @ fx.transpose(1, 2) - fy @ fy.transpose(1, 2)) / (C * H * W)
    closed = (4.0 / (B * C ** 3 * H * W) * (d @ fx)).reshape(B, C, H, W)   # 4 / (B C^3 N) D fx
    assert (gx - closed).abs().max() <= 1e-12 * closed.abs().max()
    with pytest.raises(ValueError, match="constant"):
        ref.gram_loss(x, y.requires_grad_(True))


@pytest.mark.parametrize("c", [32, 96, 576])
def test_the_size_rule_names_the_limit(c):
    with pytest.raises(ValueError, match=r"multiple of 64 in \[64, 512\]"):
        ref.gram_check((1, c, 4, 4))
    with pytest.raises(ValueError, match=r"lambda_style.*multiple of 64 in \[64, 512\]"):
        ops.gram_check((1, c, 4, 4), "lambda_style")


def test_train_cli_logs_the_style_term(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    import train
    train.main(CLI)
    with open("s.jsonl") as f:
        rows = [d for d in map(json.loads, f) if "Style" in d]
    assert len(rows) == 2
    for d in rows:
        assert 0.0 < d["Style"] < 1e3 and abs(d["G"]) < 1e6
        assert d["G"] == pytest.approx(sum(d[k] for k in ("G_GAN", "G_GAN_Feat", "VGG", "TV", "Style")), rel=1e-5)


def test_the_pix2pix_family_refuses_the_flag(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    import train
    with pytest.raises(SystemExit) as e:
        train.main(CLI + ["--netG", "unet_4", "--netD", "pixel", "--ngf", "8", "--ndf", "8"])
    assert e.value.code == 2 and "--lambda_style" in capsys.readouterr().err
