"""The Laplacian-pyramid loss oracle (ops/reference.py ``lap_loss``), its size rule, its place in
``ImageTerms`` and its trainer flags, on the CPU."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from p2p_pytorch_amd import ops  # noqa: E402
from p2p_pytorch_amd.models.losses import ImageTerms  # noqa: E402
from p2p_pytorch_amd.ops import reference as ref  # noqa: E402


def _pair(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1
    y = (x + 0.3 * torch.randn(*shape, generator=g, dtype=torch.float64)).clamp(-1, 1)
    return x, y


def test_one_level_is_l1():
    x, y = _pair((2, 3, 9, 13))
    assert abs(ref.lap_loss(x, y, 1).item() - (x - y).abs().mean().item()) <= 1e-15


@pytest.mark.parametrize("shape,levels,match", [((1, 1, 100, 100), 4, "multiples of 8"),
                                                ((1, 1, 64, 64), 7, "1 to 6 levels")])
def test_the_size_rule_names_the_limit(shape, levels, match):
    with pytest.raises(ValueError, match=match):
        ops.lap_check(shape, levels, "lambda_lap")
    with pytest.raises(ValueError, match=match):
        ops.lap_loss(torch.zeros(shape), torch.zeros(shape), levels)


def test_image_terms_keep_the_order_with_lap_last():
    terms = ImageTerms(1.0, "uniform7", 1.0, ref.ms_ssim_weights(2), 1.0, 1.0, 1.0, lambda f, r: (f - r).mean(),
                       lambda_lap=0.5, lap_levels=3)
    assert [t[0] for t in terms.terms] == ["SSIM", "MSSSIM", "FFL", "Style", "LAP"]
    x, y = _pair((1, 3, 32, 32))
    key, value, weight = terms.evaluate([x] * 5, y)[-1]
    assert (key, weight) == ("LAP", 0.5) and value.item() == ref.lap_loss(x, y, 3).item()
    assert len(ImageTerms(0.0, "uniform7", 0.0, (1.0,), 0.0, 1.0)) == 0
    with pytest.raises(ValueError, match="lambda_lap"):
        ImageTerms(0.0, "uniform7", 0.0, (1.0,), 0.0, 1.0, lambda_lap=0.5, lap_levels=3).check((1, 3, 34, 32))


@pytest.mark.parametrize("family,parts", [
    (["--netG", "unet_4", "--netD", "pixel", "--ngf", "8", "--ndf", "8"], ["G_GAN", "G_L1", "G_LAP"]),
    ([], ["G_GAN", "G_GAN_Feat", "VGG", "TV", "LAP"])], ids=["pix2pix", "reference"])   # lambda_tv = 1
def test_train_cli_logs_the_lap_term(tmp_path, monkeypatch, family, parts):
    monkeypatch.chdir(tmp_path)
    import train
    train.main(["--synthetic", "--image_size", "32", "--steps_per_epoch", "2", "--nepoch", "1", "--epochsave", "1",
                "--no_eval", "--log_every", "1", "--name", "s", "--threads", "0", "--lambda_lap", "1",
                "--lap_levels", "3", "--log_json", "s.jsonl"] + family)
    with open("s.jsonl") as f:
        rows = [d for d in map(json.loads, f) if parts[-1] in d]
    assert len(rows) == 2
    for d in rows:
        assert 0.0 < d[parts[-1]] < 4.0 and abs(d["G"]) < 1e6
        assert d["G"] == pytest.approx(sum(d[k] for k in parts), rel=1e-5)
