"""Losses (reference networks.py:808-894 and train.py:123-126).

All are device-agnostic (reference quirk A7: the original hard-codes
``torch.cuda.FloatTensor``) and never materialise constant target tensors: the
fused kernels compute ``mean((x - c)^2)`` / BCE against a scalar label directly.
"""
from __future__ import annotations

from math import pi

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops


class GANLoss(nn.Module):
    """GAN objective against a constant real/fake label.

    ``gan_mode``: 'lsgan' (MSE, reference default), 'bce' (BCE on probabilities, the
    reference's ``use_lsgan=False``), 'vanilla' (BCE-with-logits, pix2pix default) or
    'wgangp'.  Accepts a single prediction, a list of D features (uses the last) or a
    multiscale list of lists (sums the last feature of each scale, networks.py:841-847).
    """

    def __init__(self, use_lsgan=True, target_real_label=1.0, target_fake_label=0.0, tensor=None,
                 gan_mode=None):
        super().__init__()
        self.real_label = float(target_real_label)
        self.fake_label = float(target_fake_label)
        self.gan_mode = gan_mode or ("lsgan" if use_lsgan else "bce")
        if self.gan_mode not in ("lsgan", "bce", "vanilla", "wgangp"):
            raise NotImplementedError(f"gan mode {self.gan_mode} not implemented")

    def _one(self, pred, is_real):
        t = self.real_label if is_real else self.fake_label
        if self.gan_mode == "lsgan":
            return ops.mse_const(pred, t)
        if self.gan_mode == "vanilla":
            return ops.bce_logits_const(pred, t)
        if self.gan_mode == "bce":
            return ops.bce_const(pred, t)
        return -pred.float().mean() if is_real else pred.float().mean()

    def forward(self, pred, target_is_real):
        if isinstance(pred, (list, tuple)):
            if isinstance(pred[0], (list, tuple)):
                terms = [self._one(p[-1], target_is_real) for p in pred]
                return ops.lincomb_n(terms, [1.0] * len(terms))
            return self._one(pred[-1], target_is_real)
        return self._one(pred, target_is_real)


def calc_tv_Loss(x):
    return ops.tv(x)


class SSIMLoss(nn.Module):
    """1 - mean SSIM(pred, target) on model-range images (``ops.ssim_loss``): the continuous,
    differentiable SSIM, not the uint8-level metric the trainer prints."""

    def __init__(self, window="uniform7", data_range=2.0):
        super().__init__()
        self.window, self.data_range = window, float(data_range)

    def forward(self, pred, target):
        return ops.ssim_loss(pred, target, self.window, self.data_range)


class MSSSIMLoss(nn.Module):
    """1 - mean MS-SSIM(pred, target) on model-range images (``ops.ms_ssim_loss``) over the
    first ``scales`` of the five standard weights, renormalised to sum 1."""

    def __init__(self, window="gauss11", data_range=2.0, scales=5):
        super().__init__()
        self.window, self.data_range = window, float(data_range)
        self.weights = ops.ms_ssim_weights(scales)

    def forward(self, pred, target):
        return ops.ms_ssim_loss(pred, target, self.window, self.data_range, self.weights)


class FocalFrequencyLoss(nn.Module):
    """Focal frequency loss of (pred, target) (``ops.ffl_loss``; Jiang et al., ICCV 2021): the
    squared 2-D spectrum of their difference, each coefficient weighted by ``|F|^alpha`` over
    its plane's maximum.  H and W: multiples of 32 in [32, 512]."""

    def __init__(self, alpha=1.0):
        super().__init__()
        self.alpha = float(alpha)

    def forward(self, pred, target):
        return ops.ffl_loss(pred, target, self.alpha)


class LaplacianPyramidLoss(nn.Module):
    """Laplacian-pyramid L1 ("Lap1") loss of (pred, target) (``ops.lap_loss``): the sum over
    ``levels`` octave bands of their difference of the band's mean absolute value.  H and W:
    multiples of ``2 ** (levels - 1)``."""

    def __init__(self, levels=5):
        super().__init__()
        self.levels = int(levels)

    def forward(self, pred, target):
        return ops.lap_loss(pred, target, self.levels)


class ImageTerms:
    """The optional image terms of a generator loss, ``weight * term(fake, real)``, in the fixed
    order ssim, msssim, ffl, style, lap.  Only terms with a weight > 0 are in the table: with every
    weight 0 it is empty and a step builds and launches nothing for it.  The order is the
    contract: term i reads the i-th extra ``fan_out`` view (whose backward sums the views'
    bf16 gradients in view order) and is the i-th appended to the loss composition."""

    def __init__(self, lambda_ssim, ssim_window, lambda_msssim, msssim_weights, lambda_ffl, ffl_alpha,
                 lambda_style=0.0, style=None, lambda_lap=0.0, lap_levels=5):
        table = (   # (log key, weight, (fake, real) -> scalar, size rule or None)
            ("SSIM", lambda_ssim, lambda f, r: ops.ssim_loss(f, r, ssim_window), None),
            ("MSSSIM", lambda_msssim, lambda f, r: ops.ms_ssim_loss(f, r, ssim_window, weights=msssim_weights),
             lambda shape: ops.ms_ssim_check(shape, ssim_window, len(msssim_weights), "lambda_msssim")),
            ("FFL", lambda_ffl, lambda f, r: ops.ffl_loss(f, r, ffl_alpha),
             lambda shape: ops.ffl_check(shape, "lambda_ffl")),
            ("Style", lambda_style, style, None),
            ("LAP", lambda_lap, lambda f, r: ops.lap_loss(f, r, lap_levels),
             lambda shape: ops.lap_check(shape, lap_levels, "lambda_lap")))
        self.terms = [t for t in table if t[1] > 0]

    def __len__(self):
        return len(self.terms)

    def check(self, shape):
        """The size rules of the active terms: raise before any work of the step."""
        for *_, rule in self.terms:
            if rule is not None:
                rule(shape)

    def evaluate(self, views, real):
        """[(log key, value, weight)] in table order; term i reads ``views[i]``."""
        return [(key, fn(v, real), w) for (key, w, fn, _), v in zip(self.terms, views)]


class angular_loss(nn.Module):
    """mean(acos(clamp(cos_sim_c(a, b)))) in degrees (networks.py:870-894)."""

    def forward(self, illum_gt, illum_pred):
        cos = F.cosine_similarity(illum_gt.float(), illum_pred.float(), dim=1)
        cos = torch.clamp(cos, -0.99999, 0.99999)
        return torch.mean(torch.acos(cos)) * 180 / pi


_SOBEL_X = torch.tensor([[1.0, 0.0, -1.0], [2.0, 0.0, -2.0], [1.0, 0.0, -1.0]])


def sobelLayer(img, gpu_id=None):
    """Sobel gradient magnitude of channel 0 (networks.py:852-868), without building
    new modules on every call.  Returns [1, H, W] for a batch-1 input like the reference."""
    x = img[:, :1].float()
    kx = _SOBEL_X.to(x.device).view(1, 1, 3, 3)
    ky = _SOBEL_X.t().contiguous().to(x.device).view(1, 1, 3, 3)
    gx = F.conv2d(x, kx, padding=1)
    gy = F.conv2d(x, ky, padding=1)
    g = torch.sqrt(gx * gx + gy * gy)
    return g[0] if g.shape[0] == 1 else g[:, 0]
