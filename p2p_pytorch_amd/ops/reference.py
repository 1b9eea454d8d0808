"""Pure-PyTorch oracle implementations of every fused op.

These run on CPU (the 64x64 plumbing config, unit-test oracles) and are what the
``P2P_BACKEND=torch`` eager *baseline* uses on the GPU.  The HIP kernels in ``csrc/``
implement exactly these semantics; ``tests/test_kernels_gpu.py`` compares the two.

Conventions shared with the kernels:
  * ``act`` names: None | 'relu' | 'lrelu' (slope 0.2) | 'tanh' | 'sigmoid'.
  * A conv input given as a tuple ``(a, b)`` is a *virtual concat* along channels
    (the U-Net skip concat, reference pix2pix template ``cat([x, model(x)], 1)``).
  * ``act_in`` is applied to the (virtually concatenated) input *before* padding, so
    zero padding stays zero in the activated domain.
  * ``upsample`` is a nearest-neighbour factor applied before padding
    (reference ``UpsampleConvLayer``, /root/reference/networks.py:408-423).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

LRELU_SLOPE = 0.2


def apply_act(x: torch.Tensor, act: str | None, slope: float = LRELU_SLOPE) -> torch.Tensor:
    if act is None or act == "none":
        return x
    if act == "relu":
        return F.relu(x)
    if act == "lrelu":
        return F.leaky_relu(x, slope)
    if act == "tanh":
        return torch.tanh(x)
    if act == "sigmoid":
        return torch.sigmoid(x)
    raise ValueError(f"unknown activation {act!r}")


def _cat(x):
    if isinstance(x, (tuple, list)):
        return torch.cat(list(x), 1)
    return x


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def conv2d(x, weight, bias=None, stride=1, padding=0, pad_mode="zeros", upsample=1,
           act_in=None, act_out=None):
    x = apply_act(_cat(x), act_in)
    if upsample and upsample > 1:
        x = F.interpolate(x, scale_factor=upsample, mode="nearest")
    ph, pw = _pair(padding)
    if pad_mode == "reflect" and (ph or pw):
        x = F.pad(x, (pw, pw, ph, ph), mode="reflect")
        ph = pw = 0
    y = F.conv2d(x, weight.to(x.dtype), None if bias is None else bias.to(x.dtype),
                 stride=stride, padding=(ph, pw))
    return apply_act(y, act_out)


def conv_transpose2d(x, weight, bias=None, stride=2, padding=1, act_in=None, act_out=None,
                     output_padding=0):
    x = apply_act(_cat(x), act_in)
    y = F.conv_transpose2d(x, weight.to(x.dtype), None if bias is None else bias.to(x.dtype),
                           stride=stride, padding=padding, output_padding=output_padding)
    return apply_act(y, act_out)


def instance_norm(x, eps=1e-5, act=None, weight=None, bias=None):
    # PyTorch 2.10's CPU instance_norm returns a wrong input gradient for channels_last
    # inputs with N == 1 (found by tests/test_norm_fuzz_gpu.py): go NCHW there only (the
    # GPU eager baseline keeps its channels_last layout)
    if not x.is_cuda and x.shape[0] == 1:
        x = x.contiguous()
    y = F.instance_norm(x, weight=weight, bias=bias, eps=eps)
    return apply_act(y, act)


def batch_norm(x, running_mean, running_var, weight, bias, training, momentum=0.1, eps=1e-5,
               act=None):
    y = F.batch_norm(x, running_mean, running_var, weight, bias, training, momentum, eps)
    return apply_act(y, act)


def prelu(x, weight):
    return F.prelu(x, weight)


def dropout(x, p, training):
    return F.dropout(x, p, training)


# ---------------------------------------------------------------- losses
def mse_const(pred: torch.Tensor, target: float) -> torch.Tensor:
    """MSE against a constant label without materialising the target tensor."""
    return torch.mean((pred.float() - target) ** 2)


def bce_logits_const(pred: torch.Tensor, target: float) -> torch.Tensor:
    return F.binary_cross_entropy_with_logits(pred.float(), torch.full_like(pred.float(), target))


def bce_const(prob: torch.Tensor, target: float) -> torch.Tensor:
    return F.binary_cross_entropy(prob.float(), torch.full_like(prob.float(), target))


def l1(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return torch.mean(torch.abs(a.float() - b.float()))


def mse(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return torch.mean((a.float() - b.float()) ** 2)


def tv(x: torch.Tensor) -> torch.Tensor:
    """Anisotropic TV (reference ``calc_tv_Loss``, /root/reference/train.py:123-126)."""
    x = x.float()
    return (torch.mean(torch.abs(x[:, :, :, :-1] - x[:, :, :, 1:]))
            + torch.mean(torch.abs(x[:, :, :-1, :] - x[:, :, 1:, :])))


def ssim_window(window: str, dtype=torch.float64, device=None):
    """(1-D taps summing to 1, covariance factor) of a separable SSIM window."""
    if window == "uniform7":
        return torch.full((7,), 1.0 / 7.0, dtype=dtype, device=device), 49.0 / 48.0
    if window == "gauss11":
        d = torch.arange(11, dtype=torch.float64) - 5.0
        g = torch.exp(-d * d / (2.0 * 1.5 * 1.5))
        return (g / g.sum()).to(dtype=dtype, device=device), 1.0
    raise ValueError(f"ssim_loss: unknown window {window!r} (uniform7 | gauss11)")


def ssim_loss(x: torch.Tensor, y: torch.Tensor, window: str = "uniform7",
              data_range: float = 2.0) -> torch.Tensor:
    """1 - mean SSIM over n, c and the valid window origins.

    The CONTINUOUS SSIM of the values as given (model range [-1, 1], ``data_range`` 2): no
    clamp and no uint8 quantisation, which have zero gradient -- deliberately not the
    integer-level metric of ``engine.metrics.image_metrics``.  ``uniform7``: 7x7 box with the
    sample covariance factor 49/48 (that metric's window); ``gauss11``: 11x11 Gaussian,
    sigma 1.5, factor 1 (Wang et al.).  Keeps the dtype it is given (half types go to fp32).
    """
    if x.dtype in (torch.bfloat16, torch.float16):
        x = x.float()
    y = y.to(x.dtype)
    g, f = ssim_window(window, x.dtype, x.device)
    C, k = x.shape[1], g.numel()
    w = (g[:, None] * g[None, :]).expand(C, 1, k, k).contiguous()

    def E(t):
        return F.conv2d(t, w, groups=C)

    ux, uy = E(x), E(y)
    vx = f * (E(x * x) - ux * ux)
    vy = f * (E(y * y) - uy * uy)
    vxy = f * (E(x * y) - ux * uy)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    return 1.0 - s.mean()


MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)     # Wang et al. 2003


def ms_ssim_weights(scales: int):
    """The first ``scales`` of the five MS-SSIM weights, renormalised to sum 1."""
    if not 1 <= scales <= len(MS_SSIM_WEIGHTS):
        raise ValueError(f"ms_ssim: 1 to {len(MS_SSIM_WEIGHTS)} scales, got {scales}")
    w = MS_SSIM_WEIGHTS[:scales]
    return tuple(v / sum(w) for v in w)


def ms_ssim_check(shape, window: str, scales: int, what: str = "ms_ssim_loss"):
    """The size rule ``min(H, W) >> (M - 1) >= K``: the coarsest scale still holds one window."""
    k = ssim_window(window)[0].numel()
    if not 1 <= scales <= len(MS_SSIM_WEIGHTS):
        raise ValueError(f"{what}: 1 to {len(MS_SSIM_WEIGHTS)} scales, got {scales}")
    if (min(shape[-2:]) >> (scales - 1)) < k:
        raise ValueError(f"{what}: {scales} scales with the {window} window need images of at least "
                         f"{k << (scales - 1)} pixels a side, got {shape[-2]}x{shape[-1]}")


def ms_ssim(x: torch.Tensor, y: torch.Tensor, window: str = "gauss11", data_range: float = 2.0,
            weights=MS_SSIM_WEIGHTS) -> torch.Tensor:
    """Multi-scale SSIM per image and channel, [N, C]: ``prod_j f_j ** w_j``.

    Scale 1 is the input, scale j + 1 is ``F.avg_pool2d(., 2)`` of scale j (a trailing odd row
    or column is dropped).  With ``M = len(weights)``, ``f_j`` for j < M is the mean over the
    valid window origins of the contrast-structure term ``cs = A2 / B2`` and ``f_M`` the mean
    of the full SSIM; windows, covariance factor, C1 / C2 and the continuous model-range
    semantics are those of ``ssim_loss``.  An (n, c) with any ``f_j <= 0`` has the value 0 and
    contributes an exactly zero gradient (masks, not a clamp: ``clamp_min(0) ** w`` has the
    backward 0 * inf).  Keeps the dtype it is given (half types go to fp32).
    """
    if x.dtype in (torch.bfloat16, torch.float16):
        x = x.float()
    y = y.to(x.dtype)
    M = len(weights)
    ms_ssim_check(x.shape, window, M)
    g, f = ssim_window(window, x.dtype, x.device)
    C, k = x.shape[1], g.numel()
    w = (g[:, None] * g[None, :]).expand(C, 1, k, k).contiguous()
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2

    def E(t):
        return F.conv2d(t, w, groups=C)

    fs = []
    for j in range(M):
        ux, uy = E(x), E(y)
        vx = f * (E(x * x) - ux * ux)
        vy = f * (E(y * y) - uy * uy)
        vxy = f * (E(x * y) - ux * uy)
        s = (2 * vxy + c2) / (vx + vy + c2)
        if j == M - 1:
            s = s * (2 * ux * uy + c1) / (ux * ux + uy * uy + c1)
        else:
            x, y = F.avg_pool2d(x, 2), F.avg_pool2d(y, 2)
        fs.append(s.mean(dim=(2, 3)))
    fs = torch.stack(fs)                                            # [M, N, C]
    ok = (fs > 0).all(dim=0)
    wt = torch.tensor(weights, dtype=x.dtype, device=x.device)[:, None, None]
    ms = (torch.where(ok, fs, torch.ones_like(fs)) ** wt).prod(dim=0)
    return torch.where(ok, ms, torch.zeros_like(ms))


def ms_ssim_loss(x: torch.Tensor, y: torch.Tensor, window: str = "gauss11", data_range: float = 2.0,
                 weights=MS_SSIM_WEIGHTS) -> torch.Tensor:
    """1 - mean over n, c of ``ms_ssim`` (the oracle of csrc/ms_ssim_loss.hip)."""
    return 1.0 - ms_ssim(x, y, window, data_range, weights).mean()


def ffl_check(shape, what: str = "ffl_loss"):
    """The size rule of the focal frequency loss: H and W each a multiple of 32 in [32, 512]."""
    if not all(32 <= n <= 512 and n % 32 == 0 for n in shape[-2:]):
        raise ValueError(f"{what}: H and W must each be a multiple of 32 in [32, 512], "
                         f"got {shape[-2]}x{shape[-1]}")


def _dft_matrix(n: int, dtype, device):
    """(cos, sin) of 2 pi (k j mod n) / n over sqrt(n), [n, n] each, from float64."""
    k = torch.arange(n, dtype=torch.int64)
    t = (2.0 * torch.pi / n) * ((k[:, None] * k[None, :]) % n).double()
    return ((torch.cos(t) / n ** 0.5).to(dtype=dtype, device=device),
            (torch.sin(t) / n ** 0.5).to(dtype=dtype, device=device))


def ffl_loss(x: torch.Tensor, y: torch.Tensor, alpha: float = 1.0, method: str = "fft") -> torch.Tensor:
    """Focal frequency loss (Jiang et al., ICCV 2021; the oracle of csrc/ffl_loss.hip).

    With ``F = DFT2_ortho(x - y)`` per (n, c): ``mean_{n,c,u,v} w |F|^2`` where
    ``w = |F|^alpha / max_{u,v} |F|^alpha`` is a constant (detached; 0 on a plane whose
    spectrum is zero).  ``method``: ``"fft"`` uses ``torch.fft.fft2``; ``"matrix"`` is the
    formulation of the kernels, two products against twiddle matrices, row transform first.
    Keeps the dtype it is given (half types go to fp32).
    """
    if x.dtype in (torch.bfloat16, torch.float16):
        x = x.float()
    y = y.to(x.dtype)
    ffl_check(x.shape)
    d = x - y
    if method == "fft":
        f = torch.fft.fft2(d, norm="ortho")
        p = f.real ** 2 + f.imag ** 2
    elif method == "matrix":
        ch, sh = _dft_matrix(d.shape[-2], d.dtype, d.device)
        cw, sw = _dft_matrix(d.shape[-1], d.dtype, d.device)
        zr, zi = d @ cw, -(d @ sw)
        fr, fi = ch @ zr + sh @ zi, ch @ zi - sh @ zr
        p = fr ** 2 + fi ** 2
    else:
        raise ValueError(f"ffl_loss: unknown method {method!r} (fft | matrix)")
    m = p.detach() ** (0.5 * alpha)
    mx = m.amax(dim=(2, 3), keepdim=True)
    w = torch.where(mx > 0, m / mx.clamp_min(torch.finfo(m.dtype).tiny), torch.zeros_like(m))
    return (w * p).mean()


LAP_MAX_LEVELS = 6


def lap_check(shape, levels: int, what: str = "lap_loss"):
    """The size rule of the Laplacian-pyramid loss: 1 to 6 levels, H and W each a multiple of
    ``2 ** (levels - 1)`` (every level halves exactly)."""
    if not 1 <= levels <= LAP_MAX_LEVELS:
        raise ValueError(f"{what}: 1 to {LAP_MAX_LEVELS} levels, got {levels}")
    m = 1 << (levels - 1)
    if shape[-2] < m or shape[-1] < m or shape[-2] % m or shape[-1] % m:
        raise ValueError(f"{what}: {levels} levels need H and W to be multiples of {m}, "
                         f"got {shape[-2]}x{shape[-1]}")


def _lap_down(g):
    """Binomial [1, 4, 6, 4, 1] / 16 per axis on the edge-replicated image, at even positions."""
    C = g.shape[1]
    k = torch.tensor([1.0, 4.0, 6.0, 4.0, 1.0], dtype=g.dtype, device=g.device) / 16.0
    w = (k[:, None] * k[None, :]).expand(C, 1, 5, 5).contiguous()
    return F.conv2d(F.pad(g, (2, 2, 2, 2), mode="replicate"), w, stride=2, groups=C)


def _lap_up_axis(g, dim):
    """up[2i] = (g[i-1] + 6 g[i] + g[i+1]) / 8, up[2i+1] = (g[i] + g[i+1]) / 2, indices clamped."""
    n = g.shape[dim]
    lo = torch.cat((g.narrow(dim, 0, 1), g.narrow(dim, 0, n - 1)), dim)
    hi = torch.cat((g.narrow(dim, 1, n - 1), g.narrow(dim, n - 1, 1)), dim)
    even, odd = (lo + 6.0 * g + hi) / 8.0, (g + hi) / 2.0
    shape = list(g.shape)
    shape[dim] = 2 * n
    return torch.stack((even, odd), dim + 1).reshape(shape)


def lap_bands(x: torch.Tensor, y: torch.Tensor, levels: int = 5):
    """The ``levels`` bands of the Laplacian pyramid of ``x - y`` (see ``lap_loss``)."""
    if x.dtype in (torch.bfloat16, torch.float16):
        x = x.float()
    y = y.to(x.dtype)
    lap_check(x.shape, levels)
    g, bands = x - y, []
    for _ in range(levels - 1):
        d = _lap_down(g)
        bands.append(g - _lap_up_axis(_lap_up_axis(d, 2), 3))
        g = d
    return bands + [g]


def lap_loss(x: torch.Tensor, y: torch.Tensor, levels: int = 5) -> torch.Tensor:
    """Laplacian-pyramid L1 loss of two [N, C, H, W] images (the oracle of csrc/lap_loss.hip).

    ``g_0 = x - y``; ``g_{j+1} = D g_j`` with D the separable binomial [1, 4, 6, 4, 1] / 16 on the
    edge-replicated image sampled at even rows and columns; U doubles each axis (``up[2i] =
    (g[i-1] + 6 g[i] + g[i+1]) / 8``, ``up[2i+1] = (g[i] + g[i+1]) / 2``, indices clamped).  Bands
    ``b_j = g_j - U g_{j+1}`` and ``b_{M-1} = g_{M-1}``; the loss is ``sum_j mean |b_j|``, so every
    octave has the same say (``levels = 1``: plain L1).  H and W: multiples of
    ``2 ** (levels - 1)``.  Keeps the dtype it is given (half types go to fp32).
    """
    bands = lap_bands(x, y, levels)
    loss = bands[0].abs().mean()
    for b in bands[1:]:
        loss = loss + b.abs().mean()
    return loss


def gram_check(shape, what: str = "gram_loss"):
    """The size rule of the Gram-matrix style loss: [B, C, H, W] features with C a multiple of
    64 in [64, 512] (every VGG19 tap) and at least one pixel."""
    if len(shape) != 4 or not (64 <= shape[1] <= 512 and shape[1] % 64 == 0):
        raise ValueError(f"{what}: C must be a multiple of 64 in [64, 512], got shape {tuple(shape)}")
    if shape[0] < 1 or shape[2] * shape[3] < 1:
        raise ValueError(f"{what}: B >= 1 and H * W >= 1, got shape {tuple(shape)}")


def gram_loss(fx: torch.Tensor, fy: torch.Tensor) -> torch.Tensor:
    """Gram-matrix style loss of two [B, C, H, W] feature maps (Gatys et al.; the oracle of
    csrc/gram_loss.hip): ``mean_{b,i,j} (G(fx) - G(fy))^2`` with ``G(F)_b = F_b F_b^T / (C N)``,
    ``F_b`` image b as C x N, N = H W.  ``fy`` is a constant.  Keeps the dtype it is given (half
    types go to fp32)."""
    if fy.requires_grad:
        raise ValueError("gram_loss: fy is a constant target; detach it")
    if fx.dtype in (torch.bfloat16, torch.float16):
        fx = fx.float()
    fy = fy.to(fx.dtype)
    gram_check(fx.shape)
    if fx.shape != fy.shape:
        raise ValueError(f"gram_loss: shapes differ, {tuple(fx.shape)} and {tuple(fy.shape)}")
    b, c, h, w = fx.shape
    x, y = fx.reshape(b, c, h * w), fy.reshape(b, c, h * w)
    d = (x @ x.transpose(1, 2) - y @ y.transpose(1, 2)) / (c * h * w)
    return (d * d).mean()


def augment_pairs(a_u8: torch.Tensor, b_u8: torch.Tensor, params: torch.Tensor, load, crop,
                  dtype=torch.bfloat16, antialias: bool = False):
    """Random resize / crop / flip of cached pairs (the oracle of csrc/augment.hip).

    ``a_u8`` / ``b_u8``: uint8 [N, H, W, 3]; ``params``: int [B, 4] rows (index, y0, x0, flip);
    ``load`` = (LH, LW) >= (H, W); ``crop`` = (CH, CW) <= load.  Each image is resized to
    ``load`` by ``F.interpolate(mode="bicubic", align_corners=False)`` (skipped when it is the
    source size), cropped at (y0, x0), flipped horizontally when ``flip``, clamped to
    [0, 255] and scaled to [-1, 1].  Math in float32, or float64 when ``dtype`` is float64;
    returns two [B, 3, CH, CW] channels_last tensors of ``dtype``.  With ``antialias`` the
    resize is ``F.interpolate(..., antialias=True)`` (PIL's bicubic: Keys a = -0.5, the support
    stretched by the scale, edge taps cut off and the weights renormalised), also at the source
    size, and ``load`` may be as small as a quarter of (H, W).
    """
    (LH, LW), (CH, CW) = load, crop
    N, H, W = a_u8.shape[:3]
    if antialias:
        if LH < 1 or LW < 1 or H > 4 * LH or W > 4 * LW:
            raise ValueError(f"augment_pairs: load size {LH}x{LW} is less than a quarter of the images ({H}x{W}): "
                             "antialias shrinks by at most 4x")
    elif LH < H or LW < W:
        raise ValueError(f"augment_pairs: load size {LH}x{LW} is smaller than the images ({H}x{W})")
    if not (1 <= CH <= LH and 1 <= CW <= LW):
        raise ValueError(f"augment_pairs: crop {CH}x{CW} does not fit the load size {LH}x{LW}")
    rows = params.tolist()
    for i, (idx, y0, x0, fl) in enumerate(rows):
        if not (0 <= idx < N and 0 <= y0 <= LH - CH and 0 <= x0 <= LW - CW and fl in (0, 1)):
            raise ValueError(f"augment_pairs: params row {i} = {(idx, y0, x0, fl)} is out of range")
    compute = torch.float64 if dtype == torch.float64 else torch.float32
    index = torch.tensor([r[0] for r in rows], dtype=torch.long, device=a_u8.device)

    def one(src):
        x = src.index_select(0, index).permute(0, 3, 1, 2).to(compute)
        if antialias:
            x = F.interpolate(x, size=(LH, LW), mode="bicubic", align_corners=False, antialias=True)
        elif (LH, LW) != (H, W):
            x = F.interpolate(x, size=(LH, LW), mode="bicubic", align_corners=False)
        out = []
        for n, (_, y0, x0, fl) in enumerate(rows):
            v = x[n, :, y0:y0 + CH, x0:x0 + CW]
            out.append(torch.flip(v, dims=(2,)) if fl else v)
        y = torch.stack(out) if out else x[:, :, :CH, :CW]
        y = y.clamp(0.0, 255.0) * (2.0 / 255.0) - 1.0
        return y.to(dtype).contiguous(memory_format=torch.channels_last)

    return one(a_u8), one(b_u8)


def quantize(x: torch.Tensor, bits: int) -> torch.Tensor:
    """round(clamp(x,0,1)*(2^b-1))/(2^b-1) (reference ``compress``, generate_dataset.py:29-34)."""
    m = float(2 ** bits - 1)
    return torch.round(torch.clamp(x, 0.0, 1.0) * m) / m


def avg_pool3_s2(x: torch.Tensor) -> torch.Tensor:
    """AvgPool2d(3, s2, p1, count_include_pad=False) (reference networks.py:732)."""
    return F.avg_pool2d(x, 3, stride=2, padding=1, count_include_pad=False)


def l2_normalize_channels(x: torch.Tensor, eps: float = 1e-12) -> torch.Tensor:
    return F.normalize(x, p=2, dim=1, eps=eps)
