"""Autograd functions over the HIP/CDNA4 kernels (``torch.ops.p2p``).

Every GPU op of the model zoo lands here (``ops/__init__.py`` routes GPU tensors to this
module).  Conventions:

* Activations are bf16, NCHW-shaped, channels_last in memory (NHWC bytes).  Kernels need
  channel counts that are multiples of 8 (16-byte chunks); the few fringe tensors that are
  not (3-channel images, the 1-channel PatchGAN logits) are zero-padded to 8 channels on
  entry and sliced on exit -- a few MB per step.
* Weights stay fp32 masters (what the optimizer and the checkpoints see).  Each conv keeps
  bf16 GEMM-operand images of its weight (forward / dgrad layouts, see
  ``csrc/conv_fwd.hip: weight_prep``) in a per-parameter cache that is refreshed when the
  parameter's version counter moves (optimizer step, load_state_dict) or a new step
  generation starts (``begin_step``), so a captured hipGraph re-casts them every replay.
* Pad / upsample / input activation / virtual concat are folded into the conv loaders,
  output activation (+ bias) into its epilogue; backward fuses act'(x) into the dgrad
  epilogue and the concat split into two outputs.
* ``no_weight_grad(module)``-free: D's weight gradients in the G phase are skipped the
  pix2pix way (``requires_grad=False`` on D) -- ``ctx.needs_input_grad`` drives it.

Reference parity: conv/convT/IN/BN/act/losses implement networks.py:395-444 (ConvLayer,
UpsampleConvLayer, ResidualBlock), :758-806 (PatchGAN), :808-850 (GANLoss) semantics;
see ``ops/reference.py`` for the fp32 oracle each kernel is tested against.
"""
from __future__ import annotations

import contextlib
import itertools
import os
import sys

import weakref

import torch

from .. import _native
from . import fp8 as _f8

ACT = {None: 0, "none": 0, "relu": 1, "lrelu": 2, "tanh": 3, "sigmoid": 4}
# P2P_NB_FUSE=0: norm backward runs its own partial pass (A/B knob for the dgrad-epilogue fusion)
_NB_FUSE = os.environ.get("P2P_NB_FUSE", "1") != "0"
_NB_LOG = os.environ.get("P2P_NB_LOG", "0") == "1"
# reflect-pad dgrads fold in the conv epilogue (P2P_FOLD_EPI=0: padded grid + pad_fold, A/B)
_FOLD_EPI = os.environ.get("P2P_FOLD_EPI", "1") != "0"
# nearest-x2 + reflect-1 3x3 dgrads as one 4x4 stride-2 conv over dY (P2P_UP_FOLD=0: the
# upsampled-grid dgrad + pad_fold, A/B; family R B = 64 835.5 vs 808.9 img/s, gpurun_out/r4n)
_UP_FOLD = os.environ.get("P2P_UP_FOLD", "1") != "0"
CL = torch.channels_last
_NULLCTX = contextlib.nullcontext()

_gen = [0]
_seeds: dict = {}
_salt = itertools.count(1)


def P():
    return _native.ops()


def begin_step():
    """Start a new step generation: weight images are re-cast on first use (graph-safe)."""
    _gen[0] += 1
    release_handoffs()
    if _f8._pools:
        _f8.begin_step()


def release_handoffs():
    """Drop every cross-op registry entry (they hold activations of the last step: a norm's
    input, parked gradients, fp8 copies) -- host-only, no kernel.  ``CapturedStep`` calls it
    before ``empty_cache`` so the capture's private pool can take that memory."""
    _colsum_stash.clear()
    _stats_stash.clear()
    _norm_out.clear()
    _nbp_stash.clear()
    _DEFERRED.clear()   # a backward that raised part-way must not leak parked skip gradients
    _unshuffled.clear()
    _f8._qcache.clear()
    _f8._shadows.clear()


# Bias gradients handed from the norm backward to the producing conv: for a conv feeding a
# training-mode instance / batch norm, sum_p dY = sum_p dx_norm = Cc * sum_p xhat == 0
# exactly, so NormFn.backward parks that exact zero here keyed by the dx it returns and
# ConvFn.backward takes it instead of re-reading dY.  Holding the tensor keeps its storage
# alive, so a key can never alias a recycled allocation.
_colsum_stash: dict = {}


def _stash_colsum(dx, colsum):
    _colsum_stash[(dx.data_ptr(), tuple(dx.shape))] = (dx, colsum)


_stats_stash: dict = {}


def _stash_stats(y, st):
    # the entry keeps y alive, so its address cannot be reused while the entry exists
    if len(_stats_stash) >= 256:
        _stats_stash.pop(next(iter(_stats_stash)))
    _stats_stash[(y.data_ptr(), tuple(y.shape))] = (y, st)


def _take_stats(x):
    ent = _stats_stash.pop((x.data_ptr(), tuple(x.shape)), None)
    return None if ent is None else ent[1]


# Norm-backward partial sums fused into the consumer conv's dgrad epilogue.  NormFn.forward
# registers its output z with what the partial pass needs (x, mean, rstd, affine, act); a conv
# reading z as a whole input half passes that to its dgrad, whose epilogue emits sum(d) and
# sum(d * xhat) per tile (conv_dev.h nb_*); the partials are parked keyed by the gradient
# tensor and NormFn.backward takes them only if it receives exactly that tensor (an
# autograd-accumulated gradient is a new tensor: the norm then runs its own partial pass).
_norm_out: dict = {}
_nbp_stash: dict = {}
# the same hand-off for a biased conv output read whole by one conv (its act' already applied
# by that consumer, or no activation): the consumer's dgrad epilogue emits the column sums of
# the gradient -- the producer's bias gradient -- parked in _colsum_stash
_CS = ("colsum",)


def _register_norm_out(z, info):
    if len(_norm_out) >= 256:
        _norm_out.pop(next(iter(_norm_out)))
    _norm_out[(z.data_ptr(), tuple(z.shape))] = (z, info)


def _norm_lookup(t):
    if t is None:
        return None
    ent = _norm_out.get((t.data_ptr(), tuple(t.shape)))
    return None if ent is None or ent[0] is not t else ent[1]


# Invariant both stashes rely on: an entry holds a reference to the gradient tensor, so autograd
# never accumulates a second consumer's gradient INTO it in place (its InputBuffer only reuses a
# buffer it holds the last reference to) -- a summed gradient is always a new tensor, whose key
# or identity does not match, and the consumer of the stash recomputes instead.
def _stash_nbp(g, parts):
    if len(_nbp_stash) >= 256:
        _nbp_stash.pop(next(iter(_nbp_stash)))
    _nbp_stash[(g.data_ptr(), tuple(g.shape))] = (g, parts)


def _take_nbp(g):
    ent = _nbp_stash.pop((g.data_ptr(), tuple(g.shape)), None)
    return None if ent is None or ent[0] is not g else ent[1]


def _take_colsum(gy):
    ent = _colsum_stash.pop((gy.data_ptr(), tuple(gy.shape)), None)
    return None if ent is None else ent[1]


# ------------------------------------------------------------ one gradient per parameter
# A parameter read by several ops of one forward -- family R's discriminator runs its fake and
# real passes separately in the D phase (/root/reference/train.py:308-316), so every D weight
# and bias gets two contributions in one backward -- would have them summed by an aten add in
# autograd's input buffer.  Instead the first contribution's tensor is remembered for the
# current graph task and the later ones are accumulated into it by the producing kernel
# (wgrad / sn_wgrad accumulate mode, colsum accumulate); they return None to autograd.  Within
# one graph task AccumulateGrad runs only after every producer of the leaf, so the first
# tensor is still unconsumed when the later contributions land in it.
_GRAD_PAIRS: dict = {}
_GRAD_PAIRS_TASK = [-1]


def _pair_first(param, on=False):
    """The tensor already handed to autograd for ``param`` in the running backward, if any.
    Only the spectral-norm convs (``on``: family R's discriminator, run twice per D phase) and
    parameters a model marks ``_p2p_pair`` are paired; everything else keeps autograd's plain
    single-contribution path."""
    if (param is None or not isinstance(param, torch.Tensor) or not param.is_leaf
            or not (on or getattr(param, "_p2p_pair", False))):
        return None
    if os.environ.get("P2P_GRAD_PAIR", "1") == "0":
        return None
    tid = torch._C._current_graph_task_id()
    if tid < 0 or tid != _GRAD_PAIRS_TASK[0]:
        return None
    ent = _GRAD_PAIRS.get(id(param))
    return ent[1] if ent is not None and ent[0]() is param else None


def _pair_set(param, t, on=False):
    """``t`` is the first contribution of ``param``'s gradient in the running backward."""
    if (param is None or t is None or not isinstance(param, torch.Tensor) or not param.is_leaf
            or not (on or getattr(param, "_p2p_pair", False))):
        return
    if os.environ.get("P2P_GRAD_PAIR", "1") == "0":
        return
    tid = torch._C._current_graph_task_id()
    if tid < 0:
        return
    if tid != _GRAD_PAIRS_TASK[0]:      # a new backward: the old entries pin finished tensors
        _GRAD_PAIRS.clear()
        _GRAD_PAIRS_TASK[0] = tid
    # keep an ALIAS (a second TensorImpl over the same storage), not ``t`` itself: an extra
    # reference to ``t`` makes AccumulateGrad clone it instead of stealing it -- an extra copy
    # kernel, and for a weight gradient written on the side stream a compute-stream read
    # racing that write (``_wgrad_side``)
    alias = t.new_empty((0,)).set_(t.untyped_storage(), t.storage_offset(), t.size(), t.stride())
    _GRAD_PAIRS[id(param)] = (weakref.ref(param), alias)


# ------------------------------------------------------------ weight-gradient side stream
# A conv's weight gradient feeds nothing else in its backward: only the optimizer (and the
# DP reducer) read it.  Inside ``wgrad_overlap`` every ConvFn weight gradient is launched on a
# per-device side HIP stream (forked from the compute stream at that point), so the wgrad
# GEMMs -- a quarter of the headline step -- run beside the dgrad / norm-backward chain that
# the next layers wait on (LDS/MFMA-bound wgrads next to HBM-bound norm passes and the
# small-grid deep U-Net levels).  The context's exit joins the side stream back (stream
# order, no host sync; a hipGraph capture records the fork/join).  Tensors the side stream
# reads are held until that join, so the allocator cannot recycle them under it (no
# ``record_stream``: its deferred events under capture crashed a later capture).  Autograd
# then hands each gradient to AccumulateGrad, which only STEALS it (grads set to None, one
# gradient per weight); a weight that receives a second gradient in the same backward has
# its earlier one joined first (autograd's add then runs on the compute stream).  Under a DP
# reducer (parallel/ddp.py) a conv weight's gradient is written straight into its bucket by
# the kernel (accumulate mode, pre-scaled), so it may run on the side stream too; the
# reducer's collective for that bucket waits on a side-stream event.
class _WgradSide:
    on = False
    streams: dict = {}
    seen: set = set()
    keep: list = []     # operands the side stream reads, held until the join


def wgrad_overlap_enabled() -> bool:
    return os.environ.get("P2P_WGRAD_STREAM", "1") != "0"


class wgrad_overlap:
    """``with wgrad_overlap(device): loss.backward()`` -- see the block comment above."""

    def __init__(self, device, enabled=True):
        self.dev = torch.device(device)
        self.enabled = bool(enabled) and self.dev.type == "cuda" and wgrad_overlap_enabled()

    def __enter__(self):
        if self.enabled:
            idx = self.dev.index if self.dev.index is not None else torch.cuda.current_device()
            s = _WgradSide.streams.get(idx)
            if s is None:
                s = _WgradSide.streams[idx] = torch.cuda.Stream(device=idx)
            self.stream = s
            self.prev = _WgradSide.on
            _WgradSide.on = s
            _WgradSide.seen.clear()
        return self

    def __exit__(self, *exc):
        if self.enabled:
            _WgradSide.on = self.prev
            _WgradSide.seen.clear()
            torch.cuda.current_stream(self.stream.device).wait_stream(self.stream)
            _WgradSide.keep.clear()   # freed after the join: stream-ordered behind the side work
        return False


def _wgrad_side(weight):
    """The side stream for this weight's gradient (None: compute stream)."""
    s = _WgradSide.on
    if not s:
        return None
    # the side-stream gradient is only safe when AccumulateGrad STEALS it: a leaf weight with
    # no gradient yet, fp32 and dense-contiguous like the returned gw (else autograd adds /
    # clones it on the compute stream, racing the side-stream kernel that writes it)
    if (not weight.is_leaf or weight.grad is not None or weight.dtype != torch.float32
            or not weight.is_contiguous()):
        if weight.data_ptr() in _WgradSide.seen:
            torch.cuda.current_stream(s.device).wait_stream(s)
        return None
    if weight.data_ptr() in _WgradSide.seen:
        # second gradient of this weight: autograd will add it to the first on the compute
        # stream, so the first must be complete before it
        torch.cuda.current_stream(s.device).wait_stream(s)
        return None
    _WgradSide.seen.add(weight.data_ptr())
    return s


def _pad8(c: int) -> int:
    return (c + 7) // 8 * 8


def _act_code(a):
    if a not in ACT:
        raise ValueError(f"unknown activation {a!r}")
    return ACT[a]


def to_nhwc_bf16(x: torch.Tensor) -> torch.Tensor:
    if x.dtype != torch.bfloat16:
        x = x.to(torch.bfloat16)
    if not x.is_contiguous(memory_format=CL):
        x = x.contiguous(memory_format=CL)
    return x


def _weight_image(w: torch.Tensor, swap: int, xp: int, yp: int, scale=None) -> torch.Tensor:
    """bf16 GEMM-operand image of an fp32 master weight, cached per (layout, padding)."""
    cache = getattr(w, "_p2p_cache", None)
    if cache is None:
        cache = {}
        try:
            w._p2p_cache = cache
        except AttributeError:  # plain tensor without __dict__
            pass
    key = (swap, xp, yp, None if scale is None else id(scale))
    ent = cache.get(key)
    ver = w._version
    if ent is not None and ent[0] == ver and ent[1] == _gen[0] and scale is None:
        return ent[2]
    img = P().weight_prep(w.detach().contiguous().float(), swap, xp, yp, scale)
    cache[key] = (ver, _gen[0], img)
    return img


# phase sums of a 3x3 kernel seen through nearest x2 + edge pad 1 (ops/hip.py up-fold dgrad):
# tap a of the 4-tap stride-2 input-gradient kernel collects the 3x3 taps k with
# o + k + 1 in {2q, 2q + 1} for o = 2q + a - 3
# (M = ((0, 0, 1), (0, 1, 1), (1, 1, 0), (1, 0, 0)); computed on the device, misc.hip)


def _up2_dgrad_image(w: torch.Tensor, cp: int, coutp: int) -> torch.Tensor:
    """bf16 [Cp][4][4][Coutp] GEMM image of the nearest-x2 + reflect-1 3x3 conv's input
    gradient as a 4x4 stride-2 conv over dY: W''[ci][co][a][b] = sum_kl M[a][k] M[b][l]
    w[co][ci][k][l].  Cached per step like the plain weight images."""
    cache = getattr(w, "_p2p_cache", None)
    if cache is None:
        cache = {}
        w._p2p_cache = cache
    key = ("up2d", cp, coutp)
    ver = w._version
    ent = cache.get(key)
    if ent is not None and ent[0] == ver and ent[1] == _gen[0]:
        return ent[2]
    # device-only phase sum (misc.hip up2_dgrad_image_kernel): no host tensor and no GEMM,
    # so the first step after a weight update stays legal inside a hipGraph capture
    img = P().up2_dgrad_image(w.detach().contiguous().float(), cp, coutp)
    cache[key] = (ver, _gen[0], img)
    return img


def _weight_image_fp8(w: torch.Tensor, swap: int, xp: int, yp: int):
    """e4m3 copy (current scaling) of the bf16 GEMM-operand image, cached like the bf16 one;
    returns (image, scale site)."""
    cache = getattr(w, "_p2p_cache", None)
    key = (swap, xp, yp, "fp8")
    ver = w._version
    ent = cache.get(key) if cache is not None else None
    if ent is not None and ent[0] == ver and ent[1] == _gen[0]:
        return ent[2]
    img = _weight_image(w, swap, xp, yp)
    out = _f8.quant_weight(img, (_f8.obj_key(w), "w", swap))
    w._p2p_cache[key] = (ver, _gen[0], out)
    return out


def _conv_call(x1, x2, wimg, bias, mode, KH, KW, s, p, reflect, up, act_in, OH, OW, Cout, act_out,
               Csplit, xb1, xb2, act_bwd, Cvalid, want, weight=None, swap=0, xp=0, yp=0, role="x",
               y_qkey=None, res=None, alpha=None, nb=None, fold=None):
    """conv_fwd on bf16 operands, or -- fp8 precision and a geometry the fp8 kernel takes --
    on fp8 ones: x (role 'x': activations, e4m3; 'gy': gradients, e5m2) quantised with
    delayed scaling (or taken from the producer's fused shadow), the weight image with
    current scaling.  ``y_qkey``: also emit an e4m3 shadow of the output from the epilogue
    (the output feeds other fp8 convs directly) -- appended last to the returned list.
    ``wimg`` may be None (built on demand for the bf16 path).  ``res``: bf16 tensor added to
    the (unsplit) output in the epilogue, after the act' gate.  ``nb`` = (half, norm info): the
    dgrad epilogue also emits that half's norm-backward partials (bf16 path only), appended
    as the last output.  ``fold`` = (H, W, p): a MODE-1 dgrad onto the reflect-padded grid
    (OH, OW) = (H + 2p, W + 2p) returns the real input's gradient (H, W): interior pixels
    stored by the epilogue, the frame folded by elementwise.hip fold_band (xb1 / res are
    real-grid tensors)."""
    fk = {} if fold is None else dict(fold_H=int(fold[0]), fold_W=int(fold[1]), fold_p=int(fold[2]),
                                      fold_edge=int(fold[3]) if len(fold) > 3 else 0)
    C1 = x1.shape[1]
    C2 = 0 if x2 is None else x2.shape[1]
    if weight is not None and _f8.enabled() and _f8.conv_ok(C1, C2, Cout, act_in):
        fmt = _f8.E5M2 if role == "gy" else _f8.E4M3
        w8, sw = _weight_image_fp8(weight, swap, xp, yp)
        yq = ()
        if y_qkey is not None:
            ysite, fresh = _f8.producer_site(x1.device, y_qkey)
            yq = (None, 0) if fresh else (ysite, _f8.E4M3)
        k = _f8.obj_key(weight)
        a1, s1 = _f8.quant(x1, (k, role, 1), fmt)
        a2, s2 = _f8.quant(x2, (k, role, 2), fmt) if x2 is not None else (None, None)
        return P().conv_fwd(a1, a2, w8, bias, mode, KH, KW, s, p, reflect, up, act_in, OH, OW, Cout,
                            act_out, Csplit, xb1, xb2, act_bwd, Cvalid, want, s1, s2, sw, *yq, res=res,
                            alpha=alpha, **_nb_kwargs(nb if not yq else None), **fk)
    if wimg is None:
        wimg = _weight_image(weight, swap, xp, yp)
    yq = ()
    if y_qkey is not None and _f8.enabled():
        ysite, fresh = _f8.producer_site(x1.device, y_qkey)
        yq = (None, None, None, None, 0) if fresh else (None, None, None, ysite, _f8.E4M3)
    return P().conv_fwd(x1, x2, wimg, bias, mode, KH, KW, s, p, reflect, up, act_in, OH, OW, Cout,
                        act_out, Csplit, xb1, xb2, act_bwd, Cvalid, want, *yq, res=res, alpha=alpha,
                        **_nb_kwargs(nb if not yq else None), **fk)


def _nb_kwargs(nb):
    if nb is None:
        return {}
    half, info = nb
    if info is _CS:
        return dict(nb_half=half, nb_colsum=True)
    nx, nmean, nrstd, ng, nbeta, nact, nbatch, npw = info
    # the half's act' gate input is the norm's output registered for it (ctx.nb comes from
    # _norm_lookup of that very input): with no fused act and no affine it IS xhat, so the
    # epilogue gates from the xhat it already forms instead of re-reading the output.
    # Affine / shared-slope PReLU norms: batch norm only (the binding checks; family R's BNs,
    # whose partials the reflect-dgrad epilogue + fold_band emit)
    return dict(nb_x=nx, nb_mean=nmean, nb_rstd=nrstd, nb_gamma=ng, nb_beta=nbeta, nb_act=nact,
                nb_half=half, nb_batch=nbatch, nb_gate=(ng is None and not nact and npw is None),
                nb_prelu=npw)


def prepare_weights(*modules):
    """Cast every conv weight image (forward and dgrad layouts) of ``modules`` and seed the
    per-parameter cache: kernels up to 4x4 in one launch writing BOTH images from a single
    read (weight_prep_pairs), larger kernels (family R 5x5 / 7x7 / 9x9) through the
    per-layout multi-tensor cast -- instead of one launch per layout per layer on first use."""
    from ..models.layers import Conv2d, ConvTranspose2d
    pw, pa, pb, pkeys = [], [], [], []
    ws, sw, xp, yp, keys = [], [], [], [], []
    for mod in modules:
        for m in mod.modules():
            w = getattr(m, "weight", None)
            if not isinstance(w, torch.Tensor) or not w.is_cuda or w.dim() != 4:
                continue
            if not isinstance(m, (Conv2d, ConvTranspose2d)):
                continue
            wc = w.detach()
            if wc.dtype != torch.float32 or not wc.is_contiguous():
                continue
            # dim0 = A, dim1 = B for both module kinds: image 0 = [A][T][B], image 1 = [B][T][A]
            xa, xb = _pad8(w.shape[0]), _pad8(w.shape[1])
            if w.shape[2] * w.shape[3] <= 16:
                pw.append(wc)
                pa.append(xa)
                pb.append(xb)
                pkeys.append(w)
                continue
            for (s_, x_, y_) in ((0, xa, xb), (1, xb, xa)):
                ws.append(wc)
                sw.append(s_)
                xp.append(x_)
                yp.append(y_)
                keys.append((w, (s_, x_, y_, None)))
    entries = []
    if pw and _f8.enabled():
        # fp8 precision: e4m3 images (current scaling) for the layers the fp8 convs take,
        # bf16 images for the image-facing rest
        sel = [i for i in range(len(pw)) if _f8.pair_ok(pkeys[i].shape[0], pkeys[i].shape[1])]
        for j, (i0, i1, site) in zip(sel, _f8.prepare_weight_pairs(
                [pw[i] for i in sel], [pa[i] for i in sel], [pb[i] for i in sel],
                [pkeys[i] for i in sel])):
            w = pkeys[j]
            entries.append((w, (0, pa[j], pb[j], "fp8"), (i0, site)))
            entries.append((w, (1, pb[j], pa[j], "fp8"), (i1, site)))
        rest = [i for i in range(len(pw)) if i not in set(sel)]
        pw, pa, pb, pkeys = ([pw[i] for i in rest], [pa[i] for i in rest], [pb[i] for i in rest],
                             [pkeys[i] for i in rest])
    if pw:
        imgs = P().weight_prep_pairs(pw, pa, pb)
        for i, w in enumerate(pkeys):
            entries.append((w, (0, pa[i], pb[i], None), imgs[2 * i]))
            entries.append((w, (1, pb[i], pa[i], None), imgs[2 * i + 1]))
    if ws:
        imgs = P().weight_prep_multi(ws, sw, xp, yp)
        entries.extend((w, key, img) for (w, key), img in zip(keys, imgs))
    for w, key, img in entries:
        cache = getattr(w, "_p2p_cache", None)
        if cache is None:
            cache = {}
            w._p2p_cache = cache
        cache[key] = (w._version, _gen[0], img)


def _bias_padded(b, coutp):
    """fp32 bias padded to ``coutp`` columns: a persistent zero-tailed buffer cached on the
    bias tensor itself (dies with it), refreshed by a device copy each call (stream-ordered,
    graph-capturable; no pad kernel)."""
    if b is None:
        return None
    src = b.detach()
    if src.numel() == coutp:
        return src.float().contiguous()
    buf = getattr(b, "_p2p_bias_pad", None)
    if buf is None or buf.numel() != coutp or buf.device != src.device:
        buf = torch.zeros(coutp, device=src.device, dtype=torch.float32)
        try:
            b._p2p_bias_pad = buf
        except AttributeError:   # plain tensor without __dict__: a per-call buffer
            pass
    buf[: src.numel()].copy_(src)
    return buf


def _seed(device):
    s = _seeds.get(device)
    if s is None:
        s = torch.tensor([torch.initial_seed() & 0x7FFFFFFF], dtype=torch.int64, device=device)
        _seeds[device] = s
    return s


def advance_rng(device=None):
    """Advance the device-side dropout seed (captured into graphs as one tiny kernel).
    With ``device`` the seed is created first if needed, so the first step already draws
    from seed + 1 whether or not a warmup created the seed earlier (graph == eager)."""
    if device is not None:
        _seed(device)
    for d, s in _seeds.items():
        if device is None or d == device:
            P().i64_add_(s, 1)


# ============================================================== convolution
class _ConvCfg:
    """``grad_gate``: activation derivative (from the input value) applied to the input
    gradient in the dgrad epilogue -- the producer of this conv's input stored
    ``act(x)`` and set ``out_gated`` so it skips its own gate pass (valid only when every
    consumer of that output gates; the models wire both ends).

    ``skip_grad``: a tensor read by two convs (a U-Net skip: the decoder ConvT, whose backward
    runs first, and the next encoder conv) gets ONE gradient write instead of two plus an
    autograd add -- "defer": this conv's x1 gradient is parked in ``_DEFERRED`` (keyed by the
    tensor's storage) and not returned; "take": this conv's dgrad epilogue adds the parked
    gradient of its x1.  ``assert_no_deferred()`` checks after backward that every parked
    gradient was consumed."""
    __slots__ = ("transposed", "KH", "KW", "stride", "pad", "reflect", "up", "act_in", "act_out",
                 "stats", "grad_gate", "out_gated", "skip_grad", "gate_x2")

    def __init__(self, transposed, KH, KW, stride, pad, reflect, up, act_in, act_out, stats=False,
                 grad_gate=None, out_gated=False, skip_grad=None, gate_x2=True):
        self.skip_grad = skip_grad
        self.gate_x2 = gate_x2
        self.stats = stats
        self.grad_gate = grad_gate
        self.out_gated = out_gated
        self.transposed = transposed
        self.KH, self.KW = KH, KW
        self.stride, self.pad = stride, pad
        self.reflect, self.up = reflect, up
        self.act_in, self.act_out = act_in, act_out


def pack_pairs(pairs):
    """Channel-concat + zero-pad each ``(a, b)`` pair into one batch-stacked packed NHWC
    tensor (a pad-8 image conv input) with one kernel per pair and no ``torch.cat``
    (the fused 2B discriminator batch).  The result carries its logical channel split
    (``_p2p_packed``), so a conv reading it takes the packed path with the right weight
    layout; it is a constant (no gradient flows back to the pairs)."""
    a0, b0 = pairs[0]
    C1, C2 = a0.shape[1], b0.shape[1]
    N = sum(a.shape[0] for a, _ in pairs)
    out = torch.empty(N, _pad8(C1 + C2), a0.shape[2], a0.shape[3], device=a0.device,
                      dtype=torch.bfloat16, memory_format=CL)
    n0 = 0
    for a, b in pairs:
        if a.shape[1] != C1 or b.shape[1] != C2:
            raise ValueError("pack_pairs: every pair needs the same channel split")
        n = a.shape[0]
        P().pad_channels_into(to_nhwc_bf16(a.detach()), to_nhwc_bf16(b.detach()), out[n0:n0 + n])
        n0 += n
    out._p2p_packed = (C1, C2)
    return out


def _prep_inputs(x1, x2):
    """Return (q1, q2, C1, C2, Cp, packed): kernel inputs with 8-aligned channel counts."""
    pk = getattr(x1, "_p2p_packed", None)
    if pk is not None and x2 is None:   # pre-packed by pack_pairs()
        return x1, None, pk[0], pk[1], x1.shape[1], True
    x1 = to_nhwc_bf16(x1)
    C1 = x1.shape[1]
    if x2 is None:
        if C1 % 8 == 0:
            return x1, None, C1, 0, C1, False
        return P().pad_channels(x1, None, _pad8(C1)), None, C1, 0, _pad8(C1), True
    x2 = to_nhwc_bf16(x2)
    C2 = x2.shape[1]
    if C1 % 8 == 0 and C2 % 8 == 0:
        return x1, x2, C1, C2, C1 + C2, False
    cp = _pad8(C1 + C2)
    return P().pad_channels(x1, x2, cp), None, C1, C2, cp, True


_DEFERRED: dict = {}   # storage ptr -> parked input gradient (``_ConvCfg.skip_grad``)


def assert_no_deferred():
    """Every gradient parked by a skip_grad="defer" conv must have been consumed by its
    "take" partner during the same backward; a leftover would be a lost gradient."""
    if _DEFERRED:
        n = len(_DEFERRED)
        _DEFERRED.clear()
        raise RuntimeError(f"skip_grad: {n} deferred gradient(s) were never consumed")


class ConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x1, x2, weight, bias, cfg: _ConvCfg):
        # a packed (A | fake) image from ImageHeadFn: its input gradient is the fused head
        # gradient (d2s mode 2) instead of a plain dgrad
        ctx.head = getattr(x1, "_p2p_head", None) if x2 is None else None
        q1, q2, C1, C2, Cp, packed = _prep_inputs(x1, x2)
        N, _, H, W = q1.shape
        KH, KW, s, p = cfg.KH, cfg.KW, cfg.stride, cfg.pad
        if cfg.transposed:
            Cout = weight.shape[1]
            OH = (H - 1) * s - 2 * p + KH
            OW = (W - 1) * s - 2 * p + KW
            mode, swap = 1, 1
        else:
            Cout = weight.shape[0]
            OH = (H * cfg.up + 2 * p - KH) // s + 1
            OW = (W * cfg.up + 2 * p - KW) // s + 1
            mode, swap = 0, 0
        Coutp = _pad8(Cout)
        want = bool(cfg.stats) and Coutp == Cout
        # fp8: an output that feeds other convs directly (relu / lrelu epilogue, no norm)
        # gets its e4m3 shadow from the epilogue
        y_qkey = None
        if (_f8.enabled() and not cfg.stats and Coutp == Cout and Cout % 32 == 0
                and cfg.act_out in ("relu", "lrelu")):
            y_qkey = (_f8.obj_key(weight), "y")
        outs = _conv_call(q1, q2, None, _bias_padded(bias, Coutp), mode, KH, KW, s, p,
                          int(cfg.reflect), cfg.up, _act_code(cfg.act_in), OH, OW, Coutp,
                          _act_code(cfg.act_out), Coutp, None, None, 0, Cout, want,
                          weight, swap, Coutp, Cp, y_qkey=y_qkey)
        y = outs[0]
        if y_qkey is not None:
            if outs[-1].element_size() == 1:
                _f8.stash_shadow(y, outs[-1], _f8.producer_site(y.device, y_qkey)[0])
                outs = outs[:-1]
            elif _f8.producer_site(y.device, y_qkey)[1]:
                _f8.bootstrap_shadow(y, y_qkey, _f8.E4M3)
        if want and len(outs) == 2:
            _stash_stats(y, outs[1])
        if Coutp != Cout:
            y = P().slice_channels(y, 0, Cout)
        ctx.cfg = cfg
        ctx.geo = (C1, C2, Cp, packed, Cout, Coutp, H, W)
        ctx.has_x2 = x2 is not None
        ctx.has_bias = bias is not None
        ctx.bias_p = bias if (bias is not None and bias.is_leaf) else None   # gradient pairing
        ctx.nb = (None if packed else _norm_lookup(q1), _norm_lookup(q2))
        if (_NB_FUSE and bias is not None and bias.requires_grad and Coutp == Cout
                and (cfg.act_out in (None, "none") or cfg.out_gated)):
            _register_norm_out(y, _CS)
        keep_y = cfg.act_out not in (None, "none") and not cfg.out_gated
        ctx.save_for_backward(q1, q2, weight, y if keep_y else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        q1, q2, weight, y = ctx.saved_tensors
        need_x1 = ctx.needs_input_grad[0]
        if ctx.head is not None and need_x1 and _head_dgrad_ok(ctx.cfg, weight, q1):
            gx1 = _head_dgrad(ctx.head, q1, weight, to_nhwc_bf16(gy))
            gw = None
            if ctx.needs_input_grad[2] or (ctx.has_bias and ctx.needs_input_grad[3]):
                _, _, gw, gb = _conv_backward(ctx.cfg, ctx.geo, q1, q2, weight, y, gy, False, False,
                                              ctx.needs_input_grad[2],
                                              ctx.has_bias and ctx.needs_input_grad[3],
                                              side_ok=True, bias=ctx.bias_p)
                return gx1, None, gw, gb, None
            return gx1, None, None, None, None
        gx1, gx2, gw, gb = _conv_backward(ctx.cfg, ctx.geo, q1, q2, weight, y, gy, need_x1,
                                          ctx.has_x2 and ctx.needs_input_grad[1],
                                          ctx.needs_input_grad[2],
                                          ctx.has_bias and ctx.needs_input_grad[3], nb=ctx.nb,
                                          side_ok=True, bias=ctx.bias_p)
        return gx1, gx2, gw, gb, None


class SNConvFn(torch.autograd.Function):
    """y = act(conv(x, w_bar * s) + b) with s = 1 / sigma a DEVICE scalar (spectral norm,
    /root/reference/networks.py:543-549): the kernels scale the accumulator by s in the
    epilogue (conv.h ``alpha``), so W / sigma is never materialised and the bf16 weight image
    of w_bar is cast once per step for all of the step's D forwards.

    Backward: dx = dgrad(gy_eff, w_bar) * s (epilogue again); with G = wgrad(gy_eff, x),
    dL/dw_bar = s * G and dL/ds = <G, w_bar>, which autograd chains through s = 1 / sigma(w_bar)
    -- the same gradient as the reference's ``w / sigma``.  With ``uv`` = (u, v) (the power
    iteration's vectors, held by reference like SigmaFn) and a detached ``scale``, the whole
    w_bar gradient s G - <G, w_bar> s^2 u v^T is one fused pass (csrc/sn.hip sn_wgrad) instead
    of the scale / reciprocal / sigma autograd chain."""

    @staticmethod
    def forward(ctx, x, w_bar, bias, scale, cfg: _ConvCfg, uv=None):
        if cfg.transposed or cfg.reflect or cfg.up != 1:
            raise NotImplementedError("SNConvFn: plain zero-padded convs only")
        q1, _, C1, _, Cp, packed = _prep_inputs(x, None)
        N, _, H, W = q1.shape
        KH, KW, st, p = cfg.KH, cfg.KW, cfg.stride, cfg.pad
        Cout = w_bar.shape[0]
        OH = (H + 2 * p - KH) // st + 1
        OW = (W + 2 * p - KW) // st + 1
        Coutp = _pad8(Cout)
        sc = scale.detach().float().reshape(1).contiguous()
        outs = _conv_call(q1, None, None, _bias_padded(bias, Coutp), 0, KH, KW, st, p, 0, 1,
                          _act_code(cfg.act_in), OH, OW, Coutp, _act_code(cfg.act_out), Coutp, None,
                          None, 0, Cout, False, w_bar, 0, Coutp, Cp, alpha=sc)
        y = outs[0]
        if Coutp != Cout:
            y = P().slice_channels(y, 0, Cout)
        ctx.cfg = cfg
        ctx.geo = (C1, 0, Cp, packed, Cout, Coutp, H, W)
        ctx.has_bias = bias is not None
        ctx.bias_p = bias if (bias is not None and bias.is_leaf) else None   # gradient pairing
        ctx.w_p = w_bar if w_bar.is_leaf else None
        ctx.uv = uv
        keep_y = cfg.act_out not in (None, "none") and not cfg.out_gated
        ctx.save_for_backward(q1, w_bar, sc, y if keep_y else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        q1, w_bar, sc, y = ctx.saved_tensors
        need_w = ctx.needs_input_grad[1] or ctx.needs_input_grad[3]
        gx, _, G, gb = _conv_backward(ctx.cfg, ctx.geo, q1, None, w_bar, y, gy,
                                      ctx.needs_input_grad[0], False, need_w,
                                      ctx.has_bias and ctx.needs_input_grad[2], alpha=sc,
                                      bias=ctx.bias_p, pair=True)
        if ctx.uv is not None:
            u, v = ctx.uv
            wb = w_bar.detach()
            wb = wb if (wb.dtype == torch.float32 and wb.is_contiguous()) else wb.float().contiguous()
            gw = None
            if ctx.needs_input_grad[1]:
                first = _pair_first(ctx.w_p, True)   # the D phase's second pass: into the first
                if first is not None:
                    P().sn_wgrad(G, wb, u.detach(), v.detach(), sc, first)
                else:
                    gw = P().sn_wgrad(G, wb, u.detach(), v.detach(), sc)
                    _pair_set(ctx.w_p, gw, True)
            return gx, gw, gb, None, None, None
        gw = G * sc if ctx.needs_input_grad[1] else None
        gs = (G * w_bar.detach()).sum().reshape(1) if ctx.needs_input_grad[3] else None
        return gx, gw, gb, gs, None, None


def sn_scale(w2, u, v, iters=1):
    """1 / sigma of the power iteration (u, v updated in place) as a plain device scalar --
    the sigma path of the gradient is SNConvFn's fused sn_wgrad (pass ``uv`` to sn_conv2d)."""
    w = w2.detach()
    w = w if (w.dtype == torch.float32 and w.is_contiguous()) else w.float().contiguous()
    for _ in range(max(1, int(iters)) - 1):
        P().sn_power_iter(w, u.data, v.data)
    return P().sn_scale(w, u.data, v.data)


def sn_conv2d(x, w_bar, bias, scale, stride=1, padding=0, act_in=None, act_out=None,
              grad_gate=None, out_gated=False, uv=None, skip_grad=None):
    """Spectral-norm conv: ``conv2d(x, w_bar * scale)`` with ``scale`` (1 / sigma) applied in
    the conv epilogues -- either a 1-element tensor carrying its own gradient, or (``uv`` =
    (u, v)) a detached ``sn_scale`` with the sigma path fused into the weight gradient."""
    s, s2 = _pair(stride)
    p, p2 = _pair(padding)
    if s != s2 or p != p2:
        raise NotImplementedError("anisotropic stride/padding")
    cfg = _ConvCfg(False, w_bar.shape[2], w_bar.shape[3], s, p, False, 1, act_in, act_out,
                   grad_gate=grad_gate, out_gated=out_gated, skip_grad=skip_grad)
    return SNConvFn.apply(x, w_bar, bias, scale, cfg, uv)


def _nb_half(cfg, q2, nb, res_fused):
    """Which input half's dgrad epilogue emits norm-backward partials: one whose gradient this
    conv completes (not a deferred skip half; a "take" half only when its parked gradient is
    added in the epilogue)."""
    if nb is None:
        return None
    nb1, nb2 = nb
    if (nb1 is not None and cfg.skip_grad != "defer" and (cfg.skip_grad != "take" or res_fused)):
        return (1, nb1)
    if nb2 is not None and q2 is not None:
        return (2, nb2)
    return None


def _wgrad_fp8(cfg, weight, q1, q2, gyp, act_in):
    """fp8 weight gradient (BASELINE config 5): dY e5m2 x X e4m3 on the scaled f8f6f4 MFMA,
    reading the fp8 copies the forward / dgrad of this conv already made (``_f8.quant`` caches
    them per step under the same site keys) -- the image-facing layers stay bf16.  Returns
    None when the geometry is not the fp8 kernel's (the caller runs the bf16 wgrad), else
    (launch(gw) -> bool, operand tensors): the quantisation runs here, on the compute stream,
    the launch wherever the caller puts it (launch False: the caller runs the bf16 wgrad)."""
    if not _f8.enabled() or os.environ.get("P2P_FP8_WGRAD", "1") == "0":
        return None
    if cfg.reflect or cfg.up != 1 or act_in not in (0, 1):
        return None
    C1 = q1.shape[1]
    C2 = 0 if q2 is None else q2.shape[1]
    Cout = gyp.shape[1]
    # the kernel's own gate (conv_wgrad.hip p2p_conv_wgrad_f8_tile: R and taps x C multiples of
    # 128) decides the rest; 64-channel sides (U-Net e2 / d2) are covered since round 3
    if not (_f8.conv_ok(C1, C2, Cout, act_in) and C1 % 16 == 0 and C2 % 16 == 0 and Cout % 64 == 0
            and (C1 + C2) % 64 == 0 and C1 + C2 >= 64):
        return None
    k = _f8.obj_key(weight)
    x1q, sx = _f8.quant(q1, (k, "x", 1), _f8.E4M3)
    x2q = sx2 = None
    if q2 is not None:     # the concat halves keep their own scales (per-fragment exponents)
        x2q, sx2 = _f8.quant(q2, (k, "x", 2), _f8.E4M3)
    gq, sg = _f8.quant(gyp, (k, "gy", 1), _f8.E5M2)
    KH, KW, s, p = cfg.KH, cfg.KW, cfg.stride, cfg.pad

    def launch(gw, scale=1.0, acc=0):
        if cfg.transposed:
            return bool(P().conv_wgrad(x1q, x2q, act_in, gq, None, 0, KH, KW, s, p, 0, 1, gw, scale, acc,
                                       0, sx, sg, _f8.E4M3, _f8.E5M2, sx2, None))
        return bool(P().conv_wgrad(gq, None, 0, x1q, x2q, act_in, KH, KW, s, p, 0, 1, gw, scale, acc, 0,
                                   sg, sx, _f8.E5M2, _f8.E4M3, None, sx2))
    return launch, (x1q, x2q, gq, sx, sx2, sg)


def _conv_backward(cfg, geo, q1, q2, weight, y, gy, need_x1, need_x2, need_w, need_b, alpha=None,
                   nb=None, side_ok=False, bias=None, pair=False):
    """Input / weight / bias gradients of one fused conv (ConvFn's backward, shared with the
    image head): dgrad with the input-activation gate, concat split and skip-gradient
    hand-off in its epilogue; wgrad; bias = column sums (or the norm's exact zero).
    ``nb``: (x1, x2) norm-output infos (``_norm_lookup``) -- the dgrad epilogue emits the
    norm-backward partials of a half that is a norm's output.  ``side_ok``: the weight gradient
    is returned to autograd as is (not consumed here), so it may run on the wgrad side stream."""
    nbh = None
    nbp = None
    C1, C2, Cp, packed, Cout, Coutp, H, W = geo
    gy = to_nhwc_bf16(gy)
    if cfg.act_out not in (None, "none") and not cfg.out_gated:
        gy = P().act(gy, y, _act_code(cfg.act_out), 2)
    gyp = gy if (Coutp == Cout or gy.shape[1] == Coutp) else P().pad_channels(gy, None, Coutp)
    KH, KW, s, p = cfg.KH, cfg.KW, cfg.stride, cfg.pad
    gx1 = gx2 = gw = gb = None
    if need_x1 or need_x2:
        # input-gradient gate: the input activation's derivative, or the producer's
        act_in = _act_code(cfg.act_in) or _act_code(cfg.grad_gate)
        split = C1 if (q2 is not None) else Cp
        if cfg.reflect or cfg.up != 1:
            # family-R ConvLayer / UpsampleConvLayer: dgrad onto the virtual padded,
            # upsampled input (a plain pad-0 transposed conv), then fold it back
            if q2 is not None:
                raise NotImplementedError("virtual concat with reflect/upsample gather")
            Hp, Wp = H * cfg.up + 2 * p, W * cfg.up + 2 * p
            res = None
            if cfg.skip_grad == "take" and q2 is None and need_x1 and Cp == C1:
                res = _DEFERRED.pop(q1.data_ptr(), None)   # the residual add's gradient
                if res is not None and res.shape != (q1.shape[0], Cp, H, W):
                    _DEFERRED[q1.data_ptr()] = res   # not fusable: added below instead
                    res = None
            # (a batch norm's partials are NOT taken from a fold dgrad: built in round 5 and
            # measured slower -- the EXT epilogue costs the 256-row tiles more than the partial
            # pass it replaces, profiles/kernel_experiments_r5.md section 12 -- and removed in
            # round 6; the norm runs its own partial pass)
            nbh = None
            if (cfg.up == 2 and cfg.reflect and p == 1 and KH == 3 and KW == 3 and s == 1
                    and _UP_FOLD):
                # nearest x2 then reflect pad 1 == edge-replicate pad 1 of the upsample: the
                # dgrad is a 4x4 stride-2 pad-3 conv over dY with phase-summed taps onto the
                # edge-padded (H+2) x (W+2) grid, folded in the epilogue -- no 4x up-grid, 16
                # instead of 36 taps per input pixel (_up2_dgrad_image)
                outs = _conv_call(gyp, None, _up2_dgrad_image(weight, Cp, Coutp), None, 0, 4, 4, 2, 3,
                                  0, 1, 0, H + 2, W + 2, Cp, 0, Cp, q1 if act_in else None, None, act_in,
                                  C1, False, role="gy", res=res, fold=(H, W, 1, 1), nb=nbh)
            elif cfg.up == 1 and cfg.reflect and p > 0 and _FOLD_EPI:
                # reflect pad only: the fold happens in the dgrad's epilogue (interior pixels
                # gated + skip gradient straight into dx) plus a frame-band pass
                outs = _conv_call(gyp, None, None, None, 1, KH, KW, s, 0, 0, 1, 0, Hp, Wp, Cp,
                                  0, Cp, q1 if act_in else None, None, act_in, C1, False, weight,
                                  1, Cp, Coutp, "gy", res=res, fold=(H, W, p), nb=nbh)
            else:
                dxp = _conv_call(gyp, None, None, None, 1, KH, KW, s, 0, 0, 1, 0, Hp, Wp, Cp,
                                 0, Cp, None, None, 0, C1, False, weight, 1, Cp, Coutp, "gy")[0]
                outs = [P().pad_fold(dxp, H, W, p, cfg.up, int(cfg.reflect),
                                     q1 if act_in else None, act_in, res)]
        elif cfg.transposed:
            nbh = _nb_half(cfg, q2, nb, False) if not packed else None
            outs = _conv_call(gyp, None, None, None, 0, KH, KW, s, p, 0, 1, 0, H, W, Cp, 0,
                              split, q1 if act_in else None,
                              q2 if (act_in and q2 is not None and cfg.gate_x2) else None,
                              act_in, C1 + C2, False, weight, 0, Cp, Coutp, "gy", nb=nbh)
        else:
            res = None
            if cfg.skip_grad == "take" and q2 is None and not packed and need_x1:
                res = _DEFERRED.pop(q1.data_ptr(), None)
                if res is not None and (res.shape != (q1.shape[0], Cp, H, W) or Cp != C1):
                    _DEFERRED[q1.data_ptr()] = res   # not fusable: added below instead
                    res = None
            take_ok = res is not None or q1.data_ptr() not in _DEFERRED
            nbh = _nb_half(cfg, q2, nb, take_ok) if not packed else None
            # (an instance norm's partials are never fused on a grid that is not a multiple of
            # the tile rows -- the PatchGAN logits' 31 x 31 input -- so dropping nbh there
            # loses nothing: the norm runs its own partial pass either way)
            nb_lost = nbh is not None and (nbh[1] is _CS or nbh[1][6] or (H * W) % 128 == 0)
            if (Cout == 1 and s == 1 and KH * KW == 16 and q2 is None and not packed and not act_in
                    and res is None and not nb_lost and Cp == C1 and Cp % 8 == 0 and Cp <= 512
                    and (Cp // 8) & (Cp // 8 - 1) == 0 and weight.dtype == torch.float32
                    and weight.is_contiguous()
                    and os.environ.get("P2P_C1_DGRAD", "1") != "0"):
                # the logits conv (1 output channel): a bandwidth kernel instead of a K = 16 x 8
                # GEMM that is 7/8 zero padding (csrc/dgrad_c1.hip)
                outs = [P().dgrad_c1(gyp, weight.detach(), p, H, W, alpha)]
            else:
                outs = _conv_call(gyp, None, None, None, 1, KH, KW, s, p, 0, 1, 0, H, W, Cp, 0,
                                  split, q1 if act_in else None,
                                  q2 if (act_in and q2 is not None) else None, act_in, C1 + C2,
                                  False, weight, 1, Cp, Coutp, "gy", res=res, alpha=alpha, nb=nbh)
        nouts = 2 if q2 is not None else 1
        if nbh is not None and len(outs) > nouts:
            nbp = outs[nouts]
        if q2 is not None:
            gx1, gx2 = outs[0], outs[1]
        elif packed:
            g = outs[0]
            gx1 = P().slice_channels(g, 0, C1) if need_x1 else None
            gx2 = P().slice_channels(g, C1, C2) if need_x2 else None
        else:
            gx1 = outs[0]
        if nbp is not None:
            g_half = gx1 if nbh[0] == 1 else gx2
            if g_half is not None:
                if nbh[1] is _CS:
                    _stash_colsum(g_half, P().rowsum(nbp[0]))
                else:
                    _stash_nbp(g_half, nbp)
        if not need_x1:
            gx1 = None
        if not need_x2:
            gx2 = None
        if cfg.skip_grad == "take" and gx1 is not None and q2 is None:
            parked = _DEFERRED.pop(q1.data_ptr(), None)
            if parked is not None:
                gx1 = gx1 + parked
        if cfg.skip_grad == "defer" and gx1 is not None:
            key = q1.data_ptr()
            if key in _DEFERRED:
                raise RuntimeError("skip_grad: a deferred gradient of this tensor is pending")
            _DEFERRED[key] = gx1
            gx1 = None
    if need_w:
        # data-parallel direct gradient (parallel/ddp.py): the kernel accumulates straight
        # into the weight's bucket view, pre-scaled by 1/world, and the reducer is told --
        # autograd gets no gradient for the weight (no AccumulateGrad add, no rescale pass),
        # so the kernel may also run on the side stream
        red = getattr(weight, "_p2p_direct", None) if alpha is None else None
        direct = red is not None and red.direct_ok(weight)
        # a later contribution of this backward goes into the first one (see _pair_first);
        # the SN conv (alpha) pairs its final gradient in SNConvFn instead
        first = None if (direct or alpha is not None) else _pair_first(weight)
        if direct:
            gw, wscale, wacc = weight.grad, red.scale, 1
        elif first is not None:
            gw, wscale, wacc = first, 1.0, 1
        else:
            red_any = getattr(weight, "_p2p_direct", None)
            if (red_any is not None and id(weight) in red_any._direct_seen and _WgradSide.on is not None
                    and weight.is_cuda):
                # this weight was already written directly (side stream) in this backward and
                # now gets an autograd contribution: AccumulateGrad adds it on the compute
                # stream, which must not race the side-stream write
                torch.cuda.current_stream(weight.device).wait_stream(_WgradSide.on)
            gw = torch.empty_like(weight, dtype=torch.float32, memory_format=torch.contiguous_format)
            wscale, wacc = 1.0, 0
        act_in = _act_code(cfg.act_in)
        f8 = _wgrad_fp8(cfg, weight, q1, q2, gyp, act_in)
        if direct:
            side = _WgradSide.on if side_ok else None
            side = side or None
        else:
            side = _wgrad_side(weight) if side_ok else None
        if side is not None:
            side.wait_stream(torch.cuda.current_stream(side.device))
            _WgradSide.keep.append((q1, q2, gyp, f8))
        with (torch.cuda.stream(side) if side is not None else _NULLCTX):
            if f8 is not None and f8[0](gw, wscale, wacc):
                pass
            elif cfg.transposed:
                P().conv_wgrad(q1, q2, act_in, gyp, None, 0, KH, KW, s, p, 0, 1, gw, wscale, wacc)
            elif (s == 1 and Coutp <= 16 and Cp >= 128 and KH == KW and not cfg.reflect
                  and cfg.up == 1):
                # tiny-Cout stride-1 conv (PatchGAN logits): the GEMM's R = Cout would waste
                # the MFMA tile, so compute it in transposed-conv form -- rows = input
                # channels, the dY gather with pad K-1-p, taps flipped by the reduce
                P().conv_wgrad(q1, q2, act_in, gyp, None, 0, KH, KW, 1, KH - 1 - p, 0, 1, gw,
                               wscale, wacc, 1)
            else:
                P().conv_wgrad(gyp, None, 0, q1, q2, act_in, KH, KW, s, p, int(cfg.reflect),
                               cfg.up, gw, wscale, wacc)
        if direct:
            red.direct_done(weight, side)
            gw = None
        elif first is not None:
            gw = None
        elif alpha is None:
            _pair_set(weight, gw)
    if need_b:
        gb = _take_colsum(gy) if (cfg.act_out in (None, "none") or cfg.out_gated) else None
        first_b = _pair_first(bias, pair)
        if first_b is not None:
            if gb is not None:
                P().lincomb_(first_b, gb, 1.0, 1.0, 0.0)
            else:
                P().colsum(gyp, first_b, 1.0, True)
            gb = None
        else:
            if gb is None:
                gb = torch.empty(Cout, device=gy.device, dtype=torch.float32)
                P().colsum(gyp, gb, 1.0, False)
            _pair_set(bias, gb, pair)
    return gx1, gx2, gw, gb


# ============================================================== packed image head
# The pix2pix step's image-facing layers run on ONE packed [N][8][H][W] bf16 pair tensor
# per batch half (16 B per pixel: A in channels 0..2, B or the generated image in 3..5,
# zeros in 6..7) -- csrc/image.hip.  The generator's first conv reads (A | B) with zero
# weights on the B channels; its last transposed conv writes (A | fake) in place through the
# depth-to-space epilogue together with the L1 term; the discriminator reads the 2B stack
# [(A | fake); (A | B)] directly; and its first conv's input gradient comes back as the
# generator's pre-tanh gradient (L1 sign term and tanh' fused in), so no 3-channel tensor,
# channel pad / slice, col2im, tanh' or L1 kernel remains.
#
# The L1 value returned by image_head is an ordinary differentiable output: its gradient
# lambda * sign(fake - B) / n times dL/d(L1) is fused into D's first-conv dgrad, which reads
# dL/d(L1) from a device scalar that ``head_l1_tap`` (applied where the loss is composed)
# fills during backward; untapped, ImageHeadFn's backward adds the term itself.


# union GEMM columns: 16 = the halo-tile kernel (csrc/halo_conv.hip); 32 = the implicit-GEMM
# 256x32 glds tile (conv_fwd_glds.hip variant 7), kept as the A/B reference path
UNION_ROWS = 16


def _head_dgrad_ok(cfg, weight, x):
    return (not cfg.transposed and cfg.KH == 4 and cfg.KW == 4 and cfg.stride == 2
            and cfg.pad == 1 and cfg.up == 1 and not cfg.reflect and cfg.act_in is None
            and weight.shape[1] == 6 and weight.shape[0] % 64 == 0 and x.shape[1] == 8)


def _head_dgrad(head, af, weight, gy):
    """d(loss)/d(pre-tanh fake) in slots 0..2 of a packed tensor: the first D conv's input
    gradient on the fake channels (3..5) as a 3x3 union GEMM, + the L1 sign term, x tanh'.

    The L1 term's weight is dL/d(l1), read by the kernel from a device scalar that the L1
    value's gradient tap (``head_l1_tap``) writes -- so any recomposition or rescaling of the
    loss is honoured.  If no tap has delivered that weight yet (the L1 value is not in the
    loss, or it was not tapped), the term is left out here (weight 0) and ImageHeadFn's
    backward adds it with the weight autograd hands it."""
    ab, scale, state = head
    img, _ = P().union_weight(weight.detach().float().contiguous(), 3, 3, UNION_ROWS,
                              gy.shape[1], None)
    zb = _ZB.get(gy.device)
    if zb is None:     # the dgrad's (absent) bias: a persistent zero vector, read only
        zb = _ZB[gy.device] = torch.zeros(UNION_ROWS, device=gy.device, dtype=torch.float32)
    dz = torch.empty_like(af, memory_format=CL)
    tapped = state.tap_ran
    P().conv_d2s(gy, None, img, zb, 0, 0, 2, dz, ab, af, float(scale) if tapped else 0.0,
                 state.weight if tapped else None)
    dz._p2p_dz = True
    dz._p2p_l1_in = tapped
    return dz


_ZB = {}


class _HeadL1State:
    """Per-forward hand-off between the L1 value's gradient tap and the head's fused dgrad
    (``weight`` is read only after the tap has written it)."""
    __slots__ = ("weight", "tap_ran")

    def __init__(self, device):
        self.weight = torch.empty(1, device=device, dtype=torch.float32)
        self.tap_ran = False


class _L1TapFn(torch.autograd.Function):
    """Identity on the image head's L1 value whose backward stores dL/d(l1) on the device for
    the fused head dgrad.  Apply it where the loss is composed (after D's forward): autograd
    runs ready nodes latest-created first, so the tap's backward runs before D's backward
    reaches the head dgrad (``_head_dgrad`` checks that on the host)."""

    @staticmethod
    def forward(ctx, l1, state):
        ctx.state = state
        return l1.view_as(l1)

    @staticmethod
    def backward(ctx, g):
        ctx.state.weight.copy_(g.detach().reshape(1).float())
        ctx.state.tap_ran = True
        return g, None


def head_l1_tap(l1):
    """Tap the L1 value returned by the packed image head (no-op for any other tensor)."""
    state = getattr(l1, "_p2p_head_l1", None)
    return l1 if state is None else _L1TapFn.apply(l1, state)


class ImageHeadFn(torch.autograd.Function):
    """The generator's last layer, ``tanh(ConvT4x4s2p1(relu(cat(skip, u))) + b)``, written as
    the fake half of the packed pair tensor ``dd[:N]`` (with A copied from ``dd[N:]``)."""

    @staticmethod
    def forward(ctx, skip, u, weight, bias, dd, scale, cfg):
        skip, u = to_nhwc_bf16(skip), to_nhwc_bf16(u)
        N = skip.shape[0]
        ab = dd.narrow(0, N, N)
        af = dd.narrow(0, 0, N)
        img, bu = P().union_weight(weight.detach().float().contiguous(), 0, 3, UNION_ROWS,
                                   skip.shape[1] + u.shape[1],
                                   None if bias is None else bias.detach().float().contiguous())
        l1 = P().conv_d2s(skip, u, img, bu, _act_code(cfg.act_in), _act_code("tanh"), 1, af, ab,
                          None, float(scale))
        ctx.cfg = cfg
        ctx.scale = float(scale)
        ctx.has_bias = bias is not None
        ctx.geo = (skip.shape[1], u.shape[1], skip.shape[1] + u.shape[1], False, 3, 8,
                   skip.shape[2], skip.shape[3])
        ctx.save_for_backward(skip, u, weight, af, ab)
        ctx.nb = (None, _norm_lookup(u))
        state = _HeadL1State(skip.device)
        af._p2p_packed = (3, 3)
        af._p2p_head = (ab, float(scale), state)
        l1._p2p_head_l1 = state
        return af, l1

    @staticmethod
    def backward(ctx, gaf, gl1):
        skip, u, weight, af, ab = ctx.saved_tensors
        if getattr(gaf, "_p2p_dz", False):
            dz = gaf                       # fused by the consumer (_head_dgrad)
            if not gaf._p2p_l1_in and gl1 is not None:
                # the dgrad ran before any tap delivered dL/dl1: add the L1 term here
                f = af[:, 3:6].float()
                t = gl1.float() * ctx.scale * torch.sign(f - ab[:, 3:6].float()) * (1 - f * f)
                dz = dz.clone(memory_format=CL)
                dz[:, 0:3] = (dz[:, 0:3].float() + t).to(torch.bfloat16)
        else:                              # any other consumer: the same math, unfused
            f = af[:, 3:6].float()
            g = gaf[:, 3:6].float()
            if gl1 is not None:
                g = g + gl1.float() * ctx.scale * torch.sign(f - ab[:, 3:6].float())
            dz = torch.zeros_like(af, memory_format=CL)
            dz[:, 0:3] = (g * (1 - f * f)).to(torch.bfloat16)
        cfg = _ConvCfg(True, 4, 4, 2, 1, False, 1, ctx.cfg.act_in, None,
                       skip_grad=ctx.cfg.skip_grad, gate_x2=ctx.cfg.gate_x2)
        gx1, gx2, gw, gb = _conv_backward(cfg, ctx.geo, skip, u, weight, None, dz,
                                          ctx.needs_input_grad[0], ctx.needs_input_grad[1],
                                          ctx.needs_input_grad[2],
                                          ctx.has_bias and ctx.needs_input_grad[3], nb=ctx.nb,
                                          side_ok=True)
        if gb is not None:
            gb = gb[:3].contiguous()
        return gx1, gx2, gw, gb, None, None, None


def image_head(skip, u, module, dd, scale):
    """(A | fake) written into ``dd[:N]`` by ``module`` (the U-Net's outermost ConvTranspose2d,
    4x4 s2 p1, input ReLU, tanh) plus ``scale * sum|fake - B|`` (the L1 term)."""
    cfg = _ConvCfg(True, 4, 4, 2, 1, False, 1, module.act_in, "tanh",
                   skip_grad=module.skip_grad, gate_x2=getattr(module, "gate_x2", True))
    return ImageHeadFn.apply(skip, u, module.weight, module.bias, dd, float(scale), cfg)


def image_head_ok(module, skip, u) -> bool:
    w = module.weight
    return (w.shape[1] == 3 and tuple(w.shape[2:]) == (4, 4) and module.stride[0] == 2
            and module.padding[0] == 1 and module.act_in == "relu" and module.act_out == "tanh"
            and skip.shape[1] % 64 == 0 and u.shape[1] % 64 == 0
            and skip.shape[1] + u.shape[1] == w.shape[0])


def _split_input(x):
    if isinstance(x, (tuple, list)):
        if len(x) != 2:
            raise ValueError("virtual concat takes exactly two tensors")
        return x[0], x[1]
    return x, None


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def conv2d(x, weight, bias=None, stride=1, padding=0, pad_mode="zeros", upsample=1,
           act_in=None, act_out=None, stats=False, grad_gate=None, out_gated=False, skip_grad=None):
    s, s2 = _pair(stride)
    p, p2 = _pair(padding)
    if s != s2 or p != p2:
        raise NotImplementedError("anisotropic stride/padding")
    x1, x2 = _split_input(x)
    cfg = _ConvCfg(False, weight.shape[2], weight.shape[3], s, p, pad_mode == "reflect" and p > 0,
                   int(upsample or 1), act_in, act_out, stats, grad_gate, out_gated, skip_grad)
    return ConvFn.apply(x1, x2, weight, bias, cfg)


def conv_transpose2d(x, weight, bias=None, stride=2, padding=1, act_in=None, act_out=None,
                     stats=False, grad_gate=None, out_gated=False, skip_grad=None, gate_x2=True):
    x1, x2 = _split_input(x)
    cfg = _ConvCfg(True, weight.shape[2], weight.shape[3], int(stride), int(padding), False, 1,
                   act_in, act_out, stats, grad_gate, out_gated, skip_grad, gate_x2)
    return ConvFn.apply(x1, x2, weight, bias, cfg)


# ============================================================== spectral norm
class SigmaFn(torch.autograd.Function):
    """sigma of the spectral-norm power iteration (csrc/sn.hip), u / v updated in place.

    Backward: d sigma / d W = u v^T.  u and v are held by reference, not saved: like the
    reference's ``.data`` swaps (networks.py:543-546), a backward through an earlier forward
    of the step sees the newest u / v."""

    @staticmethod
    def forward(ctx, w2, u, v, iters):
        w = w2.detach()
        w = w if (w.dtype == torch.float32 and w.is_contiguous()) else w.float().contiguous()
        sigma = None
        for _ in range(max(1, int(iters))):
            sigma = P().sn_power_iter(w, u.data, v.data)
        ctx.uv = (u, v)
        return sigma

    @staticmethod
    def backward(ctx, g):
        u, v = ctx.uv
        return g * torch.outer(u.detach(), v.detach()), None, None, None


def spectral_sigma(w2, u, v, iters=1):
    return SigmaFn.apply(w2, u, v, iters)


# ============================================================== normalisation
class NormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, prelu_w, run_mean, run_var, eps, momentum, act, batch,
                training, qkey=None, res=None, defer_res=False):
        """``res``: residual added before ``act`` in the apply pass, y = act(norm(x) + res) (the
        family-R residual join; ReLU / LeakyReLU only).  Its gradient is act'(y) * dy, parked
        for the conv that also reads ``res`` when ``defer_res`` (``skip_grad="take"``)."""
        x = to_nhwc_bf16(x)
        ctx.res_key = None
        ctx.has_res = res is not None
        if res is not None:
            if prelu_w is not None or act not in ("relu", "lrelu"):
                raise ValueError("norm with residual: ReLU / LeakyReLU only, no PReLU")
            if defer_res and res.dtype == torch.bfloat16 and res.is_contiguous(memory_format=CL):
                ctx.res_key = res.data_ptr()   # the storage the consuming conv reads
            res = to_nhwc_bf16(res)
        g = gamma.detach().float().contiguous() if gamma is not None else None
        b = beta.detach().float().contiguous() if beta is not None else None
        pw = prelu_w.detach().float().contiguous() if prelu_w is not None else None
        # fp8: the normalised output is the next conv's operand -> e4m3 shadow from the apply
        # pass; the input gradient (backward) the producing conv's dgrad operand -> e5m2
        qkey = qkey if (qkey is not None and _f8.enabled() and training
                        and x.shape[1] % 32 == 0) else None
        ctx.qkey = qkey
        if training:
            qargs, qy, ysite, fresh = (), None, None, False
            if qkey is not None:
                ysite, fresh = _f8.producer_site(x.device, (qkey, "y"))
                if not fresh:
                    qy = _f8.shadow_buffer(x, _f8.E4M3)
                    qargs = (ysite, qy, _f8.E4M3)
            y, mean, rstd = P().norm_fwd(x, eps, g, b, pw, _act_code(act),
                                         run_mean if batch else None, run_var if batch else None,
                                         momentum, batch, _take_stats(x), *qargs, res=res)
            if qy is not None:
                _f8.stash_shadow(y, qy, ysite)
            elif fresh:
                _f8.bootstrap_shadow(y, (qkey, "y"), _f8.E4M3)
        else:
            mean = run_mean.float().view(1, -1)
            rstd = torch.rsqrt(run_var.float() + eps).view(1, -1)
            y = P().norm_apply(x, mean, rstd, g, b, pw, _act_code(act), True, res=res)
        ctx.cfg = (eps, act, batch, training)
        if (training and (pw is None or batch) and act in (None, "none", "relu", "lrelu") and _NB_FUSE
                and res is None):
            _register_norm_out(y, (x, mean, rstd, g, b, _act_code(act), bool(batch), pw))
        # the gate of a post-residual activation needs y (not recomputable from x alone)
        keep_y = act not in (None, "none") and (act not in ("relu", "lrelu") or not training
                                                or res is not None)
        ctx.save_for_backward(x, mean, rstd, gamma, beta, prelu_w, y if keep_y else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, mean, rstd, gamma, beta, prelu_w, y = ctx.saved_tensors
        eps, act, batch, training = ctx.cfg
        gy = to_nhwc_bf16(gy)
        gres = None
        if ctx.has_res:
            # y = act(z + res): one gated gradient for both z (the norm) and res
            gy = P().act(gy, y, _act_code(act), 2)
            act = None
            if ctx.res_key is not None and ctx.needs_input_grad[12]:
                if ctx.res_key in _DEFERRED:
                    raise RuntimeError("skip_grad: a deferred gradient of this tensor is pending")
                _DEFERRED[ctx.res_key] = gy
            elif ctx.needs_input_grad[12]:
                gres = gy
        gpw = None
        fused_act = 0
        pw = None
        if prelu_w is not None:
            # y = prelu(z): the kernels recompute z from x, gate dz = dy * (z > 0 ? 1 : w) and
            # reduce dw = sum(dy * z * [z <= 0]) in the same partial-sum pass
            pw = prelu_w.detach().float().contiguous()
            if ctx.needs_input_grad[3]:
                gpw = torch.empty(1, device=x.device, dtype=torch.float32)
        elif act in ("relu", "lrelu"):
            fused_act = _act_code(act)  # gate recomputed inside the norm backward kernels
        elif act not in (None, "none"):
            gy = P().act(gy, y, _act_code(act), 2)
        need_x = ctx.needs_input_grad[0]
        dg = db = None
        if gamma is not None and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]):
            dg = torch.empty_like(gamma, dtype=torch.float32)   # written whole by the kernel
            db = torch.empty_like(gamma, dtype=torch.float32)
        g = gamma.detach().float().contiguous() if gamma is not None else None
        b = beta.detach().float().contiguous() if beta is not None else None
        if not training:
            # eval-mode BN: an affine map with frozen statistics -- the same HIP passes with
            # dx = rstd * gamma * dz (no mean terms) and the parameter / slope gradients
            dx = P().norm_bwd(x, gy, mean, rstd, g, b, fused_act, dg, db, need_x, True, None,
                              prelu_w=pw, dprelu=gpw, frozen=True)
            gpw = _pair_slope_grad(prelu_w, gpw)
            return (dx if need_x else None), dg, db, gpw, None, None, None, None, None, None, None, None, gres, None
        dsum = torch.empty(x.shape[1], device=x.device, dtype=torch.float32) if need_x else None
        qargs, qd, dsite, fresh = (), None, None, False
        if ctx.qkey is not None and need_x:
            dsite, fresh = _f8.producer_site(x.device, (ctx.qkey, "dx"))
            if not fresh:
                qd = _f8.shadow_buffer(x, _f8.E5M2)
                qargs = (dsite, qd, _f8.E5M2)
        parts = _take_nbp(gy)
        if _NB_LOG:   # which norm backwards still run the partial-sum pass (tools/diag)
            print(f"[nb] {'fused' if parts is not None else 'PARTIAL PASS'} x{tuple(x.shape)} "
                  f"act={act} batch={bool(batch)}", file=sys.stderr)
        if parts is not None:
            dx = P().norm_bwd(x, gy, mean, rstd, g, b, fused_act, dg, db, need_x, batch, dsum,
                              *(qargs or (None, None, 0)), prelu_w=pw,
                              dprelu=gpw if pw is not None else None, partials=parts)
        elif qargs:
            dx = P().norm_bwd(x, gy, mean, rstd, g, b, fused_act, dg, db, need_x, batch, dsum,
                              *qargs, prelu_w=pw, dprelu=gpw if pw is not None else None)
        else:
            dx = P().norm_bwd(x, gy, mean, rstd, g, b, fused_act, dg, db, need_x, batch, dsum,
                              prelu_w=pw, dprelu=gpw if pw is not None else None)
        if need_x:
            _stash_colsum(dx, dsum)
            if qd is not None:
                _f8.stash_shadow(dx, qd, dsite)
            elif fresh:
                _f8.bootstrap_shadow(dx, (ctx.qkey, "dx"), _f8.E5M2)
        gpw = _pair_slope_grad(prelu_w, gpw)
        return (dx if need_x else None), dg, db, gpw, None, None, None, None, None, None, None, None, gres, None


def _pair_slope_grad(prelu_w, gpw):
    """A shared PReLU slope (family R: one slope, five sites, train and eval mode alike): its
    later gradients of this backward are added into the first in place (HIP) instead of by
    autograd (aten).  Every contribution to a paired leaf must come through here: autograd
    would sum an unpaired one out of place and the in-place adds into the first would be lost
    (``tests/test_family_r_gpu.py::test_grad_pairing_matches_autograd_sum``)."""
    if gpw is None:
        return None
    first = _pair_first(prelu_w)
    if first is not None:
        P().lincomb_(first, gpw, 1.0, 1.0, 0.0)
        return None
    _pair_set(prelu_w, gpw)
    return gpw


class _PadCFn(torch.autograd.Function):
    """Zero-pad the channel dim to a multiple of 8 (norm kernels move 8-channel vectors)."""

    @staticmethod
    def forward(ctx, x, cp):
        x = to_nhwc_bf16(x)
        ctx.c = x.shape[1]
        return P().pad_channels(x, None, cp)

    @staticmethod
    def backward(ctx, g):
        g = to_nhwc_bf16(g)
        out = P().slice_channels(g, 0, ctx.c)
        cs = _take_colsum(g)   # the norm's exact-zero bias gradient follows the slice
        if cs is not None:
            _stash_colsum(out, cs[:ctx.c])
        return out, None


class _SliceCFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, c):
        ctx.cp = x.shape[1]
        return P().slice_channels(x, 0, c)

    @staticmethod
    def backward(ctx, g):
        return P().pad_channels(to_nhwc_bf16(g), None, ctx.cp), None


def _norm_any_c(x, gamma, beta, prelu_w, run_mean, run_var, eps, momentum, act, batch, training,
                qkey=None):
    C = x.shape[1]
    if C % 8 == 0:
        return NormFn.apply(x, gamma, beta, prelu_w, run_mean, run_var, eps, momentum, act, batch,
                            training, qkey)
    # odd channel counts (family-R tail BN(3)): pad to 8 with identity channels, slice back
    # (the per-channel vectors padded / copied back by a HIP kernel, not aten cat / copy)
    cp = _pad8(C)
    g8 = b8 = rm8 = rv8 = None
    if gamma is not None:
        g8 = _VecPadFn.apply(gamma, cp, 1.0)
        b8 = _VecPadFn.apply(beta, cp, 0.0)
    if run_mean is not None:
        rm8 = _vec_pad(run_mean, cp, 0.0)
        rv8 = _vec_pad(run_var, cp, 1.0)
    y8 = NormFn.apply(_PadCFn.apply(x, cp), g8, b8, prelu_w, rm8, rv8, eps, momentum, act, batch,
                      training)
    if run_mean is not None and training:
        with torch.no_grad():
            P().vec_pad_into(rm8[:C], run_mean, 0.0)
            P().vec_pad_into(rv8[:C], run_var, 0.0)
    return _SliceCFn.apply(y8, C)


def _vec_pad(v, n, fill):
    out = torch.empty(n, device=v.device, dtype=torch.float32)
    P().vec_pad_into(v.detach().float().contiguous(), out, float(fill))
    return out


class _VecPadFn(torch.autograd.Function):
    """A norm's affine vector padded with ``fill`` to ``n`` channels; its gradient is the
    leading slice (a view: no kernel)."""

    @staticmethod
    def forward(ctx, v, n, fill):
        ctx.c = v.shape[0]
        return _vec_pad(v, n, fill)

    @staticmethod
    def backward(ctx, g):
        return g[:ctx.c], None, None


def instance_norm(x, eps=1e-5, act=None, weight=None, bias=None, qkey=None):
    """``qkey``: stable per-module key of the fp8 shadow scale sites (fp8 precision only)."""
    return _norm_any_c(x, weight, bias, None, None, None, eps, 0.0, act, False, True, qkey)


def batch_norm(x, running_mean, running_var, weight, bias, training, momentum=0.1, eps=1e-5,
               act=None, prelu_weight=None, qkey=None, residual=None, defer_residual=False):
    if not training and running_mean is None:
        training = True
    if residual is not None:
        if x.shape[1] % 8:
            raise ValueError("batch_norm with residual: channels must be a multiple of 8")
        return NormFn.apply(x, weight, bias, None, running_mean, running_var, eps, momentum, act,
                            True, training, qkey, residual, defer_residual)
    return _norm_any_c(x, weight, bias, prelu_weight, running_mean, running_var, eps, momentum,
                       act, True, training, qkey)


# ============================================================== elementwise
class ActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, name):
        x = to_nhwc_bf16(x) if x.dim() == 4 else x.to(torch.bfloat16).contiguous()
        y = P().act(x, None, _act_code(name), 0)
        ctx.name = name
        ctx.save_for_backward(x if name in ("relu", "lrelu") else y)
        return y

    @staticmethod
    def backward(ctx, gy):
        (t,) = ctx.saved_tensors
        gy = to_nhwc_bf16(gy) if gy.dim() == 4 else gy.to(torch.bfloat16).contiguous()
        mode = 1 if ctx.name in ("relu", "lrelu") else 2
        return P().act(gy, t, _act_code(ctx.name), mode), None


def act(x, name):
    return ActFn.apply(x, name)


class AddActFn(torch.autograd.Function):
    """y = act(a + b) in one pass (act kernel mode 3); the gradient gates on the output sign,
    which equals the sign of a + b for relu / lrelu, and flows unchanged to both inputs.
    ``defer_b``: b's gradient is parked in ``_DEFERRED`` for the conv that also reads b
    (``skip_grad="take"``: a residual block's first conv), which adds it in its dgrad
    epilogue / pad fold -- no autograd accumulate kernel for the residual input."""

    @staticmethod
    def forward(ctx, a, b, name, defer_b=False):
        a = to_nhwc_bf16(a)
        ctx.defer_key = None
        if defer_b and b.dtype == torch.bfloat16 and b.is_contiguous(memory_format=CL):
            ctx.defer_key = b.data_ptr()   # the storage the consuming conv reads (no copy)
        b = to_nhwc_bf16(b)
        y = P().act(a, b, _act_code(name), 3)
        ctx.name = name
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        g = P().act(to_nhwc_bf16(gy), y, _act_code(ctx.name), 2)
        if ctx.defer_key is not None and ctx.needs_input_grad[1]:
            if ctx.defer_key in _DEFERRED:
                raise RuntimeError("skip_grad: a deferred gradient of this tensor is pending")
            _DEFERRED[ctx.defer_key] = g
            return g, None, None, None
        return g, g, None, None


def add_act(a, b, name, defer_b=False):
    return AddActFn.apply(a, b, name, defer_b)


class FanOutFn(torch.autograd.Function):
    """One activation read by ``n`` consumers (family R: the generated image feeds D's first
    conv, its pooling pyramid, VGG and TV; the expander's residual trunk input feeds the trunk
    and the long skip): ``n`` aliases go to autograd, and their gradients meet here, summed
    by the bf16 add of the act kernel (mode 3, act none) -- instead of an aten add per extra
    consumer in autograd's input buffer."""

    @staticmethod
    def forward(ctx, x, n):
        ctx.dtype = x.dtype
        return tuple(x.view_as(x) for _ in range(n))

    @staticmethod
    def backward(ctx, *gs):
        gs = [g for g in gs if g is not None]
        if not gs:
            return None, None
        if ctx.dtype != torch.bfloat16 or any(g.dtype != torch.bfloat16 for g in gs):
            # not the bf16 activation path: sum in the gradients' own dtype, exactly as
            # autograd's input buffer would (no silent narrowing of an fp32 gradient)
            acc = gs[0]
            for g in gs[1:]:
                acc = acc + g
            return acc.to(ctx.dtype), None
        acc = None
        for g in gs:
            g = to_nhwc_bf16(g)
            acc = g if acc is None else P().act(acc, g, 0, 3)
        return acc, None


def fan_out(x, n):
    if n <= 1:
        return (x,)
    return FanOutFn.apply(x, int(n))


class LinCombFn(torch.autograd.Function):
    """wa * a + wb * b of fp32 loss scalars (the step's loss composition) on a HIP kernel."""

    @staticmethod
    def forward(ctx, a, b, wa, wb):
        ctx.w = (wa, wb)
        return P().lincomb(a.float().contiguous(), b.float().contiguous(), wa, wb, 0.0)

    @staticmethod
    def backward(ctx, g):
        wa, wb = ctx.w
        g = g.float().contiguous()
        ga = P().lincomb(g, None, wa, 0.0, 0.0) if ctx.needs_input_grad[0] else None
        gb = P().lincomb(g, None, wb, 0.0, 0.0) if ctx.needs_input_grad[1] else None
        return ga, gb, None, None


def lincomb(a, b, wa=1.0, wb=1.0):
    """``wa * a + wb * b`` for same-shape fp32 tensors (loss scalars)."""
    return LinCombFn.apply(a, b, float(wa), float(wb))


class LinCombNFn(torch.autograd.Function):
    """sum_i w_i * t_i of up to 16 fp32 loss scalars: one HIP launch forward, one backward
    (the composed losses of the reference step: GAN + feature matching + VGG + TV ...)."""

    @staticmethod
    def forward(ctx, ws, *ts):
        ctx.ws = ws
        return P().lincomb_n([t.float() for t in ts], list(ws))

    @staticmethod
    def backward(ctx, g):
        gs = P().scale_n(g.float(), list(ctx.ws))
        return (None,) + tuple(gs[i] for i in range(len(ctx.ws)))


def lincomb_n(terms, weights):
    """``sum(w * t)`` over fp32 scalar tensors (python-float terms are constants and are
    dropped from the gradient; at most 16 tensor terms per launch)."""
    ts, ws, const = [], [], 0.0
    for t, w in zip(terms, weights):
        if isinstance(t, torch.Tensor):
            ts.append(t)
            ws.append(float(w))
        else:
            const += float(w) * float(t)
    if const != 0.0 or not ts:
        raise ValueError("lincomb_n: tensor terms only")
    out = None
    for i in range(0, len(ts), 15):      # chains of 15 + the running total
        chunk_t, chunk_w = ts[i:i + 15], ws[i:i + 15]
        if out is not None:
            chunk_t, chunk_w = [out] + chunk_t, [1.0] + chunk_w
        out = LinCombNFn.apply(tuple(chunk_w), *chunk_t)
    return out


class _BatchHalvesFn(torch.autograd.Function):
    """(x[:n], x[n:]) whose gradients are written into one buffer by two device copies --
    instead of two slice backwards (a zero fill each) and an accumulate."""

    @staticmethod
    def forward(ctx, x, n):
        ctx.n = n
        ctx.shape, ctx.dtype = x.shape, x.dtype
        ctx.cl = x.dim() == 4 and x.is_contiguous(memory_format=CL)
        return x.narrow(0, 0, n), x.narrow(0, n, x.shape[0] - n)

    @staticmethod
    def backward(ctx, g1, g2):
        n = ctx.n
        ref = g1 if g1 is not None else g2
        mf = CL if ctx.cl else torch.contiguous_format
        out = torch.empty(ctx.shape, device=ref.device, dtype=ctx.dtype, memory_format=mf)
        for g, lo, ln in ((g1, 0, n), (g2, n, ctx.shape[0] - n)):
            dst = out.narrow(0, lo, ln)
            if g is None:
                dst.zero_()
            else:
                dst.copy_(g)
        return out, None


def batch_halves(x, n):
    return _BatchHalvesFn.apply(x, n)


class DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, salt):
        x = to_nhwc_bf16(x)
        seed = _seed(x.device)
        ctx.p, ctx.salt = p, salt
        ctx.save_for_backward(seed.clone())
        return P().dropout(x, p, seed, salt)

    @staticmethod
    def backward(ctx, gy):
        (seed,) = ctx.saved_tensors
        return P().dropout(to_nhwc_bf16(gy), ctx.p, seed, ctx.salt), None, None


def new_salt() -> int:
    return next(_salt) & 0x7FFFFFFF


def reset_rng(seed: int | None = None) -> None:
    """Restart the dropout stream: device seeds re-derived from ``seed`` (default: torch's
    initial seed) and the per-call salt counter rewound -- two runs from the same seed
    draw identical masks (determinism tests, resume)."""
    global _salt
    _seeds.clear()
    _salt = itertools.count(1)
    if seed is not None:
        torch.manual_seed(seed)


def dropout(x, p, salt=None):
    return DropoutFn.apply(x, float(p), new_salt() if salt is None else int(salt))


# ============================================================== losses
LOSS = {"mse_const": 0, "bce_logits_const": 1, "bce_const": 2, "l1": 3, "mse": 4, "l1_glrelu": 6,
        "l1_grelu": 7}


def _dense(x):
    if x.dim() == 4 and x.is_contiguous(memory_format=CL):
        return x
    return x.contiguous()


class LossConstFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, kind, target):
        a = _dense(pred)
        ctx.kind, ctx.target = kind, target
        ctx.save_for_backward(a)
        return P().loss_fwd(a, None, kind, target, 1.0 / a.numel())

    @staticmethod
    def backward(ctx, gout):
        (a,) = ctx.saved_tensors
        ga, _ = P().loss_bwd(a, None, ctx.kind, ctx.target, 1.0 / a.numel(),
                             gout.float().reshape(1), True, False)
        return ga, None, None


class LossPairFn(torch.autograd.Function):
    """``defer``: a's gradient is parked in ``_DEFERRED`` for the conv that also reads ``a``
    (``skip_grad="take"``): its dgrad epilogue adds it, so no autograd accumulate pass runs
    (the VGG loss taps, models/vgg.py).  Only when ``a`` is used as is (NHWC bf16)."""

    @staticmethod
    def forward(ctx, a, b, kind, defer=False):
        if a.dtype != b.dtype:
            b = b.to(a.dtype)
        a0 = a
        a = _dense(a)
        if b.stride() != a.stride():
            b = b.contiguous(memory_format=CL) if a.dim() == 4 and a.is_contiguous(
                memory_format=CL) else b.contiguous()
        ctx.kind = kind
        ctx.defer = bool(defer) and a is a0 and a.dtype == torch.bfloat16 and a.dim() == 4
        ctx.save_for_backward(a, b)
        return P().loss_fwd(a, b, kind, 0.0, 1.0 / a.numel())

    @staticmethod
    def backward(ctx, gout):
        a, b = ctx.saved_tensors
        na, nb = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        ga, gb = P().loss_bwd(a, b, ctx.kind, 0.0, 1.0 / a.numel(), gout.float().reshape(1),
                              na, nb)
        if na and ctx.defer and a.data_ptr() not in _DEFERRED:
            _DEFERRED[a.data_ptr()] = ga
            ga = None
            na = False
        return (ga if na else None), (gb if nb else None), None, None


def mse_const(pred, target):
    return LossConstFn.apply(pred, LOSS["mse_const"], float(target))


def bce_logits_const(pred, target):
    return LossConstFn.apply(pred, LOSS["bce_logits_const"], float(target))


def bce_const(prob, target):
    return LossConstFn.apply(prob, LOSS["bce_const"], float(target))


def l1(a, b, gate_a=None, defer=False):
    """mean |a - b|; ``gate_a="lrelu"`` / ``"relu"``: the gradient of a also carries that
    activation's derivative -- a is its output and the producer conv left the derivative to
    its consumers (out_gated).  ``defer``: see LossPairFn."""
    kinds = {None: "l1", "lrelu": "l1_glrelu", "relu": "l1_grelu"}
    if gate_a not in kinds:
        raise ValueError(f"l1: unsupported gate {gate_a!r}")
    return LossPairFn.apply(a, b, LOSS[kinds[gate_a]], defer)


def mse(a, b):
    return LossPairFn.apply(a, b, LOSS["mse"])


# ============================================================== optimizer
def adam_(params, grads, exp_avg, exp_avg_sq, lr_t, step_t, b1, b2, eps, wd, skip=None):
    P().adam(params, grads, exp_avg, exp_avg_sq, lr_t, step_t, float(b1), float(b2), float(eps),
             float(wd), skip)


# ============================================================== family-R fringe ops
# csrc/misc.hip: shared-slope PReLU, TV loss, quantiser, multiscale-D avg-pool, VGG
# max-pool, channel L2 normalisation, pixel (un)shuffle -- all NHWC bf16.
def _nhwc(x):
    return to_nhwc_bf16(x)


class PReLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w):
        x = _nhwc(x)
        wf = w.detach().float().reshape(1).contiguous()
        ctx.wshape = w.shape
        ctx.save_for_backward(x, wf)
        return P().prelu_fwd(x, wf)

    @staticmethod
    def backward(ctx, gy):
        x, wf = ctx.saved_tensors
        outs = P().prelu_bwd(x, _nhwc(gy), wf, bool(ctx.needs_input_grad[0]))
        gx = outs[1] if ctx.needs_input_grad[0] else None
        gw = outs[0].reshape(ctx.wshape) if ctx.needs_input_grad[1] else None
        return gx, gw


def prelu(x, weight):
    if weight.numel() != 1:
        # per-channel PReLU is not used by either model family; explicit stock-PyTorch op
        return torch.nn.functional.prelu(x, weight.to(x.dtype))
    return PReLUFn.apply(x, weight)


class TVFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _nhwc(x)
        ctx.save_for_backward(x)
        return P().tv_fwd(x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return P().tv_bwd(x, g)


def tv(x):
    return TVFn.apply(x)


SSIM_WINDOWS = {"uniform7": 0, "gauss11": 1}


class SSIMLossFn(torch.autograd.Function):
    """1 - mean SSIM (csrc/ssim_loss.hip).  Saves only the two images: the backward kernel
    recomputes the window moments, so no per-origin map lives between the passes.  Inputs
    are read through their strides (NHWC bf16, channel-padded views, NCHW fp32)."""

    @staticmethod
    def forward(ctx, x, y, window, data_range):
        if y.dtype != x.dtype:
            y = y.to(x.dtype)
        ctx.window, ctx.data_range = window, data_range
        ctx.save_for_backward(x, y)
        return P().ssim_loss_fwd(x, y, window, data_range)

    @staticmethod
    def backward(ctx, gout):
        x, y = ctx.saved_tensors
        nx, ny = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        gx, gy = P().ssim_loss_bwd(x, y, ctx.window, ctx.data_range, gout.float().reshape(1), nx, ny)
        return (gx if nx else None), (gy if ny else None), None, None


def ssim_loss(x, y, window="uniform7", data_range=2.0):
    if window not in SSIM_WINDOWS:
        raise ValueError(f"ssim_loss: unknown window {window!r} (uniform7 | gauss11)")
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"ssim_loss: fp32 or bf16 images, got {x.dtype}")   # no silent upcast
    return SSIMLossFn.apply(x, y, SSIM_WINDOWS[window], float(data_range))


class MSSSIMLossFn(torch.autograd.Function):
    """1 - mean MS-SSIM (csrc/ms_ssim_loss.hip).  Saves the two images, the fp32 pyramid of
    their pooled scales (2 x 1/3 of the pixels) and the [M, N, C] backward coefficients; the
    backward kernels recompute the window moments, so no per-origin map is kept.  Also
    returns the per-(n, c) values (not differentiable)."""

    @staticmethod
    def forward(ctx, x, y, window, data_range, weights):
        if y.dtype != x.dtype:
            y = y.to(x.dtype)
        loss, ms, pyr, coef = P().ms_ssim_loss_fwd(x, y, window, data_range, weights)
        ctx.window, ctx.data_range = window, data_range
        ctx.save_for_backward(x, y, pyr, coef)
        ctx.mark_non_differentiable(ms)
        return loss, ms

    @staticmethod
    def backward(ctx, gout, _gms):
        x, y, pyr, coef = ctx.saved_tensors
        nx, ny = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        gx, gy = P().ms_ssim_loss_bwd(x, y, pyr, coef, ctx.window, ctx.data_range, gout.float().reshape(1),
                                      nx, ny)
        return (gx if nx else None), (gy if ny else None), None, None, None


def _ms_ssim(x, y, window, data_range, weights):
    from . import reference as ref
    if window not in SSIM_WINDOWS:
        raise ValueError(f"ms_ssim_loss: unknown window {window!r} (uniform7 | gauss11)")
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"ms_ssim_loss: fp32 or bf16 images, got {x.dtype}")   # no silent upcast
    ref.ms_ssim_check(x.shape, window, len(weights))
    return MSSSIMLossFn.apply(x, y, SSIM_WINDOWS[window], float(data_range), [float(w) for w in weights])


def ms_ssim_loss(x, y, window="gauss11", data_range=2.0, weights=None):
    from . import reference as ref
    return _ms_ssim(x, y, window, data_range, ref.MS_SSIM_WEIGHTS if weights is None else weights)[0]


def ms_ssim(x, y, window="gauss11", data_range=2.0, weights=None):
    from . import reference as ref
    with torch.no_grad():
        return _ms_ssim(x, y, window, data_range, ref.MS_SSIM_WEIGHTS if weights is None else weights)[1]


class FFLLossFn(torch.autograd.Function):
    """Focal frequency loss (csrc/ffl_loss.hip).  Saves only the half spectrum F (fp32,
    [N, C, 2, H, W / 2 + 1], about 4 bytes per pixel) and the per-plane scales inv [N, C]:
    neither image.  The gradients take the layout ``empty_like`` would give each image."""

    @staticmethod
    def forward(ctx, x, y, alpha):
        if y.dtype != x.dtype:
            y = y.to(x.dtype)
        loss, f, inv = P().ffl_loss_fwd(x, y, alpha)
        like = torch.empty_like(torch.empty_strided(x.shape, x.stride(), dtype=x.dtype, device="meta"))
        ctx.alpha, ctx.strides, ctx.bf16 = alpha, list(like.stride()), x.dtype == torch.bfloat16
        ctx.save_for_backward(f, inv)
        return loss

    @staticmethod
    def backward(ctx, gout):
        f, inv = ctx.saved_tensors
        nx, ny = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        gx, gy = P().ffl_loss_bwd(f, inv, gout.float().reshape(1), ctx.strides, int(ctx.bf16), ctx.alpha, ny)
        return (gx if nx else None), (gy if ny else None), None


def ffl_loss(x, y, alpha=1.0):
    from . import reference as ref
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"ffl_loss: fp32 or bf16 images, got {x.dtype}")   # no silent upcast
    ref.ffl_check(x.shape)
    return FFLLossFn.apply(x, y, float(alpha))


class LapLossFn(torch.autograd.Function):
    """Laplacian-pyramid L1 loss (csrc/lap_loss.hip).  Saves only the int8 sign pyramid (4/3
    byte per pixel): neither image.  The gradients take the layout ``empty_like`` would give
    each image; y's is the exact negative of x's, written by the same launch."""

    @staticmethod
    def forward(ctx, x, y, levels):
        if y.dtype != x.dtype:
            y = y.to(x.dtype)
        loss, signs = P().lap_loss_fwd(x, y, levels)
        like = torch.empty_like(torch.empty_strided(x.shape, x.stride(), dtype=x.dtype, device="meta"))
        ctx.levels, ctx.sizes, ctx.strides = levels, list(x.shape), list(like.stride())
        ctx.bf16 = x.dtype == torch.bfloat16
        ctx.save_for_backward(signs)
        return loss

    @staticmethod
    def backward(ctx, gout):
        (signs,) = ctx.saved_tensors
        nx, ny = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        gx, gy = P().lap_loss_bwd(signs, gout.float().reshape(1), ctx.sizes, ctx.strides, int(ctx.bf16),
                                  ctx.levels, ny)
        return (gx if nx else None), (gy if ny else None), None


def lap_loss(x, y, levels=5):
    from . import reference as ref
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"lap_loss: fp32 or bf16 images, got {x.dtype}")   # no silent upcast
    ref.lap_check(x.shape, int(levels))
    return LapLossFn.apply(x, y, int(levels))


class GramLossFn(torch.autograd.Function):
    """Gram-matrix style loss (csrc/gram_loss.hip).  Saves fx and the bf16 image of
    D = G(fx) - G(fy) ([B, C, C]); the gradient has the dtype and strides of fx."""

    @staticmethod
    def forward(ctx, fx, fy):
        loss, _, dh = P().gram_loss_fwd(fx, fy)
        ctx.save_for_backward(fx, dh)
        return loss

    @staticmethod
    def backward(ctx, gout):
        fx, dh = ctx.saved_tensors
        return P().gram_loss_bwd(fx, dh, gout.float().reshape(1)), None


def gram_loss(fx, fy):
    from . import reference as ref
    if fy.requires_grad:
        raise ValueError("gram_loss: fy is a constant target; detach it")
    for name, f in (("fx", fx), ("fy", fy)):   # no silent upcast, no silent re-layout
        if f.dtype != torch.bfloat16 or f.dim() != 4 or not f.is_contiguous(memory_format=torch.channels_last):
            raise TypeError(f"gram_loss: {name} must be bf16 channels_last [B, C, H, W] features, got {f.dtype} "
                            f"with strides {tuple(f.stride())}")
    ref.gram_check(fx.shape)
    if fx.shape != fy.shape:
        raise ValueError(f"gram_loss: shapes differ, {tuple(fx.shape)} and {tuple(fy.shape)}")
    return GramLossFn.apply(fx, fy)


AUGMENT_DTYPES = {torch.float32: 0, torch.bfloat16: 1}


def augment_pairs(a_u8, b_u8, params, load, crop, dtype=torch.bfloat16, antialias=False):
    """csrc/augment.hip: one launch from the uint8 cache to the two model-range batches."""
    if dtype not in AUGMENT_DTYPES:
        raise TypeError(f"augment_pairs: bf16 or fp32 output, got {dtype}")
    a, b = P().augment_pairs(a_u8, b_u8, params, int(load[0]), int(load[1]), int(crop[0]), int(crop[1]),
                             AUGMENT_DTYPES[dtype], bool(antialias))
    return a, b


# y -> its unshuffled, channel-padded copy written by the same quantise pass (the expander's
# head input); entries hold y, so a key never aliases a recycled allocation
_unshuffled: dict = {}


def quantize(x, bits, unshuffle=0):
    """Forward value only: round() has zero gradient (the reference's quantiser).
    ``unshuffle`` r: also write the pixel-unshuffled copy, channel-padded to 8 and tagged as a
    packed conv input, for ``pixel_unshuffle(y, r, conv_input=True)``."""
    x = _nhwc(x.detach())
    r = int(unshuffle)
    if r <= 1 or x.shape[2] % r or x.shape[3] % r:
        return P().quantize(x, int(bits))
    cu = x.shape[1] * r * r
    y, yu = P().quantize_unshuffle(x, int(bits), r, _pad8(cu))
    yu._p2p_packed = (cu, 0)
    if len(_unshuffled) >= 16:
        _unshuffled.pop(next(iter(_unshuffled)))
    _unshuffled[(y.data_ptr(), tuple(y.shape), r)] = (y, yu, y._version)
    return y


class AvgPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _nhwc(x)
        ctx.hw = (x.shape[2], x.shape[3])
        return P().avgpool3s2(x, 0, 0, 0)

    @staticmethod
    def backward(ctx, gy):
        return P().avgpool3s2(_nhwc(gy), 1, ctx.hw[0], ctx.hw[1])


def avg_pool3_s2(x):
    return AvgPoolFn.apply(x)


class MaxPool2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _nhwc(x)
        ctx.save_for_backward(x)
        return P().maxpool2(x, None)

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        return P().maxpool2(x, _nhwc(gy))


def max_pool2(x):
    return MaxPool2Fn.apply(x)


class L2NormFn(torch.autograd.Function):
    """y = x / ||x||_C (+ res): the residual add rides in the same pass.  ``shuffle`` r > 1:
    x is the pre-PixelShuffle(r) tensor and y the normalised shuffled one -- the shuffle is
    the kernel's addressing (and the un-shuffle of the gradient the backward's), no pass."""

    @staticmethod
    def forward(ctx, x, eps, res, shuffle=1):
        x = _nhwc(x)
        ctx.eps, ctx.has_res, ctx.r = eps, res is not None, shuffle
        ctx.save_for_backward(x)
        return P().l2norm(x, None, eps, _nhwc(res) if res is not None else None, shuffle)

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        gy = _nhwc(gy)
        return P().l2norm(x, gy, ctx.eps, None, ctx.r), None, (gy if ctx.has_res else None), None


def l2_normalize_channels(x, eps=1e-12, residual=None, shuffle=1):
    return L2NormFn.apply(x, float(eps), residual, int(shuffle))


class PixelShuffleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, r, direction):
        ctx.r, ctx.dir = r, direction
        return P().pixel_shuffle(_nhwc(x), r, direction)

    @staticmethod
    def backward(ctx, gy):
        return P().pixel_shuffle(_nhwc(gy), ctx.r, 1 - ctx.dir), None, None


def pixel_shuffle(x, r):
    return PixelShuffleFn.apply(x, int(r), 1)


def pixel_unshuffle(x, r, conv_input=False):
    if conv_input and not x.requires_grad:
        # y itself or a view of it (``compressed.detach()``): the entry holds y, so a matching
        # address is y's storage, and the shared version counter says it is unmodified
        ent = _unshuffled.get((x.data_ptr(), tuple(x.shape), int(r)))
        if ent is not None and x._version == ent[2] and x.stride() == ent[0].stride():
            return ent[1]
    return PixelShuffleFn.apply(x, int(r), 0)
