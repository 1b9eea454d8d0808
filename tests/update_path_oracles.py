"""Float64 oracles and derived error bounds of the fp32 update path (shared by
test_update_path_cpu.py and test_update_path_gpu.py; a plain module, not a conftest).

Every oracle is the kernel's formula as written in the .hip file, evaluated in ``dtype``
(float64 = the oracle, float32 = the same formula at the kernel's precision) on the exact values
the kernel sees: bf16 inputs rounded to bf16 first, hyperparameters rounded to fp32 first (the
binding casts them to ``float``; the kernel forms ``1 - b`` from the rounded value).

Bound of a case: max(10 x E, floor).  E = |oracle(float32) - oracle(float64)| on the case's own
inputs; floor = (number of roundings in the longest chain an output passes through in the kernel
source) x u x (sum of the magnitudes of the terms), u = 2^-24.  Two errors E does not model
get their own floor term: ``powf`` in Adam's bias correction (K_POW ulp) and ``__expf`` in loss
kind 1 (EXPF_ABS / EXPF_REL); their values and sources are in profiles/update_path_tests.md.
"""
import functools
import math

import numpy as np
import torch

U = 2.0 ** -24           # fp32 unit round-off
BF16 = 2.0 ** -9         # one bf16 rounding, relative
K_POW = 2                # ulp bound assumed for powf (no HIP accuracy table on the build machine)
# __expf alone, measured on an MI355X against float64 (4 x the measured maxima, see the profile):
EXPF_ABS = 4 * 5.11e-8   # |__expf(x) - exp(x)| over x in [-100, 0]   (feeds log1pf in kind 1)
EXPF_REL = 4 * 9.86e-7   # relative, over x in [-20, 20]              (feeds the sigmoid of kind 1)
EXPF_REL_FAR = 4 * 3.87e-6   # relative, over 20 < |x| <= 100 where the result is finite and normal
LRELU_SLOPE = 0.2
F32, F64 = torch.float32, torch.float64


def r32(x):
    """A python float rounded to fp32 (what ``(float)x`` in the binding gives the kernel)."""
    return float(np.float32(x))


def ulp32(x):
    """fp32 ulp of |x| elementwise (float64 tensor; 0 where x == 0)."""
    x = x.double().abs()
    _, e = torch.frexp(x)
    return torch.where(x == 0, torch.zeros_like(x), torch.ldexp(torch.ones_like(x), e - 24))


def tol_of(o32, o64, floor):
    """max(10 E, floor) elementwise, E from the two oracle evaluations."""
    return torch.maximum(10 * (o32.double() - o64).abs(), floor.double() if torch.is_tensor(floor)
                         else torch.full_like(o64, float(floor)))


# ------------------------------------------------------------------------------------- Adam
def adam_grad(n, seed):
    """Gradient of n elements: magnitudes 10^U(-8, 0), random signs, ~6 % exact zeros."""
    g = torch.Generator().manual_seed(seed)
    mag = torch.pow(10.0, -8 * torch.rand(n, generator=g, dtype=F64))
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    keep = (torch.rand(n, generator=g) >= 0.06).double()
    return (mag * sign * keep).float()


def adam_params(sizes, init, seed):
    """init: 'unit' (randn), 'milli' (1e-3 * randn) or 'zero'."""
    g = torch.Generator().manual_seed(seed)
    scale = {"unit": 1.0, "milli": 1e-3, "zero": 0.0}[init]
    return [(torch.randn(n, generator=g) * scale).float() for n in sizes]


class AdamOracle:
    """csrc/optim.hip adam_kernel, one state per parameter group, in ``dtype``.

    The float64 instance also carries the floors of p, exp_avg and exp_avg_sq, accumulated over
    steps (u = 2^-24, |g| + |wd p| =: A, the terms of gj):
      exp_avg     += u (4 |b1 m| + 6 (1 - b1) A) + (1 - b1) wd floor_p   (1 - b1, two products, the sum; gj: 2 more)
      exp_avg_sq  += u (4 |b2 v| + 8 (1 - b2) A^2) + 2 (1 - b2) A wd floor_p   (gj^2 doubles gj's error,
                     three products, the sum)
      den          : sqrt (half of v's relative error, 1 rounding), x rbc2 (rsqrtf + 1 - pow + the
                     product: 3 u, and half of powf's K_POW u b2^t / (1 - b2^t)), + eps (1 rounding)
      p           += |upd| (4 u + K_POW u b1^t / (1 - b1^t)) + step_size floor_m / den
                     + |upd| floor_den / den + ulp(|p|)    (lr / bc1, x m, / den; the store of p)
    """

    def __init__(self, groups, params, dtype):
        self.dt = dtype
        self.g = []
        for spec, ps in zip(groups, params):
            z = lambda: [torch.zeros(p.numel(), dtype=dtype) for p in ps]   # noqa: E731
            f = lambda: [torch.zeros(p.numel(), dtype=F64) for p in ps]    # noqa: E731
            self.g.append(dict(lr=spec.get("lr", 2e-4), betas=spec.get("betas", (0.5, 0.999)),
                               eps=spec.get("eps", 1e-8), wd=spec.get("wd", 0.0), t=0.0,
                               p=[p.detach().reshape(-1).to(dtype).clone() for p in ps], m=z(), v=z(),
                               fp=f(), fm=f(), fv=f()))

    def c(self, x):
        return torch.tensor(r32(x), dtype=self.dt)

    def step(self, grads, skip=False):
        if skip:   # the kernel returns before any load; the device counter adds 1 - skip = 0
            return
        for G, gr in zip(self.g, grads):
            G["t"] += 1.0
            lr, b1, b2, eps, wd, t = (self.c(x) for x in (G["lr"], *G["betas"], G["eps"], G["wd"], G["t"]))
            p1, p2 = torch.pow(b1, t), torch.pow(b2, t)
            bc1, bc2 = 1 - p1, 1 - p2
            ss, rbc2 = lr / bc1, 1 / torch.sqrt(bc2)
            pw1, pw2 = (K_POW * U * float(q) / float(1 - q) for q in (p1.double(), p2.double()))
            for i, g in enumerate(gr):
                p, m, v = G["p"][i], G["m"][i], G["v"][i]
                g = g.reshape(-1).to(self.dt)
                gj = g + wd * p
                m1 = b1 * m + (1 - b1) * gj
                v1 = b2 * v + (1 - b2) * gj * gj
                sq = torch.sqrt(v1)
                den = sq * rbc2 + eps
                upd = ss * m1 / den
                p1_ = p - upd
                if self.dt == F64:
                    A = g.abs() + (wd * p).abs()
                    dgj = float(wd) * G["fp"][i]
                    fm = G["fm"][i] + U * (4 * (b1 * m).abs() + 6 * (1 - b1) * A) + (1 - b1) * dgj
                    fv = G["fv"][i] + U * (4 * (b2 * v).abs() + 8 * (1 - b2) * A * A) + 2 * (1 - b2) * A * dgj
                    dsq = torch.where(sq > 0, fv / (2 * sq.clamp_min(1e-300)), torch.zeros_like(sq)) + U * sq
                    dden = dsq * rbc2 + sq * rbc2 * (3 * U + 0.5 * pw2) + U * den
                    dupd = upd.abs() * (4 * U + pw1) + ss * fm / den + upd.abs() * dden / den
                    G["fp"][i] = G["fp"][i] + dupd + torch.maximum(ulp32(p), ulp32(p1_))
                    G["fm"][i], G["fv"][i] = fm, fv
                G["p"][i], G["m"][i], G["v"][i] = p1_, m1, v1


def adam_tols(o32, o64):
    """[(group, index, name, oracle64, tol)] for p, exp_avg, exp_avg_sq of every tensor."""
    out = []
    for gi, (a, b) in enumerate(zip(o32.g, o64.g)):
        for i in range(len(b["p"])):
            for name, fl in (("p", "fp"), ("m", "fm"), ("v", "fv")):
                out.append((gi, i, name, b[name][i], tol_of(a[name][i], b[name][i], b[fl][i])))
    return out


# ------------------------------------------------------------------- spectral-norm gradient
def sn_inputs(h, wd, correlated, seed):
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(h, wd, generator=g)
    G = torch.randn(h, wd, generator=g) + (3 * W if correlated else 0)   # correlated: the sigma path dominates
    u = torch.nn.functional.normalize(torch.randn(h, generator=g), dim=0)
    v = torch.nn.functional.normalize(torch.randn(wd, generator=g), dim=0)
    return W.float(), G.float(), u.float(), v.float()


def sn_power_iter(W, u, dtype):
    """One iteration of csrc/sn.hip: v = l2n(W^T u), u = l2n(W v), sigma = u . (W v); -> 1 / sigma."""
    W, u = W.to(dtype), u.to(dtype)
    eps = torch.tensor(r32(1e-12), dtype=dtype)
    t = W.t() @ u
    v = t / (t.norm() + eps)
    s = W @ v
    u = s / (s.norm() + eps)
    return 1 / (u @ s), u, v


def sn_scale_floor(W, u0):
    """Relative floor of 1 / sigma.  sigma = ||W v|| up to the eps, v = l2n(W^T u): chains of
    h / 8 + 8 additions (sn_wtu + sn_tsum), wd / 64 + 6 (one wave per row in sn_wv), h / 256 + 10
    (sn_finish) and ~10 roundings of norms, quotients and the reciprocal; each dot's error is
    bounded by u x sum |terms|, so relative to sigma the count is multiplied by
    kappa = (|u|^T |W| |v|) / sigma >= 1 of the final u, v."""
    h, wd = W.shape
    s, u, v = sn_power_iter(W, u0, F64)
    kappa = float(u.abs() @ (W.double().abs() @ v.abs())) * float(s)
    return (h / 8 + 8 + wd / 64 + 6 + h / 256 + 10 + 10) * U * max(kappa, 1.0)


def sn_wgrad(G, W, u, v, scale, dtype, acc=None):
    """sn_dot_kernel + sn_grad_kernel: sc G - (<G, W> sc sc) u v^T (+ acc)."""
    G, W, u, v, sc = (x.to(dtype) for x in (G, W, u, v, scale.reshape(())))
    k = (G * W).sum() * sc * sc
    out = sc * G - (k * u)[:, None] * v[None, :]
    return out if acc is None else acc.to(dtype) + out


def sn_wgrad_blocks(n):
    return max(1, min(256, (n + 4095) // 4096))


def sn_wgrad_floor(G, W, u, v, scale, acc=None):
    """The dot: ceil(n / (256 nb)) additions per thread (+ 1 product), 6 in the wave tree, 4 in
    the LDS combine, nb in the serial loop of sn_grad_kernel -> count x u x sum |G W|, scaled by
    sc^2 |u_r v_c|; then 5 roundings on |sc G| + |k u v| and 1 on the accumulate."""
    G, W, u, v, sc = (x.double() for x in (G, W, u, v, scale.reshape(())))
    n, nb = G.numel(), sn_wgrad_blocks(G.numel())
    count = math.ceil(n / (256 * nb)) + 1 + 6 + 4 + nb
    dot_err = count * U * (G * W).abs().sum()
    uv = u.abs()[:, None] * v.abs()[None, :]
    k = ((G * W).sum() * sc * sc).abs()
    fl = sc * sc * uv * dot_err + 5 * U * ((sc * G).abs() + k * uv)
    if acc is not None:
        fl = fl + U * (acc.double().abs() + (sc * G).abs() + k * uv)
    return fl


# ------------------------------------------------------------------------------- column sums
def colsum_input(M_shape, C, seed):
    """bf16 NHWC activations as an [N, C, H, W] channels_last tensor."""
    N, H, W = M_shape
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, H, W, C, generator=g).to(torch.bfloat16).permute(0, 3, 1, 2)


def colsum(x, cout, scale, dtype, before=None):
    """scale x sum over pixels of the bf16 values, leading ``cout`` channels (+ before)."""
    C = x.shape[1]
    s = x.permute(0, 2, 3, 1).reshape(-1, C).to(dtype).sum(0)[:cout] * torch.tensor(r32(scale), dtype=dtype)
    return s if before is None else before.to(dtype) + s


def colsum_blocks(M):
    return max(1, min(1024, (M + 511) // 512))


def colsum_floor(x, cout, scale, before=None):
    """colsum_partial_kernel: ceil(rpb / RP) additions per thread (RP = 256 / (C / 8) rows in
    flight), RP in the LDS combine; colsum_final_kernel: ceil(nb / 32) per thread, 32 in its
    combine, the product with scale, the accumulate: count x u x |scale| sum |x| per channel."""
    C = x.shape[1]
    M = x.numel() // C
    nb = colsum_blocks(M)
    rpb = -(-M // nb)
    RP = 256 // (C // 8)
    count = -(-rpb // RP) + RP + -(-nb // 32) + 32 + 2
    mag = x.permute(0, 2, 3, 1).reshape(-1, C).double().abs().sum(0)[:cout] * abs(r32(scale))
    return count * U * (mag if before is None else mag + before.double().abs())


# ------------------------------------------------------------------------------------ losses
PAIR_KINDS = (3, 4, 6, 7)


def loss_inputs(kind, n, dtype, seed):
    """(a, b or None) as CPU tensors of ``dtype`` with the planted edge elements (as many as fit):
    pair kinds: a[0] == b[0]; kinds 6 / 7 also a[1] == 0; kind 2: a[0] = 0, a[1] = 1 exactly;
    kind 1: logits 80, -80, 100, -100."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(n, generator=g)
    b = torch.randn(n, generator=g) if kind in PAIR_KINDS else None
    plant = []
    if kind == 1:
        a, plant = a * 3, [80.0, -80.0, 100.0, -100.0]
    elif kind == 2:
        a, plant = torch.rand(n, generator=g) * 0.98 + 0.01, [0.0, 1.0]
    elif kind in (6, 7):
        plant = [None, 0.0]
    for i, val in enumerate(plant[:n]):
        if val is not None:
            a[i] = val
    a = a.to(dtype)
    if b is not None:
        b = b.to(dtype)
        b[0] = a[0]
    return a, b


def _loss_elem(kind, a, b, t):
    dt = a.dtype
    c = lambda x: torch.tensor(r32(x), dtype=dt)   # noqa: E731
    if kind == 0:
        return (a - t) ** 2
    if kind == 1:
        return a.clamp_min(0) - a * t + torch.log1p(torch.exp(-a.abs()))
    if kind == 2:
        lp, lq = torch.log(a).clamp_min(c(-100.0)), torch.log(1 - a).clamp_min(c(-100.0))
        return -(t * lp + (1 - t) * lq)
    if kind in (3, 6, 7):
        return (a - b).abs()
    if kind == 4:
        return (a - b) ** 2
    return a


def _loss_grad(kind, a, b, t):
    dt = a.dtype
    c = lambda x: torch.tensor(r32(x), dtype=dt)   # noqa: E731
    if kind == 0:
        return 2 * (a - t)
    if kind == 1:
        return 1 / (1 + torch.exp(-a)) - t
    if kind == 2:
        return (a - t) / (a * (1 - a)).clamp_min(c(1e-12))
    if kind == 3:
        return torch.sign(a - b)
    if kind == 6:
        return torch.sign(a - b) * torch.where(a > 0, c(1.0), c(LRELU_SLOPE))
    if kind == 7:
        return torch.where(a > 0, torch.sign(a - b), torch.zeros_like(a))
    if kind == 4:
        return 2 * (a - b)
    return torch.ones_like(a)


def loss_blocks(n):
    return max(1, min(1024, (n + 2047) // 2048))


def loss_fwd(kind, a, b, t, scale, dtype):
    """(value, floor): scale x sum of loss_elem.  Floor: every term carries <= 8 roundings of its
    own; the sum adds ceil(n / (256 nb)) per thread, 6 (wave tree) + 3 (LDS) in the partial
    kernel, ceil(nb / 256) + 6 + 3 in loss_final_kernel and the product with scale -> count x u x
    |scale| sum |terms| (for kinds 1 / 2 the magnitudes of the summands of each term); kind 1
    adds EXPF_ABS per element (d log1p(e) <= d e)."""
    A = a.to(dtype)
    B = None if b is None else b.to(dtype)
    T = torch.tensor(r32(t), dtype=dtype)
    S = torch.tensor(r32(scale), dtype=dtype)
    val = _loss_elem(kind, A, B, T).sum() * S
    A6 = a.double()
    if kind == 1:
        mag = A6.clamp_min(0) + (A6 * r32(t)).abs() + torch.log1p(torch.exp(-A6.abs()))
    elif kind == 2:
        e = _loss_elem(2, A6, None, torch.tensor(1.0, dtype=F64)).abs() + _loss_elem(
            2, A6, None, torch.tensor(0.0, dtype=F64)).abs()
        mag = e   # t |lp| + (1 - t) |lq| <= |lp| + |lq|
    elif kind == 0:
        mag = (A6.abs() + abs(r32(t))) ** 2
    elif kind == 4:
        mag = (A6.abs() + b.double().abs()) ** 2
    elif kind == 5:
        mag = A6.abs()
    else:
        mag = A6.abs() + b.double().abs()
    n, nb = a.numel(), loss_blocks(a.numel())
    count = 8 + math.ceil(n / (256 * nb)) + 9 + math.ceil(nb / 256) + 9 + 1
    floor = count * U * abs(r32(scale)) * float(mag.sum())
    if kind == 1:
        floor += EXPF_ABS * n * abs(r32(scale))
    return val, floor


def loss_bwd(kind, a, b, t, scale, gout, dtype):
    """(ga, floor) elementwise: (gout x scale) x loss_grad; gb = -ga exactly.  <= 8 roundings on
    the magnitudes of the terms (gout x scale, the differences, product, quotient); kind 1:
    sigmoid s = 1 / (1 + e), d s = s (1 - s) rel(e) with rel(e) <= EXPF_REL inside |a| <= 20 and
    <= EXPF_REL_FAR beyond, where s (1 - s) <= e^-20; a bf16 result adds one bf16 rounding
    (2^-9 relative in the floor; the float32 evaluation rounds its result to bf16 too)."""
    A = a.to(dtype)
    B = None if b is None else b.to(dtype)
    T = torch.tensor(r32(t), dtype=dtype)
    g = torch.tensor(r32(gout), dtype=dtype) * torch.tensor(r32(scale), dtype=dtype)
    val = g * _loss_grad(kind, A, B, T)
    A6, g6 = a.double(), abs(r32(gout) * r32(scale))
    if kind == 0:
        mag = 2 * (A6.abs() + abs(r32(t)))
    elif kind == 4:
        mag = 2 * (A6.abs() + b.double().abs())
    elif kind == 1:
        mag = torch.sigmoid(A6) + abs(r32(t))
    else:
        mag = _loss_grad(kind, A6, None if b is None else b.double(), torch.tensor(r32(t), dtype=F64)).abs()
    floor = 8 * U * g6 * mag
    if kind == 1:
        s = torch.sigmoid(A6)
        floor = floor + g6 * s * (1 - s) * torch.where(A6.abs() <= 20, EXPF_REL, EXPF_REL_FAR)
    if a.dtype == torch.bfloat16:
        floor = floor + BF16 * val.double().abs()
        if dtype == F32:   # the kernel-precision evaluation stores its result as the kernel does, so
            val = val.to(torch.bfloat16).float()   # E carries the rounding's worst case, 2^-8 relative
    return val, floor


# -------------------------------------------------------------------------- scalar composition
def lincomb_n(vals, ws, dtype):
    """lincomb_n_kernel: s += w_i * t_i in order, chained 15 terms at a time by the wrapper
    (the running total re-enters with weight 1: the same serial sum)."""
    s = torch.zeros((), dtype=dtype)
    for x, w in zip(vals, ws):
        s = s + torch.tensor(r32(w), dtype=dtype) * torch.tensor(r32(x), dtype=dtype)
    return s


def lincomb_terms(n):
    """n loss values ~ U(0, 2) and weights ~ N(0, 1) with a 0 at index 1 and a negative one at 2."""
    g = torch.Generator().manual_seed(n)
    vals = (torch.rand(n, generator=g) * 2).float().tolist()
    ws = torch.randn(n, generator=g).tolist()
    if n > 2:
        ws[1], ws[2] = 0.0, -abs(ws[2]) - 0.25
    return vals, ws


def lincomb_n_floor(vals, ws):
    """n products and n additions in one serial chain: 2 n u sum |w_i t_i|."""
    return 2 * len(vals) * U * sum(abs(r32(w) * r32(x)) for x, w in zip(vals, ws))


# ------------------------------------------------------------------------------- case tables

INITS = ("unit", "milli", "zero")
# 1 - 4 chunks of 4096, both the n & 3 path and the float4 path; multi-chunk tensors mid-list
ADAM_SIZES = [1, 3, 4, 8192, 7, 8, 4092, 12289, 4095, 4096, 4097, 4100]
# 100 tensors > 2 x MT_MAX = 40: tensors 40 and 41 (indices 39, 40) are n = 2 (scalar path) and
# n = 4 (float4 path), likewise 80 and 81
ADAM_MANY = [(4, 5, 8, 3, 12, 1, 16, 7, 20, 2)[i % 10] for i in range(100)]
ADAM_CASES = {
    "sizes": dict(groups=[dict(sizes=ADAM_SIZES)], steps=3),
    "many": dict(groups=[dict(sizes=ADAM_MANY)], steps=2),
    "wd_groups": dict(groups=[dict(sizes=[7, 4096, 5], wd=1e-2),
                              dict(sizes=[4100, 3], lr=1e-3, betas=(0.9, 0.99), wd=1e-2)], steps=3),
    "step999": dict(groups=[dict(sizes=[7, 4096])], steps=2, step0=999.0),
    "step19999": dict(groups=[dict(sizes=[7, 4096])], steps=2, step0=19999.0),
    "lr_change": dict(groups=[dict(sizes=[5, 4096]), dict(sizes=[8], lr=1e-3)], steps=3,
                      lrs={1: (1e-4, 5e-4), 2: (3e-4, 5e-4)}),
    "skip": dict(groups=[dict(sizes=[7, 4096, 4097])], steps=4, skips={1: 1.0, 2: 0.0, 3: 1.0}),
    "guarded": dict(groups=[dict(sizes=[7, 4096])], steps=1),
    # GradReducer._add_bucket's layout (off += n): in this order the float4-path tensors 64 and
    # 4096 start at float offsets 1 and 65 of the flat buffer, 4 and 4 bytes off a 16-byte boundary
    "bucket": dict(groups=[dict(sizes=[1, 64, 4096, 3])], steps=2),
    # the replay order of the captured step: lr 2e-4; lr 1e-4 + sync_lr; flag 1; flag 0
    "graph": dict(groups=[dict(sizes=[7, 4096, 4097, 64])], steps=4, lrs={1: (1e-4,)},
                  skips={0: 0.0, 1: 0.0, 2: 1.0, 3: 0.0}),
}


def adam_case_grads(name, k):
    return [[adam_grad(n, 7919 * (k + 1) + 131 * gi + i) for i, n in enumerate(g["sizes"])]
            for gi, g in enumerate(ADAM_CASES[name]["groups"])]


def adam_case_params(name, init):
    return [adam_params(g["sizes"], init, 100 + gi) for gi, g in enumerate(ADAM_CASES[name]["groups"])]


@functools.lru_cache(maxsize=None)
def adam_trajectory(name, init):
    """Per step: [(group, index, 'p' | 'm' | 'v', oracle64, tol, oracle32)] after that step."""
    case = ADAM_CASES[name]
    params = adam_case_params(name, init)
    o32, o64 = AdamOracle(case["groups"], params, F32), AdamOracle(case["groups"], params, F64)
    for o in (o32, o64):
        for G in o.g:
            G["t"] = case.get("step0", 0.0)
    traj = []
    for k in range(case["steps"]):
        grads = adam_case_grads(name, k)
        for o in (o32, o64):
            for G, lr in zip(o.g, case.get("lrs", {}).get(k, ())):
                G["lr"] = lr
            o.step(grads, skip=case.get("skips", {}).get(k, 0.0) != 0.0)
        traj.append([(gi, i, nm, x.clone(), tol, o32.g[gi][nm][i].clone())
                     for gi, i, nm, x, tol in adam_tols(o32, o64)])
    return traj


SN_SHAPES = [(3, 70), (64, 1024), (512, 8192)]   # the last: 4 M elements, the 256-block cap
COLSUM_C = [8, 24, 136, 1032, 2048]
# M = N H W: 1, 7, 5000, and 1023 / 1025 around 2 x 512 (p2p_colsum_blocks: one block per 512
# rows, rows_per_block = ceil(M / blocks) = 512 at M = 1023 / 1024, 342 at 1025 with a 3rd block)
COLSUM_M = [(1, 1, 1), (1, 7, 1), (2, 50, 50), (1, 33, 31), (1, 41, 25)]
LOSS_N = [1, 5, 8, 189, 2051, 70001]
LOSS_T = [0.0, 1.0, 0.9]
LOSS_DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
