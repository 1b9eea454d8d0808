"""The fp32 update path -- multi-tensor Adam, the NaN/Inf guard, scalar composition, the
spectral-norm weight gradient, the bias-gradient column sums and the loss kernels -- against
float64 oracles of the kernels' own formulas (tests/update_path_oracles.py).

Bound of every case: max(10 x E, floor), elementwise.  E = |oracle in float32 - oracle in
float64| on the case's inputs; the floor counts the roundings of the longest chain in the kernel
source times u = 2^-24 times the magnitudes of the terms (each oracle's docstring derives its
own), plus K_POW = 2 ulp of ``powf`` in Adam's bias correction and the measured ``__expf`` error in
loss kind 1.  tests/test_update_path_cpu.py proves every bound reachable in float32;
profiles/update_path_tests.md records E, the floors and the errors seen on the GPU.
"""
import copy
import json
import os

import numpy as np
import pytest
import torch

import update_path_oracles as O
from p2p_pytorch_amd import _native
from p2p_pytorch_amd import ops
from p2p_pytorch_amd.engine.optim import FusedAdam, guarded_step
from p2p_pytorch_amd.utils.guards import nonfinite

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(autouse=True, scope="module")
def _native_backend():
    _native.set_backend("native")
    assert _native.load(), _native.load_error()
    yield


def _record(tag, **row):
    """Print the measured figures of a case and, with P2P_RECORD_DIR set, append them to
    update_path.jsonl there (the evidence behind profiles/update_path_tests.md)."""
    print(tag, row)
    if os.environ.get("P2P_RECORD_DIR"):
        with open(os.path.join(os.environ["P2P_RECORD_DIR"], "update_path.jsonl"), "a") as f:
            f.write(json.dumps({"case": tag, **row}) + "\n")


def _cmp(got, x64, tol):
    """(ok, max error, max tolerance, max E-free ratio err / tol) of a GPU result against the oracle."""
    got = got.detach().double().cpu().reshape(x64.shape)
    err = (got - x64.double()).abs()
    ok = bool(torch.isfinite(got).all()) and bool((err <= tol).all())
    return ok, float(err.max()), float(tol.max()), float((err / tol.clamp_min(1e-300)).max())


# ======================================================================================= Adam
def _fused(name, init):
    case = O.ADAM_CASES[name]
    ps = [[torch.nn.Parameter(p.to(DEV)) for p in grp] for grp in O.adam_case_params(name, init)]
    opt = FusedAdam([dict(params=grp, lr=g.get("lr", 2e-4), betas=g.get("betas", (0.5, 0.999)),
                          weight_decay=g.get("wd", 0.0)) for grp, g in zip(ps, case["groups"])])
    if "step0" in case:
        sd = opt.state_dict()
        sd["device_step"] = [case["step0"]] * len(ps)
        opt.load_state_dict(sd)
    return ps, opt


def _state(opt, ps):
    return [t.detach().clone() for grp in ps for p in grp
            for t in (p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])] + [t.clone() for t in opt._step_t]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _set_grads(name, ps, k):
    for grp, gs in zip(ps, O.adam_case_grads(name, k)):
        for p, g in zip(grp, gs):
            p.grad = g.to(DEV)


def _play(name, opt, ps, k):
    """Step k of a case, eagerly: its gradients, its learning rates, its skip flag."""
    case = O.ADAM_CASES[name]
    _set_grads(name, ps, k)
    for gi, lr in enumerate(case.get("lrs", {}).get(k, ())):
        opt.param_groups[gi]["lr"] = lr
    skip = case.get("skips", {}).get(k)
    opt.step(skip=None if skip is None else torch.tensor(skip, device=DEV))
    return skip


def _check_step(tag, opt, ps, rows):
    worst = {"p": [0.0] * 4, "m": [0.0] * 4, "v": [0.0] * 4}   # error, E, error / bound, bound
    bad = []
    for gi, i, nm, x64, tol, x32 in rows:
        p = ps[gi][i]
        got = {"p": p, "m": opt.state[p]["exp_avg"], "v": opt.state[p]["exp_avg_sq"]}[nm]
        ok, err, tmax, ratio = _cmp(got, x64, tol)
        E = float((x32.double() - x64).abs().max())
        w = worst[nm]
        w[:] = max(w[0], err), max(w[1], E), max(w[2], ratio), max(w[3], tmax)
        if not ok:
            bad.append((gi, i, nm, err, tmax, ratio))
    _record(tag, **{f"{nm}_err_E_ratio_bound": ["%.3e" % x for x in w] for nm, w in worst.items()})
    assert not bad, (tag, bad[:6])


@pytest.mark.parametrize("init", O.INITS)
@pytest.mark.parametrize("name", list(O.ADAM_CASES))
def test_adam_state_matches_the_oracle_after_every_step(name, init):
    """exp_avg, exp_avg_sq and the parameter after every step of every case (tensor sizes around
    the 4096 chunk and n % 4, 100 tensors through the MT_MAX = 40 flush loop, weight decay with
    two groups, device steps 999 / 19999, lr changes, skips), from unit, 1e-3 and zero
    parameters: the floor of p is steps x ulp(|p|) plus the propagated floors of the update
    (AdamOracle), so from zero / 1e-3 the movement itself is compared.  A skipped step leaves
    parameters, moments and the device step counter bitwise unchanged; the device counter
    follows the unskipped steps only."""
    case = O.ADAM_CASES[name]
    ps, opt = _fused(name, init)
    t = case.get("step0", 0.0)
    for k, rows in enumerate(O.adam_trajectory(name, init)):
        before = _state(opt, ps)
        skip = _play(name, opt, ps, k)
        torch.cuda.synchronize()
        if skip:
            assert _same(before, _state(opt, ps)), (name, init, k)
        else:
            t += 1.0
        assert [float(x) for x in opt._step_t] == [t] * len(ps)
        _check_step(f"adam/{name}/{init}/step{k}", opt, ps, rows)


def test_adam_state_dict_round_trip_continues_bitwise():
    name = "wd_groups"
    ps, opt = _fused(name, "unit")
    qs, ref = _fused(name, "unit")
    for k in range(2):
        _play(name, opt, ps, k)
        _play(name, ref, qs, k)
    sd = copy.deepcopy(opt.state_dict())
    assert sd["device_step"] == [2.0, 2.0]
    rs = [[torch.nn.Parameter(p.detach().clone()) for p in grp] for grp in ps]
    new = FusedAdam([dict(params=grp) for grp in rs])
    new.load_state_dict(sd)
    for k in range(2, 4):
        _play(name, new, rs, k % 3)
        _play(name, ref, qs, k % 3)
    assert _same(_state(new, rs), _state(ref, qs))


def test_guarded_step_skips_on_a_nan_loss_then_updates():
    ps, opt = _fused("guarded", "milli")
    _set_grads("guarded", ps, 0)
    before = _state(opt, ps)
    skipped = guarded_step(opt, None, None, torch.tensor(float("nan"), device=DEV), torch.tensor(1.0, device=DEV))
    assert float(skipped) == 1.0 and _same(before, _state(opt, ps))
    skipped = guarded_step(opt, None, skipped, torch.tensor(0.25, device=DEV))
    assert float(skipped) == 1.0 and float(opt._step_t[0]) == 1.0
    assert not any(torch.equal(a, b) for a, b in zip(before, _state(opt, ps)))
    _check_step("adam/guarded_step", opt, ps, O.adam_trajectory("guarded", "milli")[0])


def test_adam_bucket_view_gradients_equal_separate_gradients_bitwise():
    """Gradients as views of one flat fp32 buffer laid out as GradReducer._add_bucket lays them
    out (off += n, no padding): the float4-path tensors start 4 bytes off a 16-byte boundary."""
    ps, opt = _fused("bucket", "unit")
    qs, ref = _fused("bucket", "unit")
    flat = torch.zeros(sum(p.numel() for p in ps[0]), device=DEV)
    off = 0
    for p in ps[0]:
        p.grad = flat[off:off + p.numel()].view_as(p)
        off += p.numel()
    assert [p.grad.data_ptr() % 16 for p in ps[0]][1:3] == [4, 4] and flat.data_ptr() % 16 == 0
    for k, rows in enumerate(O.adam_trajectory("bucket", "unit")):
        for p, g in zip(ps[0], O.adam_case_grads("bucket", k)[0]):
            p.grad.copy_(g)
        opt.step()
        _play("bucket", ref, qs, k)
        assert _same(_state(opt, ps), _state(ref, qs))
        _check_step(f"adam/bucket_views/step{k}", opt, ps, rows)


@pytest.mark.parametrize("init", O.INITS)
def test_adam_graph_replay_follows_lr_and_skip_like_eager(init):
    """One step(skip=flag) captured with static gradient buffers (thread_local capture mode, a
    single stream), replayed as (a) lr 2e-4 flag 0, (b) lr 1e-4 + sync_lr() flag 0, (c) flag 1,
    (d) flag 0: after every replay bitwise the eager sequence, and the oracle within the bound."""
    name = "graph"
    case = O.ADAM_CASES[name]
    ps, opt = _fused(name, init)
    qs, ref = _fused(name, init)
    for grp in ps:
        for p in grp:
            p.grad = torch.zeros_like(p)
    flag = torch.zeros((), device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        opt.step(skip=flag)
    for k, rows in enumerate(O.adam_trajectory(name, init)):
        for grp, gs in zip(ps, O.adam_case_grads(name, k)):
            for p, g in zip(grp, gs):
                p.grad.copy_(g)
        if k in case["lrs"]:
            opt.param_groups[0]["lr"] = case["lrs"][k][0]
            opt.sync_lr()
        flag.fill_(case["skips"][k])
        graph.replay()
        _play(name, ref, qs, k)
        torch.cuda.synchronize()
        assert _same(_state(opt, ps), _state(ref, qs)), (init, k)
        _check_step(f"adam/graph/{init}/replay{k}", opt, ps, rows)


def test_adam_binding_rejects_moments_that_do_not_match_the_parameter():
    p, g, v = (torch.zeros(8, device=DEV) for _ in range(3))
    m = torch.zeros(12, device=DEV)   # larger than p: harmless even unchecked
    lr, step = torch.full((1,), 2e-4, device=DEV), torch.ones(1, device=DEV)
    with pytest.raises(RuntimeError, match="adam: moment sizes"):
        torch.ops.p2p.adam([p], [g], [m], [v], lr, step, 0.5, 0.999, 1e-8, 0.0, None)
    with pytest.raises(RuntimeError, match="adam: fp32 moments"):
        torch.ops.p2p.adam([p], [g], [v.double()], [v], lr, step, 0.5, 0.999, 1e-8, 0.0, None)
    torch.cuda.synchronize()
    assert float(p.abs().max()) == 0.0 and float(m.abs().max()) == 0.0


# ===================================================================== spectral-norm gradient
@pytest.mark.parametrize("correlated", [True, False])
@pytest.mark.parametrize("shape", O.SN_SHAPES)
def test_sn_wgrad_matches_the_oracle(shape, correlated):
    """sn_wgrad called directly on fp32 inputs against s G - <G, W> s^2 u v^T in float64, with
    G = randn + 3 W (the sigma path dominates, so its sign and factor are visible) and a purely
    random G; scale from sn_scale on the same W, u, v, itself checked against 1 / (u^T W v) after
    one power iteration in float64.  Floors: O.sn_wgrad_floor, O.sn_scale_floor.  acc mode: the
    result is acc_before + gradient, returned in acc itself, bitwise repeatable."""
    W, G, u0, v0 = O.sn_inputs(*shape, correlated, 3)
    Wd, Gd, u, v = W.to(DEV), G.to(DEV), u0.to(DEV), v0.to(DEV)
    scale = torch.ops.p2p.sn_scale(Wd, u, v)
    s64, s32 = O.sn_power_iter(W, u0, O.F64)[0], O.sn_power_iter(W, u0, O.F32)[0]
    s_tol = max(10 * abs(float(s32) - float(s64)), O.sn_scale_floor(W, u0) * abs(float(s64)))
    s_err = abs(float(scale) - float(s64))
    uc, vc, sc = u.cpu(), v.cpu(), scale.cpu()
    tag = f"sn_wgrad/{shape[0]}x{shape[1]}/{'correlated' if correlated else 'random'}"
    acc0 = torch.randn(shape, generator=torch.Generator().manual_seed(4))
    res = {}
    for mode, a0 in (("out", None), ("acc", acc0)):
        acc = None if a0 is None else a0.to(DEV)
        out = torch.ops.p2p.sn_wgrad(Gd, Wd, u, v, scale, acc)
        if acc is not None:
            assert out.data_ptr() == acc.data_ptr()
            again = a0.to(DEV)
            torch.ops.p2p.sn_wgrad(Gd, Wd, u, v, scale, again)
            assert torch.equal(again, acc)
        else:
            assert torch.equal(out, torch.ops.p2p.sn_wgrad(Gd, Wd, u, v, scale, None))
        o64, o32 = O.sn_wgrad(G, W, uc, vc, sc, O.F64, a0), O.sn_wgrad(G, W, uc, vc, sc, O.F32, a0)
        tol = O.tol_of(o32, o64, O.sn_wgrad_floor(G, W, uc, vc, sc, a0))
        res[mode] = _cmp(out, o64, tol) + (float((o32.double() - o64).abs().max()),)
    _record(tag, scale_err="%.3e" % s_err, scale_tol="%.3e" % s_tol,
            **{m: ["%.3e" % x for x in r[1:]] for m, r in res.items()})
    assert s_err <= s_tol
    assert all(r[0] for r in res.values()), res


# ================================================================================ column sums
@pytest.mark.parametrize("C", O.COLSUM_C)
def test_colsum_matches_the_oracle(C):
    """colsum of bf16 NHWC inputs against the float64 sum of the bf16 values, for every M of
    COLSUM_M, scale 1 and 0.5, with and without accumulate onto a non-zero out, and for C = 8 also
    the padded out.numel() = 1 and 3 (the logits and image bias gradients), whose neighbours in a
    larger buffer must stay untouched; two calls are bitwise equal.  Floor: O.colsum_floor."""
    worst = [0.0] * 4   # error, E, error / bound, bound
    for mi, shape in enumerate(O.COLSUM_M):
        x = O.colsum_input(shape, C, 10 * C + mi)
        xd = x.to(DEV)
        assert xd.is_contiguous(memory_format=torch.channels_last)
        for scale in (1.0, 0.5):
            for cout in ((C, 1, 3) if C == 8 else (C,)):
                before = torch.randn(cout, generator=torch.Generator().manual_seed(5))
                for b in (None, before):
                    outs = []
                    for _ in range(2):
                        big = torch.full((C + 4,), 77.0, device=DEV)
                        if b is not None:
                            big[:cout] = b.to(DEV)
                        torch.ops.p2p.colsum(xd, big[:cout], scale, b is not None)
                        outs.append(big)
                    assert torch.equal(outs[0], outs[1])
                    assert bool((outs[0][cout:] == 77.0).all()), (C, shape, cout)
                    o64, o32 = O.colsum(x, cout, scale, O.F64, b), O.colsum(x, cout, scale, O.F32, b)
                    tol = O.tol_of(o32, o64, O.colsum_floor(x, cout, scale, b))
                    ok, err, tmax, ratio = _cmp(outs[0][:cout], o64, tol)
                    worst = [max(worst[0], err), max(worst[1], float((o32.double() - o64).abs().max())),
                             max(worst[2], ratio), max(worst[3], tmax)]
                    assert ok, (C, shape, scale, cout, b is not None, err, tmax)
    _record(f"colsum/C{C}", err_E_ratio_bound=["%.3e" % w for w in worst])


# ===================================================================================== losses
def _dev_pair(a, b, misaligned):
    """The inputs on the GPU; ``misaligned``: as views one element into a larger buffer."""
    def put(x):
        if x is None:
            return None
        if not misaligned:
            return x.to(DEV)
        buf = torch.empty(x.numel() + 1, dtype=x.dtype, device=DEV)
        buf[1:] = x.to(DEV)
        return buf[1:]
    return put(a), put(b)


@pytest.mark.parametrize("dtype", list(O.LOSS_DTYPES))
@pytest.mark.parametrize("kind", range(8))
def test_loss_kernels_match_the_oracle(kind, dtype):
    """loss_fwd / loss_bwd of every kind on bf16 and fp32 inputs of 1 ... 70001 elements with the
    planted edge elements (O.loss_inputs), targets 0, 1, 0.9, upstream gradient 3.

    Dispatch (p2p_loss_fwd / p2p_loss_bwd): 16-byte aligned a (and b, and the fresh gradient
    buffers, which always are) take loss_partial_vec_kernel / loss_grad_vec_kernel -- torch
    allocations are aligned, so the plain inputs reach them, with a tail block whenever
    n % (4 fp32 | 8 bf16) != 0 and nothing but the tail at n = 1, 5; the same values as views one
    element into a larger buffer (4 or 2 bytes off) take the scalar loss_partial_kernel /
    loss_grad_kernel.  Both results must meet the bound.  Floors: O.loss_fwd, O.loss_bwd."""
    dt = O.LOSS_DTYPES[dtype]
    worst = {"fwd": [0.0] * 4, "bwd": [0.0] * 4}   # error, E, error / bound, bound
    gout = torch.tensor([3.0], device=DEV)
    for n in O.LOSS_N:
        a, b = O.loss_inputs(kind, n, dt, 1000 * kind + n)
        for t in (O.LOSS_T if kind < 3 else [0.0]):
            v64, vfl = O.loss_fwd(kind, a, b, t, 1.0 / n, O.F64)
            v32, _ = O.loss_fwd(kind, a, b, t, 1.0 / n, O.F32)
            vtol = O.tol_of(v32, v64, vfl)
            g64, gfl = O.loss_bwd(kind, a, b, t, 1.0 / n, 3.0, O.F64)
            g32, _ = O.loss_bwd(kind, a, b, t, 1.0 / n, 3.0, O.F32)
            gtol = O.tol_of(g32, g64, gfl)
            for mis in (False, True):
                ad, bd = _dev_pair(a, b, mis)
                assert (ad.data_ptr() % 16 != 0) == mis
                val = torch.ops.p2p.loss_fwd(ad, bd, kind, t, 1.0 / n)
                ok, err, tmax, ratio = _cmp(val, v64, vtol)
                w = worst["fwd"]
                w[:] = max(w[0], err), max(w[1], abs(float(v32) - float(v64))), max(w[2], ratio), max(w[3], tmax)
                assert ok and val.dtype == torch.float32, (kind, dtype, n, t, mis, err, tmax)
                assert torch.equal(val, torch.ops.p2p.loss_fwd(ad, bd, kind, t, 1.0 / n))
                ga, none = torch.ops.p2p.loss_bwd(ad, bd, kind, t, 1.0 / n, gout, True, False)
                assert none is None and ga.dtype == dt
                ok, err, tmax, ratio = _cmp(ga, g64, gtol)
                w = worst["bwd"]
                w[:] = (max(w[0], err), max(w[1], float((g32.double() - g64).abs().max())), max(w[2], ratio),
                        max(w[3], tmax))
                assert ok, (kind, dtype, n, t, mis, err, tmax)
                if kind in O.PAIR_KINDS:
                    ga2, gb2 = torch.ops.p2p.loss_bwd(ad, bd, kind, t, 1.0 / n, gout, True, True)
                    none, gb = torch.ops.p2p.loss_bwd(ad, bd, kind, t, 1.0 / n, gout, False, True)
                    assert none is None and torch.equal(ga2, ga) and torch.equal(gb, gb2)
                    assert torch.equal(gb2, -ga2) and bool((ga2[0] == 0).all())   # a[0] == b[0]
    _record(f"loss/kind{kind}/{dtype}", **{k + "_err_E_ratio_bound": ["%.3e" % x for x in w] for k, w in worst.items()})


@pytest.mark.parametrize("dtype", list(O.LOSS_DTYPES))
def test_loss_wrappers_match_the_oracle_through_autograd(dtype):
    """ops.mse_const / bce_logits_const / bce_const / l1 (plain, lrelu- and relu-gated) / mse:
    value and the gradients of (loss * 3).backward(), for a alone, b alone and both."""
    dt = O.LOSS_DTYPES[dtype]
    const = {0: ops.mse_const, 1: ops.bce_logits_const, 2: ops.bce_const}
    pair = {3: lambda a, b: ops.l1(a, b), 4: ops.mse, 6: lambda a, b: ops.l1(a, b, gate_a="lrelu"),
            7: lambda a, b: ops.l1(a, b, gate_a="relu")}
    for n in (189, 2051):
        for kind in (0, 1, 2, 3, 4, 6, 7):
            a, b = O.loss_inputs(kind, n, dt, 1000 * kind + n)
            for t in (O.LOSS_T if kind < 3 else [0.0]):
                v64, vfl = O.loss_fwd(kind, a, b, t, 1.0 / n, O.F64)
                vtol = O.tol_of(O.loss_fwd(kind, a, b, t, 1.0 / n, O.F32)[0], v64, vfl)
                g64, gfl = O.loss_bwd(kind, a, b, t, 1.0 / n, 3.0, O.F64)
                gtol = O.tol_of(O.loss_bwd(kind, a, b, t, 1.0 / n, 3.0, O.F32)[0], g64, gfl)
                for need in ((True, False), (False, True), (True, True)) if kind in pair else ((True, False),):
                    ad = a.to(DEV).requires_grad_(need[0])
                    bd = None if b is None else b.to(DEV).requires_grad_(need[1])
                    val = const[kind](ad, t) if kind in const else pair[kind](ad, bd)
                    (val * 3).backward()
                    assert _cmp(val, v64, vtol)[0], (kind, n, t)
                    if need[0]:
                        assert ad.grad.dtype == dt and _cmp(ad.grad, g64, gtol)[0], (kind, n, t, need)
                    if need[1]:
                        assert _cmp(bd.grad, -g64, gtol)[0], (kind, n, t, need)
                    if need == (True, True):
                        assert torch.equal(bd.grad, -ad.grad)


# ================================================================ guard and scalar composition
def test_guard_flag_with_eight_scalars_and_every_kind_of_bad_value():
    def sc(x):
        return torch.tensor(x, device=DEV, dtype=torch.float32)
    cnt = torch.zeros((), device=DEV)
    good = [sc(float(i)) for i in range(7)]
    expect = 0.0
    for last, bad in ((float("nan"), 1.0), (float("inf"), 1.0), (float("-inf"), 1.0), (3.4e38, 0.0),
                      (-3.4e38, 0.0), (1e-45, 0.0)):
        x = sc(last)
        assert last != last or float(x) == float(np.float32(last))   # the denormal survives the copy
        expect += bad
        assert float(nonfinite(*good, x, counter=cnt)) == bad and float(cnt) == expect
    assert float(nonfinite(sc(float("nan")), *good, counter=cnt)) == 1.0 and float(cnt) == expect + 1.0
    with pytest.raises(RuntimeError, match="guard_flag: 1..8"):
        nonfinite(*good, sc(1.0), sc(2.0), counter=cnt)
    assert float(cnt) == expect + 1.0


@pytest.mark.parametrize("n", [1, 15, 16, 17, 31])
def test_lincomb_n_through_autograd(n):
    """sum_i w_i t_i with zero and negative weights, chained 15 terms at a time beyond 16: value
    within max(10 E, 2 n u sum |w_i t_i|); the gradient of (out * 3) is the single fp32 product
    3 w_i per term (the running total re-enters each chain with weight 1), compared bitwise."""
    vals, ws = O.lincomb_terms(n)
    ts = [torch.tensor(v, device=DEV, requires_grad=True) for v in vals]
    out = ops.lincomb_n(ts, ws)
    (out * 3).backward()
    o64, o32 = O.lincomb_n(vals, ws, O.F64), O.lincomb_n(vals, ws, O.F32)
    tol = max(10 * abs(float(o32) - float(o64)), O.lincomb_n_floor(vals, ws))
    err = abs(float(out.detach().double()) - float(o64))
    _record(f"lincomb_n/{n}", err="%.3e" % err, E="%.3e" % abs(float(o32) - float(o64)), tol="%.3e" % tol)
    assert out.dtype == torch.float32 and out.dim() == 0 and err <= tol
    for t, w in zip(ts, ws):
        assert t.grad.cpu().numpy().reshape(()).tobytes() == (np.float32(3.0) * np.float32(w)).tobytes(), (n, w)


def test_lincomb_n_rejects_a_python_float_term():
    from p2p_pytorch_amd.ops import hip
    t = torch.tensor(1.0, device=DEV, requires_grad=True)
    with pytest.raises(ValueError, match="tensor terms only"):
        hip.lincomb_n([t, 0.5], [1.0, 2.0])
