"""The bounds of tests/test_update_path_gpu.py are reachable: on every case, the float32
evaluation of the float64 oracle (tests/update_path_oracles.py) passes max(10 x E, floor) by
itself, every oracle value is finite, and ``torch.optim.Adam`` agrees with the Adam oracle.

``torch.optim.Adam`` is a cross-check only: it forms 1 - b2 in double from the unrounded b2, the
kernel in fp32 from the rounded one (1.3e-5 relative in exp_avg_sq), hence 1e-4.
"""
import pytest
import torch

import update_path_oracles as O


def _within(x32, x64, tol):
    err = (x32.double() - x64.double()).abs()
    return bool(torch.isfinite(x64.double()).all()) and bool((err <= tol).all())


@pytest.mark.parametrize("init", O.INITS)
@pytest.mark.parametrize("name", list(O.ADAM_CASES))
def test_adam_fp32_oracle_is_inside_the_bound_at_every_step(name, init):
    for step in O.adam_trajectory(name, init):
        for gi, i, nm, x64, tol, x32 in step:
            assert _within(x32, x64, tol), (name, init, gi, i, nm)
            assert bool((tol >= 0).all())


@pytest.mark.parametrize("name", ["sizes", "wd_groups", "lr_change"])
def test_torch_adam_agrees_with_the_adam_oracle_in_the_moments(name):
    case = O.ADAM_CASES[name]
    params = [[torch.nn.Parameter(p.double()) for p in ps] for ps in O.adam_case_params(name, "unit")]
    opt = torch.optim.Adam([dict(params=ps, lr=g.get("lr", 2e-4), betas=g.get("betas", (0.5, 0.999)), eps=1e-8,
                                 weight_decay=g.get("wd", 0.0)) for ps, g in zip(params, case["groups"])])
    for k, step in enumerate(O.adam_trajectory(name, "unit")):
        for gi, lr in enumerate(case.get("lrs", {}).get(k, ())):
            opt.param_groups[gi]["lr"] = lr
        for ps, gs in zip(params, O.adam_case_grads(name, k)):
            for p, g in zip(ps, gs):
                p.grad = g.double()
        opt.step()
        for gi, i, nm, x64, _, _ in step:
            st = opt.state[params[gi][i]]
            got = {"p": params[gi][i].detach(), "m": st["exp_avg"], "v": st["exp_avg_sq"]}[nm]
            # relative to the tensor's largest magnitude: b m + (1 - b) g cancels in single elements
            assert float((got - x64).abs().max()) <= 1e-4 * float(x64.abs().max()) + 1e-30, (name, k, gi, i, nm)


@pytest.mark.parametrize("correlated", [True, False])
@pytest.mark.parametrize("shape", O.SN_SHAPES[:2])   # the 4 M-element case is the same code on the CPU
def test_sn_fp32_oracle_is_inside_the_bound(shape, correlated):
    W, G, u0, _ = O.sn_inputs(*shape, correlated, 3)
    s64, u, v = O.sn_power_iter(W, u0, O.F64)
    s32 = O.sn_power_iter(W, u0, O.F32)[0]
    rel = O.sn_scale_floor(W, u0)
    assert abs(float(s32) - float(s64)) <= max(10 * abs(float(s32) - float(s64)), rel * abs(float(s64)))
    sc = s32.reshape(1)
    acc = torch.randn(shape, generator=torch.Generator().manual_seed(4))
    for a in (None, acc):
        o64 = O.sn_wgrad(G, W, u.float(), v.float(), sc, O.F64, a)
        o32 = O.sn_wgrad(G, W, u.float(), v.float(), sc, O.F32, a)
        assert _within(o32, o64, O.tol_of(o32, o64, O.sn_wgrad_floor(G, W, u.float(), v.float(), sc, a)))
    if correlated and shape == (64, 1024):   # the sigma path is not masked by the direct term
        k = (G.double() * W.double()).sum() * float(sc) ** 2
        assert float(k * u.abs().max() * v.abs().max()) > 10 * float(sc) * float(G.abs().mean())


@pytest.mark.parametrize("C", O.COLSUM_C)
def test_colsum_fp32_oracle_is_inside_the_bound(C):
    for mi, shape in enumerate(O.COLSUM_M):
        x = O.colsum_input(shape, C, 10 * C + mi)
        for scale in (1.0, 0.5):
            for cout in ((C, 1, 3) if C == 8 else (C,)):
                before = torch.randn(cout, generator=torch.Generator().manual_seed(5))
                for b in (None, before):
                    o64, o32 = O.colsum(x, cout, scale, O.F64, b), O.colsum(x, cout, scale, O.F32, b)
                    assert _within(o32, o64, O.tol_of(o32, o64, O.colsum_floor(x, cout, scale, b)))


@pytest.mark.parametrize("dtype", list(O.LOSS_DTYPES))
@pytest.mark.parametrize("kind", range(8))
def test_loss_fp32_oracle_is_inside_the_bound_and_finite(kind, dtype):
    for n in O.LOSS_N:
        a, b = O.loss_inputs(kind, n, O.LOSS_DTYPES[dtype], 1000 * kind + n)
        for t in (O.LOSS_T if kind < 3 else [0.0]):
            v64, fl = O.loss_fwd(kind, a, b, t, 1.0 / n, O.F64)
            v32, _ = O.loss_fwd(kind, a, b, t, 1.0 / n, O.F32)
            assert _within(v32, v64, O.tol_of(v32, v64, fl)), (kind, n, t)
            g64, gfl = O.loss_bwd(kind, a, b, t, 1.0 / n, 3.0, O.F64)
            g32, _ = O.loss_bwd(kind, a, b, t, 1.0 / n, 3.0, O.F32)
            assert _within(g32, g64, O.tol_of(g32, g64, gfl)), (kind, n, t)


def test_planted_loss_edges_are_what_they_claim():
    a, b = O.loss_inputs(6, 8, torch.float32, 0)
    g = O.loss_bwd(6, a, b, 0.0, 1.0, 1.0, O.F64)[0]
    assert a[0] == b[0] and g[0] == 0.0 and a[1] == 0.0 and abs(float(g[1])) == pytest.approx(0.2, rel=1e-7)
    assert O.loss_bwd(7, *O.loss_inputs(7, 8, torch.float32, 0), 0.0, 1.0, 1.0, O.F64)[0][1] == 0.0
    a, _ = O.loss_inputs(2, 8, torch.bfloat16, 0)
    assert a[0] == 0.0 and a[1] == 1.0
    assert float(O.loss_fwd(2, a[:1], None, 0.9, 1.0, O.F64)[0]) == pytest.approx(90.0, rel=1e-6)   # the -100 clamp
    assert abs(float(O.loss_bwd(2, a[:1], None, 0.9, 1.0, 1.0, O.F64)[0][0])) == pytest.approx(0.9e12, rel=1e-6)
    a, _ = O.loss_inputs(1, 8, torch.float32, 0)
    assert a[:4].tolist() == [80.0, -80.0, 100.0, -100.0]


@pytest.mark.parametrize("n", [1, 15, 16, 17, 31])
def test_lincomb_n_fp32_oracle_is_inside_the_bound(n):
    vals, ws = O.lincomb_terms(n)
    o64, o32 = O.lincomb_n(vals, ws, O.F64), O.lincomb_n(vals, ws, O.F32)
    assert abs(float(o32) - float(o64)) <= max(10 * abs(float(o32) - float(o64)), O.lincomb_n_floor(vals, ws))
    assert 0.0 in ws or n == 1
    assert any(w < 0 for w in ws) or n == 1
