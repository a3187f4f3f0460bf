"""CPU checks of the leave-one-out pass (irbfn_amd/loo.py, irbfn_rows_quad_f64): the float64 statement of tests/_loo_util.py against
a brute-force refit without the row, its trace against the Gram matrix alone, the refusals of the ABI decided before any HIP call,
and ``loo.factor`` on CPU tensors (``solve``'s steps: the fit bit for bit, P = [T^T | sol])."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _linear_fit_util as lu
import _loo_util as lo
from irbfn_amd import _lib, build, linear_fit, loo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARG = 0, -1
RIDGE = 1e-8


def _fit_case64():
    cfg, centers, log_sigs, x, y, h64, gsum = lu.fit_case()
    return h64, y.astype(np.float64), RIDGE * np.trace(h64.T @ h64) / h64.shape[1]


def test_symbol_is_declared_exported_bound_and_built():
    hdr = open(os.path.join(ROOT, "include", "irbfn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\birbfn_rows_quad_f64\s*\(", code)
    assert hasattr(_lib.load(), "irbfn_rows_quad_f64") and "irbfn_rows_quad_f64" in _lib.SIGNATURES
    assert any(u[0] == "rows_quad_f64.hip" and u[1] == "rows_quad_f64.o" for u in build.UNITS)
    import irbfn_amd
    assert irbfn_amd.loo is loo
    for name in ("factor", "rows_quad", "leverage", "loo", "select_ridge", "select_scale", "Factor", "LooResult", "RidgeSearch"):
        assert hasattr(loo, name)


def test_status_table_without_gpu():
    lib = _lib.load()
    one = C.c_void_p(8)                  # a non-null pointer that is never dereferenced: every call stops earlier
    good = dict(z=one, ldz=20, rows=100, m=17, p=one, ldp=30, nd=10, q=one, v=one)

    def call(**kw):
        a = dict(good, **kw)
        return lib.irbfn_rows_quad_f64(a["z"], a["ldz"], a["rows"], a["m"], a["p"], a["ldp"], a["nd"], a["q"], a["v"], None)
    assert call(z=None) == BAD_ARG and call(p=None) == BAD_ARG and call(q=None) == BAD_ARG and call(v=None) == BAD_ARG
    assert call(m=0) == BAD_ARG and call(m=-2) == BAD_ARG and call(m=8193, ldz=9000, ldp=9000) == BAD_ARG
    assert call(ldz=16) == BAD_ARG and call(ldp=26) == BAD_ARG and call(nd=-1) == BAD_ARG and call(nd=257, ldp=300) == BAD_ARG
    assert call(rows=-1) == BAD_ARG
    assert call(rows=0) == OK and call(rows=0, z=None, p=None, q=None, v=None) == OK        # nothing to do: no launch, no pointer needed
    assert call(rows=0, m=0) == BAD_ARG and call(rows=0, ldz=16) == BAD_ARG                # the shape is still checked


def test_statement_equals_the_refit_without_the_row():
    Zh, Y, lam = _fit_case64()
    st = lo.statement(Zh, Y, lam)
    assert st["cond"] < 1e3                                               # a condition on the input, not on the code
    top = int(np.argmax(st["leverage"]))
    rows = [top] + [r for r in (0, 1, 2, 500, 777, 1234, 1499) if r != top][:7]
    assert len(rows) == 8
    brute = lo.brute_loo(Zh, Y, lam, rows)
    err = np.abs(st["loo_residual"][rows] - brute).max()
    print(f"cond {st['cond']:.1f}  max leverage {st['leverage'][top]:.4f} (row {top})  |e / (1 - l) - refit| {err:.2e}  "
          f"max|y| {np.abs(Y).max():.2f}  press / rss {st['press'].sum() / st['rss'].sum():.4f}")
    assert err <= 1e-10 * np.abs(Y).max()
    assert (st["leverage"] > 0).all() and (st["leverage"] < 1).all()
    assert (st["press"] >= st["rss"]).all()
    # the statement's solution is the stacked least-squares one
    W, b, rss = lu.lstsq_ref(Zh, Y, lam, True)
    assert np.abs(st["sol"] - np.vstack([W, b[None]])).max() <= 1e-10 * np.abs(W).max()
    assert (np.abs(st["rss"] - rss) <= 1e-9 * (Y ** 2).sum(0)).all()


@pytest.mark.parametrize("ridge", (1e-10, 1e-8, 1e-4))
def test_statement_trace_equals_the_trace_from_the_gram_matrix(ridge):
    Zh, Y, _ = _fit_case64()
    lam = ridge * np.trace(Zh.T @ Zh) / Zh.shape[1]
    st = lo.statement(Zh, Y, lam)
    tr = lo.trace_from_gram(lu.stacked_gram(Zh, Y), Zh.shape[1], lam)
    assert abs(st["trace"] - tr) <= 1e-10 * tr and tr <= Zh.shape[1] + 1 + 1e-9
    if ridge == 1e-4:
        assert tr < Zh.shape[1] + 1 - 1e-3                                # the ridge is visible in the effective parameters


def test_numpy_float64_sits_well_inside_the_kernels_bound():
    Zh, Y, lam = _fit_case64()
    Z, A0, A, s = lo.system(Zh.astype(np.float32).astype(np.float64), lam)
    T = lo._solve_lower(np.linalg.cholesky(A * s[:, None] * s[None, :]), np.diag(s))
    z32 = Z.astype(np.float32)
    P = np.hstack([T.T, np.zeros((T.shape[0], 0))])
    q, _, qb, _ = lo.quad_ref(z32, P)
    q64 = ((Z @ T.T) ** 2).sum(1)
    worst = float((np.abs(q64 - q.astype(np.float64)) / qb).max())
    print(f"float64 NumPy against longdouble: {worst:.3f} of the q bound")
    assert worst <= 1.0                                                   # float64 in any order meets the any-order bound


@pytest.mark.parametrize("fit_bias", (True, False))
@pytest.mark.parametrize("ridge", (0.0, 1e-8, 1e-2))
def test_factor_is_solve_and_keeps_the_triangle(ridge, fit_bias):
    Zh, Y, _ = _fit_case64()
    K, O = Zh.shape[1], Y.shape[1]
    ne = linear_fit.NormalEquations(lu.Shape(K, O), G=torch.from_numpy(lu.stacked_gram(Zh, Y)))
    fac, fit = loo.factor(ne, ridge=ridge, fit_bias=fit_bias), ne.solve(ridge=ridge, fit_bias=fit_bias)
    for a, b in ((fac.fit.kernel, fit.kernel), (fac.fit.bias, fit.bias), (fac.fit.rss, fit.rss), (fac.fit.sol, fit.sol)):
        assert a.numpy().tobytes() == b.numpy().tobytes()
    assert fac.fit.n == fit.n == fac.n == 1500 and fac.fit.ridge_abs == fit.ridge_abs == fac.ridge_abs and fac.fit_bias == fit_bias
    m = K + 1 if fit_bias else K
    P = fac.P.numpy()
    assert fac.m == m and fac.O == O and P.shape == (m, m + O) and fac.P.is_contiguous() and fac.P.dtype == torch.float64
    assert (np.tril(P[:, :m], -1) == 0).all() and P[:, m:].tobytes() == fit.sol.numpy().tobytes()
    st = lo.statement(Zh, Y, fac.ridge_abs, fit_bias)
    lev = ((lo.design(Zh, fit_bias) @ P[:, :m]) ** 2).sum(1)
    assert np.abs(lev - st["leverage"]).max() <= lo.SOLVE_RTOL * st["leverage"].max()
    assert tuple(fac.L.shape) == (m, m) and tuple(fac.s.shape) == (m,)


def test_factor_refuses_what_solve_refuses():
    Zh, Y = np.array(lu.fit_case()[5][:, :12]), lu.fit_case()[4].astype(np.float64)
    Zh[:, 5] = Zh[:, 2]                                                   # a duplicated column
    ne = linear_fit.NormalEquations(lu.Shape(12, 3), G=torch.from_numpy(lu.stacked_gram(Zh, Y)))
    with pytest.raises(ValueError, match="not positive definite at ridge=0; raise ridge"):
        loo.factor(ne, ridge=0.0)
    assert loo.factor(ne, ridge=1e-6).fit.kernel.numpy().tobytes() == ne.solve(ridge=1e-6).kernel.numpy().tobytes()
    G = ne.G.clone()
    G[3, :] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        loo.factor(linear_fit.NormalEquations(lu.Shape(12, 3), G=G))
    with pytest.raises(ValueError, match="no rows"):
        loo.factor(linear_fit.NormalEquations(lu.Shape(12, 3)))


def test_integer_cases_stay_below_2_to_53():
    z, p = lo.integer_case(257, 200, 17, seed=1)
    assert np.isnan(p[:, :200][np.tril_indices(200, -1)]).all() and np.isfinite(p[:, :200][np.triu_indices(200)]).all()
    assert 200 * (200 * 64) ** 2 < 2 ** 53
    q, v = lo.quad_int(z, p)
    qr, vr, _, _ = lo.quad_ref(z, p)
    assert np.array_equal(q, qr.astype(np.float64)) and np.array_equal(v, vr.astype(np.float64)) and q.max() > 1e6
