"""Leverages and leave-one-out errors of the closed-form output-layer fit on the device (``irbfn_rows_quad_f64``,
include/irbfn_hip.h): every row is used for fitting and for pricing.

``linear_fit`` solves (Z^T Z + Lambda) [W; b] = Z^T Y with z_n = [h(x_n) | 1].  The fit is a linear smoother, and one number per
row, the leverage l_n = z_n^T (Z^T Z + Lambda)^-1 z_n, prices it without a held-out part: with the ridge held fixed the residual
of row n under the fit of all *other* rows is exactly e_n / (1 - l_n) (Sherman-Morrison), so

    PRESS = sum_n |e_n / (1 - l_n)|^2        the sum of squared leave-one-out residuals, per output
    trace = sum_n l_n                        the effective number of parameters
    GCV   = n RSS / (n - trace)^2            per output
    1 + l(x)                                 the predictive variance factor of any query x (``leverage``; no labels needed)

    ne = linear_fit.NormalEquations(net).add(params, table.x, table.y)
    fac = loo.factor(ne, ridge=1e-8)                                  # fac.fit is ne.solve(ridge=1e-8), bit for bit
    res = loo.loo(net, params, table.x, table.y, fac, per_row=True)   # res.press, res.gcv, res.trace, res.loo_residual ...
    search = loo.select_ridge(net, params, table.x, table.y)          # the ridge by PRESS; loo.select_scale: the width multiplier

``factor`` is ``NormalEquations.solve`` itself (one factorisation serves both) and keeps the Cholesky factor L of the scaled
system: with T = L^-1 diag(s), l_n = |T z_n|^2.  The pass over the rows is the one of ``NormalEquations.add``
(``linear_fit.hidden_rows``): one hidden-layer launch and one K11 launch per chunk; the
rows x m x m / 2 product in float64 is never stored.  The reference has no counterpart (its "table cleaning" notebooks are not in
its snapshot): parity is unpinned; each stage is pinned against a float64 statement of it (tests/_loo_util.py).

The identities hold on the rows the accumulator was built from, at its ridge.  It works unchanged on ``ne.subset(...)`` /
``OLSResult.subnet(...)``: an OLS path is priced by PRESS per prefix.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .linear_fit import NormalEquations, _rows_f32, hidden_rows, with_fit
from .model import _ptr, _stream_ptr, to_device_f32
from .widths import finite_lists, search_scales


class Factor:
    """What ``factor`` keeps of a solved system of m = K + 1 columns (K without ``fit_bias``): ``L`` [m,m] the lower Cholesky factor
    of the scaled matrix diag(s) (A + Lambda) diag(s), ``s`` [m] the scaling, ``ridge_abs`` the absolute lambda, ``n`` the rows of
    the accumulator, ``fit_bias``, ``fit`` = the ``LinearFit`` (bit for bit that of ``solve``), and ``P`` [m, m + O] float64 on G's
    device = [ (L^-1 diag(s))^T | sol ]: what ``irbfn_rows_quad_f64`` reads."""

    def __init__(self, L, s, ridge_abs, n, fit_bias, fit, P):
        self.L, self.s, self.ridge_abs, self.n, self.fit_bias, self.fit, self.P = L, s, float(ridge_abs), int(n), bool(fit_bias), fit, P

    @property
    def m(self) -> int:
        return int(self.P.shape[0])

    @property
    def O(self) -> int:
        return int(self.P.shape[1] - self.P.shape[0])


def factor(ne: NormalEquations, ridge: float = 1e-8, fit_bias: bool = True) -> Factor:
    """``NormalEquations.solve`` with its refusals (no rows, non-finite entries of G, ``info != 0``, a pivot of the unit-diagonal
    matrix below m 2^-52), keeping the factor: ``fit`` is the ``LinearFit`` of the one factorisation ``solve`` returns, so it equals
    ``ne.solve(ridge, fit_bias)`` bit for bit.  On top of it one triangular solve against diag(s), O(m^3), once per factor."""
    import torch
    L, s, fit = ne._factorise(ridge, fit_bias)
    T = torch.linalg.solve_triangular(L, torch.diag(s), upper=False)               # L^-1 diag(s): lower triangular
    P = torch.cat([T.mT, fit.sol], dim=1).contiguous()
    return Factor(L, s, fit.ridge_abs, fit.n, fit_bias, fit, P)


def rows_quad(z, P, nd: int):
    """z [rows, m] float32 on the device (rows may be strided: ``z.stride(0) >= m``), P [m, m + nd] float64 on the same device
    (``P.stride(0) >= m + nd``) -> (q [rows], v [rows, nd]) float64 (``irbfn_rows_quad_f64``):
    q[n] = sum_{j<m} (sum_{k<=j} z[n,k] P[k,j])^2 -- the strict lower triangle of P[:, :m] is never read -- and
    v[n,o] = sum_k z[n,k] P[k, m + o]."""
    torch = _lib.require_gpu()
    lib = _lib.load()
    nd = int(nd)
    z, ldz = _rows_f32(z, "rows_quad needs z [rows, m]", torch)
    rows, m = z.shape
    if (not isinstance(P, torch.Tensor) or P.dtype != torch.float64 or P.device != z.device or P.dim() != 2 or nd < 0
            or tuple(P.shape) != (m, m + nd) or (m + nd > 1 and P.stride(1) != 1) or (m > 1 and P.stride(0) < m + nd)):
        raise ValueError(f"rows_quad: P must be a float64 tensor of shape ({m}, {m} + nd) with unit column stride on z's device")
    ldp = P.stride(0) if m > 1 else max(P.stride(0), m + nd)
    q = torch.empty((rows,), dtype=torch.float64, device=z.device)
    v = torch.empty((rows, nd), dtype=torch.float64, device=z.device)
    with torch.cuda.device(z.device):
        st = lib.irbfn_rows_quad_f64(_ptr(z), ldz, rows, m, _ptr(P), ldp, nd, _ptr(q), _ptr(v) if nd else None, _stream_ptr(torch))
    _lib.check(st, "irbfn_rows_quad_f64")
    return q, v


def _chunks(net, params, x, fac: Factor, batch_size: int, nd: int):
    """-> (chunks, xd): ``chunks`` yields (i, n, q [n], v [n, nd]) per chunk of ``batch_size`` rows of x, one ``irbfn_rows_quad_f64`` on
    each Z = [h | 1] of ``linear_fit.hidden_rows`` (no ones column for a factor without ``fit_bias``)."""
    K = int(net.num_kernels)
    if fac.m != K + (1 if fac.fit_bias else 0):
        raise ValueError(f"a factor of {fac.m} columns on a net of num_kernels={K} (fit_bias={fac.fit_bias})")
    xd, _, rows = hidden_rows(net, params, x, fac.m, K if fac.fit_bias else None, batch_size, "loo")
    if fac.P.device != xd.device:
        raise ValueError(f"the factor lives on {fac.P.device}, the rows on {xd.device}")
    P = fac.P if nd else fac.P[:, :fac.m]
    return ((i, n, *rows_quad(Z, P, nd)) for i, n, Z in rows), xd


def leverage(net, params: dict, x, fac: Factor, batch_size: int = 65536):
    """-> q [N] float64 on the device: the leverage z^T (Z^T Z + Lambda)^-1 z of every row of x [N,D] under the factor's system,
    z = [h(x) | 1] from the net's hidden layer under ``params`` (centres, widths and gate; the linear leaves are not read).  No
    labels are needed, and x need not be the fitted table: 1 + q is the predictive variance factor of a query, q the squared
    distance of its hidden layer from what the net was fitted on.  Bit for bit ``loo(...).leverage`` of the same rows."""
    torch = _lib.require_gpu()
    it, xd = _chunks(net, params, x, fac, batch_size, 0)
    out = torch.empty((xd.shape[0],), dtype=torch.float64, device=xd.device)
    for i, n, q, _ in it:
        out[i:i + n] = q
    return out


class LooResult:
    """What ``loo`` found, float64 on the device, nothing read by the host: ``n`` rows (an int); ``rss`` [O] = sum_n e_n^2 from the
    rows; ``press`` [O] = sum_n (e_n / (1 - l_n))^2; ``trace`` = sum_n l_n; ``gcv`` [O] = n rss / (n - trace)^2; ``max_leverage``
    and ``max_leverage_row`` (over the rows with a finite leverage; -inf / 0 without one); ``n_degenerate`` = the rows with
    1 - l_n <= 0 or a non-finite l_n: their leave-one-out residuals are ``inf``, and so is ``press``.  With ``per_row``:
    ``leverage`` [N], ``residual`` [N,O] = y - prediction and ``loo_residual`` [N,O]; else None.  ``press_mse`` = sum(press) /
    (n O), a host float."""

    def __init__(self, n, rss, press, trace, max_leverage, max_leverage_row, n_degenerate, leverage=None, residual=None,
                 loo_residual=None):
        self.n, self.rss, self.press, self.trace = int(n), rss, press, trace
        self.max_leverage, self.max_leverage_row, self.n_degenerate = max_leverage, max_leverage_row, n_degenerate
        self.leverage, self.residual, self.loo_residual = leverage, residual, loo_residual

    @property
    def gcv(self):
        return self.n * self.rss / (self.n - self.trace) ** 2

    @property
    def press_mse(self) -> float:
        return float(self.press.sum().item()) / (max(self.n, 1) * max(self.press.numel(), 1))


def loo(net, params: dict, x, y, fac: Factor, batch_size: int = 65536, per_row: bool = False) -> LooResult:
    """Residuals, leverages and leave-one-out residuals of the rows (x [N,D], y [N,O]) under the factor's fit.  Per chunk of
    ``batch_size`` rows: ``net._hidden_into`` into a reused Z, the ones column, one ``irbfn_rows_quad_f64`` launch that gives the
    leverage q and the float64 prediction v = z [W; b]; e = y - v and e / (1 - q) are torch operations on the device.  Nothing is
    read by the host.
    ``params`` gives the hidden layer only (centres, widths, gate); the output layer is the factor's solution ``fac.fit``,
    whatever ``linear/*`` of ``params`` hold.  The leave-one-out identity holds for the rows the accumulator behind ``fac`` was
    built from, with the ridge held fixed at ``fac.ridge_abs``."""
    torch = _lib.require_gpu()
    O = fac.O
    ys = tuple(y.shape)
    if len(ys) != 2 or ys[1] != O or O != int(net.out_features):
        raise ValueError(f"y must have shape (N, {O}) for a net of out_features={net.out_features}, got {ys}")
    if tuple(x.shape)[:1] != ys[:1]:
        raise ValueError(f"x has {tuple(x.shape)[0]} rows, y has {ys[0]}")
    it, xd = _chunks(net, params, x, fac, batch_size, O)
    yd = to_device_f32(y, torch, device=xd.device)
    dev, f64 = xd.device, torch.float64
    N = xd.shape[0]
    rss, press = torch.zeros(O, dtype=f64, device=dev), torch.zeros(O, dtype=f64, device=dev)
    trace = torch.zeros((), dtype=f64, device=dev)
    qmax = torch.full((), float("-inf"), dtype=f64, device=dev)
    qrow = torch.zeros((), dtype=torch.int64, device=dev)
    ndeg = torch.zeros((), dtype=torch.int64, device=dev)
    lev = torch.empty((N,), dtype=f64, device=dev) if per_row else None
    res = torch.empty((N, O), dtype=f64, device=dev) if per_row else None
    lres = torch.empty((N, O), dtype=f64, device=dev) if per_row else None
    inf = torch.full((), float("inf"), dtype=f64, device=dev)
    for i, n, q, v in it:
        e = yd[i:i + n].to(f64) - v
        d = 1.0 - q
        deg = ~(d > 0) | ~torch.isfinite(q)
        le = torch.where(deg[:, None], inf, e / d[:, None])
        rss += (e * e).sum(0)
        press += (le * le).sum(0)
        trace += q.sum()
        ndeg += deg.sum()
        cm, ci = torch.where(torch.isfinite(q), q, -inf).max(0)
        qrow = torch.where(cm > qmax, ci + i, qrow)
        qmax = torch.maximum(qmax, cm)
        if per_row:
            lev[i:i + n], res[i:i + n], lres[i:i + n] = q, e, le
    return LooResult(N, rss, press, trace, qmax, qrow, ndeg, lev, res, lres)


class RidgeSearch:
    """``ridges``; ``press`` [R][O], ``gcv`` [R][O] and ``trace`` [R] per ridge as host lists (``inf`` where the system was refused
    or a row was degenerate); ``best`` = the index of the smallest summed PRESS (ties: the smaller ridge); ``fit`` and ``params`` =
    the best ridge's ``LinearFit`` and the tree with it."""

    def __init__(self, ridges, press, gcv, trace, best, fit, params):
        self.ridges, self.press, self.gcv, self.trace = tuple(ridges), press, gcv, trace
        self.best, self.fit, self.params = int(best), fit, params

    @property
    def best_ridge(self) -> float:
        return self.ridges[self.best]


def select_ridge(net, params: dict, x, y, ridges=(1e-10, 1e-8, 1e-6, 1e-4, 1e-2), fit_bias: bool = True,
                 batch_size: int = 65536) -> RidgeSearch:
    """The ridge from all rows: one ``NormalEquations.add`` for all ridges, then per ridge ``factor`` + ``loo``; no row is held
    out.  A system ``factor`` refuses gets ``inf``.  Host reads: those of ``factor`` per ridge and one read of the path at the
    end.  Raises ``ValueError`` where no ridge gives a finite PRESS."""
    torch = _lib.require_gpu()
    ridges = tuple(float(r) for r in ridges)
    if not ridges or not all(r >= 0.0 for r in ridges):
        raise ValueError("select_ridge needs at least one ridge, none negative")
    ne = NormalEquations(net).add(params, x, y, batch_size=batch_size)
    O, dev = ne.O, ne.G.device
    inf_o = torch.full((O,), float("inf"), dtype=torch.float64, device=dev)
    fits, press, gcv, trace = [], [], [], []
    for r in ridges:
        try:
            fac = factor(ne, ridge=r, fit_bias=fit_bias)
        except ValueError:             # not positive definite, or non-finite entries: this ridge is out
            fits.append(None)
            press.append(inf_o)
            gcv.append(inf_o)
            trace.append(inf_o[0])
            continue
        res = loo(net, params, x, y, fac, batch_size=batch_size)
        fits.append(fac.fit)
        press.append(res.press)
        gcv.append(res.gcv)
        trace.append(res.trace)
    press, gcv, trace = finite_lists(torch.stack(press)), finite_lists(torch.stack(gcv)), finite_lists(torch.stack(trace))
    total = [float(np.sum(p)) for p in press]
    best = min(range(len(ridges)), key=lambda i: (total[i], ridges[i]))
    if fits[best] is None or not np.isfinite(total[best]):
        raise ValueError("select_ridge: no ridge gave a positive definite system with a finite PRESS")
    return RidgeSearch(ridges, press, gcv, trace, best, fits[best], with_fit(params, fits[best]))


def select_scale(net, widths, x, y, scales=(0.5, 1, 2, 4, 8), ridge: float = 1e-8, batch_size: int = 65536):
    """The leave-one-out counterpart of ``widths.select_scale``: the same net per scale s (``log_sigs = widths.scaled(s).log_sigs(net)``),
    but ALL rows fitted and priced by PRESS / (n O) -- one Gram pass and one K11 pass per scale where the hold-out search gives up a
    fifth of the table and runs two Gram passes.  -> ``widths.ScaleSearch`` with ``train_mse`` = rss / (n O) and ``holdout_mse``
    holding the leave-one-out MSE; a scale whose system is refused gets ``inf``."""
    torch = _lib.require_gpu()
    xd = to_device_f32(x, torch)
    yd = to_device_f32(y, torch, device=xd.device)
    N, O = xd.shape[0], net.out_features
    if N < 1:
        raise ValueError("select_scale needs rows")

    def press(net_s, p, ne):
        fac = factor(ne, ridge=ridge)
        return fac.fit, loo(net_s, p, xd, yd, fac, batch_size=batch_size).press.sum() / (N * O)
    return search_scales(net, widths, xd, yd, scales, batch_size, press, "leave-one-out error")
