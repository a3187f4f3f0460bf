"""The leave-one-out pass on the GPU (run on the MI355X box with ``-m gpu``): irbfn_rows_quad_f64 through the C ABI on guarded
buffers, then ``loo.factor`` / ``loo`` / ``leverage`` / ``select_ridge`` / ``select_scale`` end to end against the float64 statement
of tests/_loo_util.py on the device's own hidden layer.

Kernel: integer z and p bit for bit against NumPy int64; normal z and p within (4 m + 8) 2^-53 sum_j (sum_k |z_k p_kj|)^2 of q and
(m + 1) 2^-53 sum_k |z_k p_ko| of v in ``np.longdouble``.  z carries NaN guard rows past `rows` and NaN guard columns in [m, ldz); p
carries NaN in its strict lower triangle, in the columns [m + nd, ldp) and behind its last row; q and v are prefilled with NaN and
carry guard elements behind them.

End to end: the device's solve is within SOLVE_RTOL = 1e-9 of the float64 one relative to the largest weight (the tolerance of
tests/test_gpu_linear_fit.py), so a prediction z sol is within SOLVE_RTOL max|sol| sum_k |z_k|, a leverage within the kernel's bound
plus SOLVE_RTOL of the largest leverage, and e / (1 - l) within what those two propagate to.

Largest err / bound measured (printed by the tests): float rows q 0.013 and v 0.15 (m = 17), q below 0.0005 and v 0.023 (m = 130); end
to end, err / tolerance: leverage 8.4e-7, residual 2.7e-6, leave-one-out residual 2.6e-6 on the 1500-row case (fit_bias and not), 4.0e-7 /
1.0e-6 / 9.8e-7 on the 7-centre OLS prefix, 1.8e-6 / 2.1e-7 / 2.2e-7 on the two-region net.  Times: profiles/loo.txt."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _linear_fit_util as lu
import _loo_util as lo
from irbfn_amd import _lib, linear_fit, loo, ols, widths
from irbfn_amd.model import WCRBFNet, _ptr, _stream_ptr

pytestmark = pytest.mark.gpu
GUARD = 3
OK, BAD_ARG = 0, -1
MS = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 130, 200)
ROWS = (1, 31, 33, 64, 65, 257)
NDS = (0, 1, 10, 17)
RIDGE = 1e-8
BLOCK_ROWS = 128                 # rows of z per block (kRqRows kRqRowTiles)
MAX_BLOCKS = 1 << 16             # blocks of a launch (kRqMaxBlocks): more row tiles are walked by a grid-stride loop


class Quad:
    """irbfn_rows_quad_f64 calls on guarded, prefilled buffers; (q, v) as NumPy arrays after every call."""

    def __init__(self, z, p, nd, pad_z=0, pad_p=0):
        self.lib = _lib.load()
        z = np.ascontiguousarray(z, np.float32)
        self.rows, self.m = z.shape
        self.nd, self.ldz, self.ldp = nd, self.m + pad_z, self.m + nd + pad_p
        assert p.shape == (self.m, self.m + nd)
        zg = np.full((self.rows + GUARD, self.ldz), np.nan, np.float32)
        zg[:self.rows, :self.m] = z
        pg = np.full((self.m + GUARD, self.ldp), np.nan, np.float64)
        pg[:self.m, :self.m + nd] = p
        self.zg, self.pg = torch.from_numpy(zg).cuda(), torch.from_numpy(pg).cuda()

    def run(self, row0=0, rows=None):
        rows = self.rows - row0 if rows is None else rows
        nd = self.nd
        q = torch.full((rows + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
        v = torch.full((rows * nd + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
        zp = C.c_void_p(self.zg.data_ptr() + 4 * row0 * self.ldz)
        st = self.lib.irbfn_rows_quad_f64(zp, self.ldz, rows, self.m, _ptr(self.pg), self.ldp, nd, _ptr(q), _ptr(v) if nd else None,
                                          _stream_ptr(torch))
        assert st == OK, st
        torch.cuda.synchronize()
        assert torch.isnan(q[rows:]).all() and torch.isnan(v[rows * nd:]).all()              # the guard zones are untouched
        return q[:rows].cpu().numpy(), v[:rows * nd].cpu().numpy().reshape(rows, nd)


@pytest.mark.parametrize("m", MS)
def test_integer_rows_are_exact(gpu, m):
    for i, nd in enumerate(NDS):
        z, p = lo.integer_case(max(ROWS), m, nd, seed=100 * m + nd)
        qi, vi = lo.quad_int(z, p)
        for j, rows in enumerate(ROWS):
            q, v = Quad(z[:rows], p, nd, pad_z=GUARD * ((i + j) % 2), pad_p=GUARD * (j % 2)).run()
            assert q.tobytes() == qi[:rows].tobytes(), (m, nd, rows)
            assert v.tobytes() == vi[:rows].tobytes(), (m, nd, rows)


@pytest.mark.parametrize("m,nd,rows", ((130, 10, 257), (17, 10, 257), (17, 0, 40)))
def test_float_rows_meet_the_any_order_bounds(gpu, m, nd, rows):
    z, p = lo.float_case(rows, m, nd, seed=m + nd)
    qr, vr, qb, vb = lo.quad_ref(z, p)
    run = Quad(z, p, nd, pad_z=1, pad_p=2)
    q, v = run.run()
    assert np.isfinite(q).all() and np.isfinite(v).all()                  # the NaN triangle reaches no output
    eq, ev = np.abs(q - qr).astype(np.float64), np.abs(v - vr).astype(np.float64)
    print(f"m={m} nd={nd} rows={rows}: largest err / bound q {float((eq / qb).max()):.3f}" + (f", v {float((ev / vb).max()):.3f}" if nd else ""))
    assert (eq <= qb).all() and (ev <= vb).all()
    q2, v2 = run.run()
    assert q2.tobytes() == q.tobytes() and v2.tobytes() == v.tobytes()    # a repeat is bit-identical


def test_rows_are_independent_of_their_call_and_their_neighbours(gpu):
    m, nd, rows = 130, 10, 257
    z, p = lo.float_case(rows, m, nd, seed=5)
    q, v = Quad(z, p, nd).run()
    # split at an odd offset: the same buffers, two calls
    run = Quad(z, p, nd, pad_z=2)
    qa, va = run.run(row0=0, rows=37)
    qb, vb = run.run(row0=37)
    assert np.concatenate([qa, qb]).tobytes() == q.tobytes() and np.vstack([va, vb]).tobytes() == v.tobytes()
    # permuted rows
    perm = np.random.default_rng(0).permutation(rows)
    qp, vp = Quad(z[perm], p, nd).run()
    assert qp.tobytes() == q[perm].tobytes() and vp.tobytes() == v[perm].tobytes()
    # nd does not touch q
    assert Quad(z, p[:, :m], 0).run()[0].tobytes() == q.tobytes()
    # one row of NaN and one of Inf: non-finite q for exactly those rows, every other row as before
    zn = z.copy()
    zn[70, :] = np.nan
    zn[200, :] = np.inf
    qn, vn = Quad(zn, p, nd).run()
    keep = np.ones(rows, bool)
    keep[[70, 200]] = False
    assert not np.isfinite(qn[[70, 200]]).any() and not np.isfinite(vn[[70, 200]]).any()
    assert qn[keep].tobytes() == q[keep].tobytes() and vn[keep].tobytes() == v[keep].tobytes()
    # a single NaN entry stays in its row as well
    zn = z.copy()
    zn[64, 129] = np.nan
    qn, vn = Quad(zn, p, nd).run()
    keep = np.arange(rows) != 64
    assert np.isnan(qn[64]) and qn[keep].tobytes() == q[keep].tobytes() and vn[keep].tobytes() == v[keep].tobytes()


def test_more_row_tiles_than_blocks_are_walked_by_the_grid_stride_loop(gpu):
    rows = MAX_BLOCKS * BLOCK_ROWS + BLOCK_ROWS + 2                       # every block takes a second tile or none, the last one ragged
    rng = np.random.default_rng(9)
    z = torch.from_numpy(rng.integers(-8, 9, size=(rows, 2)).astype(np.float32)).cuda()
    p = torch.tensor([[3.0, -2.0, 5.0], [float("nan"), 7.0, -4.0]], dtype=torch.float64, device="cuda")
    q, v = loo.rows_quad(z, p, 1)
    z64 = z.to(torch.float64)
    assert torch.equal(q, (3.0 * z64[:, 0]) ** 2 + (-2.0 * z64[:, 0] + 7.0 * z64[:, 1]) ** 2)
    assert torch.equal(v[:, 0], 5.0 * z64[:, 0] - 4.0 * z64[:, 1])


def test_refusals_launch_nothing_and_the_wrapper(gpu):
    lib = _lib.load()
    z = torch.ones((8, 20), dtype=torch.float32, device="cuda")
    p = torch.ones((17, 30), dtype=torch.float64, device="cuda")
    q = torch.full((8,), float("nan"), dtype=torch.float64, device="cuda")
    v = torch.full((80,), float("nan"), dtype=torch.float64, device="cuda")

    def call(m=17, ldz=20, ldp=30, nd=10, rows=8, vp=_ptr(v)):
        return lib.irbfn_rows_quad_f64(_ptr(z), ldz, rows, m, _ptr(p), ldp, nd, _ptr(q), vp, _stream_ptr(torch))
    assert call(m=0) == BAD_ARG and call(m=8193, ldz=9000, ldp=9000) == BAD_ARG and call(ldz=16) == BAD_ARG
    assert call(ldp=26) == BAD_ARG and call(nd=-1) == BAD_ARG and call(vp=None) == BAD_ARG and call(rows=0) == OK
    torch.cuda.synchronize()
    assert torch.isnan(q).all() and torch.isnan(v).all()
    assert call() == OK
    torch.cuda.synchronize()
    tri = sum((j + 1) ** 2 for j in range(17))
    assert (q == tri).all() and (v == 17).all()
    # the wrapper: a strided view of z and of P is read in place
    zi, pi = lo.integer_case(70, 21, 4, seed=3)
    qi, vi = lo.quad_int(zi, pi)
    wide = torch.full((70, 30), float("nan"), dtype=torch.float32, device="cuda")
    wide[:, :21] = torch.from_numpy(zi).cuda()
    P = torch.from_numpy(pi).cuda()
    qw, vw = loo.rows_quad(wide[:, :21], P, 4)
    assert qw.dtype == torch.float64 and qw.cpu().numpy().tobytes() == qi.tobytes() and vw.cpu().numpy().tobytes() == vi.tobytes()
    q0, v0 = loo.rows_quad(torch.from_numpy(zi).cuda(), P[:, :21], 0)
    assert q0.cpu().numpy().tobytes() == qi.tobytes() and tuple(v0.shape) == (70, 0)
    qe, ve = loo.rows_quad(torch.zeros((0, 21), dtype=torch.float32, device="cuda"), P, 4)
    assert tuple(qe.shape) == (0,) and tuple(ve.shape) == (0, 4)
    with pytest.raises(ValueError):
        loo.rows_quad(wide[:, :21], P, 3)
    with pytest.raises(ValueError):
        loo.rows_quad(wide[:, :21], P.float(), 4)


# ------------------------------------------------------------------ end to end
def _fit_net(frozen=False, log_sigs=True):
    cfg, centers, log_sigs_, x, y, h64, gsum = lu.fit_case()
    if frozen:
        extra = dict(log_sigs=log_sigs_[None].tolist()) if log_sigs else {}
        net = WCRBFNet.from_config(dict(cfg, fixed_centers=True, fixed_width=True, **extra), centers=centers)
        return net, net.init()
    net = WCRBFNet.from_config(cfg)
    p = net.init()
    p["params"]["rbf_list"]["centers"] = centers[None].copy()
    p["params"]["rbf_list"]["log_sigs"] = log_sigs_[None].copy()
    return net, p


def hold_to_statement(net, params, x, y, fac, res, lev=None):
    """``loo(per_row=True)`` against the statement on the device's own hidden layer at the factor's absolute ridge."""
    y64 = np.asarray(y, np.float32).astype(np.float64)
    h = net.hidden(params, x)
    st = lo.statement(h.astype(np.float64), y64, fac.ridge_abs, fac.fit_bias)
    assert st["cond"] < 1e3                                               # a condition on the input: SOLVE_RTOL rests on it
    Z = lo.design(h.astype(np.float64), fac.fit_bias)
    n, m = Z.shape
    T = fac.P[:, :m].cpu().numpy().T
    q, e, le = res.leverage.cpu().numpy(), res.residual.cpu().numpy(), res.loo_residual.cpu().numpy()
    tq = lo.leverage_bound(Z, T) + lo.SOLVE_RTOL * st["leverage"].max()
    te = lo.SOLVE_RTOL * np.abs(st["sol"]).max() * np.abs(Z).sum(1)[:, None] + (m + 1) * lo.U53 * (np.abs(Z) @ np.abs(st["sol"]))
    d = 1.0 - st["leverage"]
    tl = te / d[:, None] + np.abs(st["residual"]) * (tq / d ** 2)[:, None]
    worst = [float((np.abs(a - b) / t).max()) for a, b, t in ((q, st["leverage"], tq), (e, st["residual"], te), (le, st["loo_residual"], 1.01 * tl))]
    print(f"loo n={n} m={m}: largest err / tolerance: leverage {worst[0]:.2e}, residual {worst[1]:.2e}, loo residual {worst[2]:.2e}; "
          f"trace {float(res.trace):.6f}, press / rss {float(res.press.sum() / res.rss.sum()):.4f}")
    assert max(worst) <= 1.0, worst
    assert res.n == n and int(res.n_degenerate) == 0
    assert abs(float(res.trace) - st["trace"]) <= tq.sum()
    assert (np.abs(res.rss.cpu().numpy() - st["rss"]) <= (2 * np.abs(st["residual"]) * te + te ** 2).sum(0)).all()
    assert (np.abs(res.press.cpu().numpy() - st["press"]) <= 1.01 * (2 * np.abs(st["loo_residual"]) * tl + tl ** 2).sum(0)).all()
    gcv = n * res.rss.cpu().numpy() / (n - float(res.trace)) ** 2        # of its own rss and trace, which are held above
    assert np.abs(res.gcv.cpu().numpy() - gcv).max() <= 1e-14 * gcv.max()
    assert int(res.max_leverage_row) == int(np.argmax(q)) and float(res.max_leverage) == q.max()
    assert bool((res.press >= res.rss).all())
    return st


def test_factor_is_solve_bit_for_bit(gpu):
    cfg, centers, log_sigs, x, y, h64, gsum = lu.fit_case()
    net, p = _fit_net()
    ne = linear_fit.NormalEquations(net).add(p, x, y, batch_size=512)
    for ridge, fit_bias in ((RIDGE, True), (1e-2, False)):
        fac, fit = loo.factor(ne, ridge=ridge, fit_bias=fit_bias), ne.solve(ridge=ridge, fit_bias=fit_bias)
        assert torch.equal(fac.fit.kernel, fit.kernel) and torch.equal(fac.fit.bias, fit.bias) and torch.equal(fac.fit.rss, fit.rss)
        assert fac.fit.ridge_abs == fit.ridge_abs and fac.n == fit.n == 1500 and fac.P.is_cuda
        assert torch.equal(ne.rss_of(fac.fit), fac.fit.rss)


@pytest.mark.parametrize("fit_bias", (True, False))
def test_loo_meets_the_statement_on_the_devices_hidden_layer(gpu, fit_bias):
    cfg, centers, log_sigs, x, y, h64, gsum = lu.fit_case()
    net, p = _fit_net()
    ne = linear_fit.NormalEquations(net).add(p, x, y, batch_size=512)
    fac = loo.factor(ne, ridge=RIDGE, fit_bias=fit_bias)
    res = loo.loo(net, p, x, y, fac, batch_size=97, per_row=True)         # 15 chunks of 97 and one of 45
    hold_to_statement(net, p, x, y, fac, res)
    # the trace from G alone, and the rows' rss against the rss from G
    tr = lo.trace_from_gram(ne.G.cpu().numpy(), 48, fac.ridge_abs, fit_bias)
    Z = lo.design(net.hidden(p, x).astype(np.float64), fit_bias)
    assert abs(float(res.trace) - tr) <= lo.leverage_bound(Z, fac.P[:, :fac.m].cpu().numpy().T).sum() + lo.SOLVE_RTOL * fac.m
    y64 = y.astype(np.float64)
    assert (np.abs(res.rss.cpu().numpy() - fac.fit.rss.cpu().numpy()) <= 1e-9 * (y64 ** 2).sum(0)).all()
    # without per_row the sums are the same bits; leverage() needs no labels and gives the same bits, however the rows are cut
    plain = loo.loo(net, p, x, y, fac, batch_size=97)
    assert plain.leverage is None and plain.residual is None and plain.loo_residual is None
    assert torch.equal(plain.press, res.press) and torch.equal(plain.rss, res.rss) and torch.equal(plain.trace, res.trace)
    assert torch.equal(loo.leverage(net, p, x, fac, batch_size=97), res.leverage)
    assert torch.equal(loo.leverage(net, p, torch.from_numpy(x.copy()).cuda(), fac, batch_size=1000), res.leverage)
    # the linear leaves of params are not read: v comes from the factor
    junk = {"params": {"rbf_list": p["params"]["rbf_list"], "linear": {"kernel": np.full((48, 3), 7.0, np.float32), "bias": np.ones(3, np.float32)}}}
    assert torch.equal(loo.loo(net, junk, x, y, fac, batch_size=97).press, res.press)


def test_degenerate_rows_and_refusals(gpu):
    cfg, centers, log_sigs, x, y, h64, gsum = lu.fit_case()
    net, p = _fit_net()
    fac = loo.factor(linear_fit.NormalEquations(net).add(p, x, y), ridge=RIDGE)
    xn = x[:200].copy()
    xn[17, 1] = np.nan
    res = loo.loo(net, p, xn, y[:200], fac, batch_size=97, per_row=True)
    assert int(res.n_degenerate) == 1 and bool(torch.isinf(res.press).all()) and bool(torch.isinf(res.loo_residual[17]).all())
    keep = np.arange(200) != 17
    good = loo.loo(net, p, x[:200], y[:200], fac, batch_size=97, per_row=True)
    assert torch.equal(res.leverage[keep], good.leverage[keep]) and torch.equal(res.loo_residual[keep], good.loo_residual[keep])
    lev = res.leverage.cpu().numpy()
    assert int(res.max_leverage_row) == int(np.argmax(np.where(np.isfinite(lev), lev, -np.inf))) != 17
    with pytest.raises(ValueError, match="rows"):
        loo.loo(net, p, x[:100], y[:99], fac)
    with pytest.raises(ValueError):
        loo.loo(net, p, x[:, :2], y, fac)
    with pytest.raises(ValueError):
        loo.loo(net, p, x, y[:, :2], fac)
    with pytest.raises(ValueError, match="columns"):
        loo.leverage(net, p, x, loo.Factor(fac.L, fac.s, fac.ridge_abs, fac.n, False, fac.fit, fac.P))     # 49 columns, no bias
    with pytest.raises(ValueError, match="float64"):
        loo.leverage(WCRBFNet.from_config(cfg, use_float64=True), p, x, fac)


def test_select_ridge_is_the_argmin_of_its_own_path(gpu):
    cfg, centers, log_sigs, x, y, h64, gsum = lu.fit_case()
    net, p = _fit_net()
    ridges = (1e-10, 1e-8, 1e-4, 1e-1)
    search = loo.select_ridge(net, p, x, y, ridges=ridges, batch_size=512)
    ne = linear_fit.NormalEquations(net).add(p, x, y, batch_size=512)
    for i, r in enumerate(ridges):
        fac = loo.factor(ne, ridge=r)
        res = loo.loo(net, p, x, y, fac, batch_size=512)
        assert search.press[i] == res.press.tolist() and search.gcv[i] == res.gcv.tolist() and search.trace[i] == float(res.trace)
    total = [sum(v) for v in search.press]
    assert search.best == int(np.argmin(total)) and search.best_ridge == ridges[search.best]
    assert total[3] > total[search.best] and search.trace[3] < search.trace[0]               # a heavy ridge costs, and shrinks the trace
    want = ne.solve(ridge=search.best_ridge)
    assert torch.equal(search.fit.kernel, want.kernel) and torch.equal(search.fit.bias, want.bias)
    lin = search.params["params"]["linear"]
    assert lin["kernel"].dtype == np.float32 and np.array_equal(lin["kernel"], want.kernel.cpu().numpy().astype(np.float32))
    assert np.array_equal(lin["bias"], want.bias.cpu().numpy().astype(np.float32))
    assert search.params["params"]["rbf_list"]["centers"] is p["params"]["rbf_list"]["centers"]


def test_select_ridge_refuses_a_singular_system_as_inf(gpu):
    cfg, centers, log_sigs, x, y, h64, gsum = lu.fit_case()
    net, p = _fit_net()
    c, ls = centers[None].copy(), log_sigs[None].copy()
    c[0, 5], ls[0, 5] = c[0, 2], ls[0, 2]                                 # a duplicated centre: two bit-equal columns
    p["params"]["rbf_list"]["centers"], p["params"]["rbf_list"]["log_sigs"] = c, ls
    search = loo.select_ridge(net, p, x, y, ridges=(0.0, 1e-6))
    assert all(np.isinf(v) for v in search.press[0]) and np.isinf(search.trace[0]) and search.best == 1
    assert np.isfinite(search.press[1]).all() and search.fit.ridge_abs > 0
    with pytest.raises(ValueError, match="no ridge"):
        loo.select_ridge(net, p, x, y, ridges=(0.0,))


def test_select_scale_is_the_argmin_of_its_own_path(gpu):
    cfg, centers, log_sigs, x, y, h64, gsum = lu.fit_case()
    net0, _ = _fit_net(frozen=True, log_sigs=False)
    w = widths.nearest_neighbour(centers, p=2)
    search = loo.select_scale(net0, w, x, y, scales=(0.25, 0.5, 1, 2), batch_size=512)
    assert isinstance(search, widths.ScaleSearch) and len(search.holdout_mse) == 4
    assert search.best == int(np.argmin(search.holdout_mse)) and np.isfinite(search.holdout_mse[search.best])
    want = np.log(w.sigma.cpu().numpy().astype(np.float64) * search.best_scale).astype(np.float32)
    assert np.array_equal(search.net.log_sigs[0], want)
    # its params reproduce the fit: the same net fitted directly, and the fit's rss priced from the rows
    again, fit = linear_fit.fit_linear(search.net, search.net.init(), x, y, batch_size=512)
    assert torch.equal(fit.kernel, search.fit.kernel) and torch.equal(fit.rss, search.fit.rss)
    assert np.array_equal(again["params"]["linear"]["kernel"], search.params["params"]["linear"]["kernel"])
    assert np.array_equal(again["params"]["linear"]["bias"], search.params["params"]["linear"]["bias"])
    assert search.train_mse[search.best] == pytest.approx(search.fit.mse, rel=1e-12)
    fac = loo.factor(linear_fit.NormalEquations(search.net).add(search.params, x, y, batch_size=512))
    assert loo.loo(search.net, search.params, x, y, fac, batch_size=512).press_mse == pytest.approx(search.holdout_mse[search.best], rel=1e-12)
    with pytest.raises(ValueError, match="fixed-width"):
        loo.select_scale(_fit_net()[0], w, x, y)


def test_an_ols_prefix_is_priced_by_loo(gpu):
    cfg, centers, log_sigs, x, y, h64, gsum = lu.fit_case()
    net, p = _fit_net(frozen=True)
    ne = linear_fit.NormalEquations(net).add(p, x, y)
    sel = ols.select(ne, 16)
    net_k, p_k, fit_k = sel.subnet(net, p, 7)
    fac = loo.factor(ne.subset(sel.indices[:7], net_k), ridge=sel.ridge)
    assert torch.equal(fac.fit.kernel, fit_k.kernel) and fac.m == 8
    res = loo.loo(net_k, p_k, x, y, fac, batch_size=97, per_row=True)
    hold_to_statement(net_k, p_k, x, y, fac, res)
    full = loo.loo(net, p, x, y, loo.factor(ne), batch_size=512)
    assert float(res.press.sum()) > float(full.press.sum())                                  # 7 centres explain less than 48


@functools.lru_cache(maxsize=None)
def _two_regions():
    """D = 3, K = 12, O = 2, two regions gated by tanh on dimension 0 ([0, 2] and [2, 4], delta = 5); 300 rows in [0.2, 3.8]^3."""
    rng = np.random.default_rng(21)
    cfg = dict(in_features=3, out_features=2, num_kernels=12, basis_func="gaussian", num_regions=2, lower_bounds=[[0.0, 2.0]],
               upper_bounds=[[2.0, 4.0]], dimension_ranges=[[0], [1]], activation_idx=[0], delta=[5.0])
    centers = rng.uniform(0.3, 3.7, size=(2, 12, 3)).astype(np.float32)
    log_sigs = np.log(rng.uniform(0.8, 1.3, size=(2, 12))).astype(np.float32)
    x = rng.uniform(0.2, 3.8, size=(300, 3)).astype(np.float32)
    y = (np.stack([np.sin(x[:, 0]) * x[:, 1], np.cos(x[:, 2]) + 0.3 * x[:, 0]], 1) + 0.05 * rng.normal(size=(300, 2))).astype(np.float32)
    return cfg, centers, log_sigs, x, y


def test_loo_of_a_two_region_gated_net(gpu):
    cfg, centers, log_sigs, x, y = _two_regions()
    net = WCRBFNet.from_config(cfg)
    p = net.init()
    p["params"]["rbf_list"]["centers"], p["params"]["rbf_list"]["log_sigs"] = centers.copy(), log_sigs.copy()
    fac = loo.factor(linear_fit.NormalEquations(net).add(p, x, y, batch_size=97), ridge=1e-6)
    res = loo.loo(net, p, x, y, fac, batch_size=97, per_row=True)
    hold_to_statement(net, p, x, y, fac, res)


# ------------------------------------------------------------------ the shared pass over the rows
@functools.lru_cache(maxsize=None)
def _tiny():
    """K = 4, D = 3, O = 2, gaussian, one region: (net, params, 5 rows x, y, a factor with the ones column and one without)."""
    rng = np.random.default_rng(3)
    net = WCRBFNet.from_config(lu.synthetic_cfg(3, 4, "gaussian"))
    p = net.init()
    p["params"]["rbf_list"]["centers"] = rng.uniform(0.5, 3.5, size=(1, 4, 3)).astype(np.float32)
    p["params"]["rbf_list"]["log_sigs"] = rng.uniform(0.0, 1.0, size=(1, 4)).astype(np.float32)
    xs = rng.uniform(0.3, 3.7, size=(40, 3)).astype(np.float32)           # the rows the factors are solved on
    ne = linear_fit.NormalEquations(net).add(p, xs, rng.normal(size=(40, 2)).astype(np.float32))
    x, y = rng.uniform(0.3, 3.7, size=(5, 3)).astype(np.float32), rng.normal(size=(5, 2)).astype(np.float32)
    return net, p, x, y, loo.factor(ne, ridge=1e-6), loo.factor(ne, ridge=1e-6, fit_bias=False)


def test_the_shared_row_pass_at_its_edges(gpu):
    """N = 0, 1, 5 in chunks of 1, 2, 5, 8 through ``NormalEquations.add`` and ``loo.leverage``: one answer however the rows are
    cut, nothing for no rows, and no ones column for a factor without one."""
    net, p, x, y, fac, flat = _tiny()
    assert (fac.m, flat.m, fac.O) == (5, 4, 2)
    h = net.hidden(p, x)
    Z32 = np.hstack([h, np.ones((5, 1), np.float32), y])
    for N in (0, 1, 5):
        Gs, levs, flats = [], [], []
        for bs in (1, 2, 5, 8):
            ne = linear_fit.NormalEquations(net).add(p, x[:N], y[:N], batch_size=bs)
            assert tuple(ne.G.shape) == (7, 7) and ne.G.dtype == torch.float64 and ne.G.is_cuda
            Gs.append(ne.G)
            levs.append(loo.leverage(net, p, x[:N], fac, batch_size=bs))
            flats.append(loo.leverage(net, p, x[:N], flat, batch_size=bs))
            assert tuple(levs[-1].shape) == tuple(flats[-1].shape) == (N,) and levs[-1].dtype == torch.float64
        print(f"N = {N}: largest |G - G(batch_size=1)| over the batch sizes {max(float((G - Gs[0]).abs().max()) for G in Gs):.3e}")
        assert all(torch.equal(G, Gs[0]) for G in Gs) and all(torch.equal(q, levs[0]) for q in levs) and all(torch.equal(q, flats[0]) for q in flats)
        if N == 0:
            assert not bool(Gs[0].any())                                  # no rows: G stays at zero, and an empty leverage tensor
            continue
        z = Z32[:N].astype(np.float64)
        assert (np.abs(Gs[0].cpu().numpy() - z.T @ z) <= lu.gram_bound(Z32[:N])).all()
        for f, q in ((fac, levs[0]), (flat, flats[0])):                   # flat: z = h alone, column K is never written
            m = f.m
            U = f.P[:, :m].cpu().numpy()                                  # (L^-1 diag(s))^T, upper triangular
            ref = ((z[:, :m] @ np.triu(U)) ** 2).sum(1)
            assert (np.abs(q.cpu().numpy() - ref) <= lo.leverage_bound(z[:, :m], U.T) + 1e-15 * ref).all()
