"""CPU checks of OLS forward selection: the float64 statement the GPU tests are written against (tests/_ols_util.py: ols_ref) against
the independent lstsq statement, the condition those tests rely on (no near-tie among the scores), the argument validation of the
C entry points (decided before any HIP call) and the slicing of nets, trees and accumulators."""
import ctypes as C

import numpy as np
import pytest
import torch

import _linear_fit_util as lu
import _ols_util as ou
import _widths_util as wu
from irbfn_amd import _lib, linear_fit, ols
from irbfn_amd.model import ClusterWCRBFNet, DeeperWCRBFNet, WCRBFNet


@pytest.mark.parametrize("case", ou.CASES, ids=lambda c: "N%d-M%d-O%d-K%d" % c)
def test_the_gram_statement_agrees_with_lstsq(case):
    N, M, O, K = case
    H, Y, G = ou.case(N, M, O)
    lam = ou.lam_of(G, M)
    r = ou.ols_ref(G, M, O, K)
    sel, gain, obj, best, second = ou.lstsq_path(H, Y, lam, True, K)
    assert r["count"] == K + 1 and r["sel"][0] == M
    dg, do = ou.rel_entries(r["gain"][1:].sum(1), gain.sum(1)), ou.rel_entries(r["objective"][1:], obj)
    gap_ref = float(((r["best"][1:] - r["second"][1:]) / r["best"][1:]).min())
    gap_ls = float(((best - second) / best).min())
    mg, mo = ou.rel(r["gain"][1:], gain), ou.rel(r["objective"][1:], obj)
    print(f"N={N} M={M} O={O} K={K}: step gain {dg:.2e} objective {do:.2e} relative (of the largest entry: {mg:.2e}, {mo:.2e}); "
          f"smallest relative gap between the two best "
          f"scores {gap_ref:.2e} (Gram form) {gap_ls:.2e} (lstsq); cond(H) {np.linalg.cond(H):.2e}")
    assert np.array_equal(r["sel"][1:], sel)
    assert max(dg, do) <= ou.TOL                                      # 16 times the largest figure printed above
    assert gap_ref > ou.GAP and gap_ls > ou.GAP                       # the condition of the GPU tests' index equality
    # the path is what solve reaches: the objective of the full prefix against NormalEquations.solve's own arithmetic
    sol = wu.solve_ref(H[:, sel], Y, ou.RIDGE * np.trace(G[:M, :M]) / M * K / np.trace(H[:, sel].T @ H[:, sel]))
    res = np.hstack([H[:, sel], np.ones((N, 1))]) @ sol - Y
    want = (res ** 2).sum(0) + lam * (sol[:K] ** 2).sum(0)
    assert np.abs(r["objective"][-1] - want).max() <= ou.TOL * np.diagonal(G)[M + 1:].max()


def test_without_the_ones_column_and_on_a_dependent_pool():
    H, Y, G = ou.case(300, 40, 2)
    lam = ou.lam_of(G, 40)
    r = ou.ols_ref(G, 40, 2, 12, fit_bias=False)
    sel, gain, obj, _, _ = ou.lstsq_path(H, Y, lam, False, 12)
    assert np.array_equal(r["sel"], sel)
    assert ou.rel_entries(r["gain"].sum(1), gain.sum(1)) <= ou.TOL and ou.rel_entries(r["objective"], obj) <= ou.TOL
    # a pool of rank 5 without a ridge: five pivots, then nothing qualifies
    rng = np.random.default_rng(1)
    Hr = (rng.integers(-3, 4, size=(60, 5)) @ rng.integers(-2, 3, size=(5, 12))).astype(np.float64)
    Yr = rng.integers(-3, 4, size=(60, 1)).astype(np.float64)
    rr = ou.ols_ref(lu.stacked_gram(Hr, Yr), 12, 1, 12, fit_bias=False, lam=0.0)
    assert rr["count"] == 5 == np.linalg.matrix_rank(Hr)


def _host(n, dtype=C.c_double):
    return (dtype * n)()


def test_argument_validation_without_a_gpu():
    lib = _lib.load()
    M, O, k = 5, 2, 3
    need = lib.irbfn_ols_workspace_bytes(M, O, k)
    assert need > 0 and need % 4 == 0
    assert lib.irbfn_ols_workspace_bytes(8000, 10, 1000) > lib.irbfn_ols_workspace_bytes(8000, 10, 999) > need
    for bad in ((0, 1, 1), (5, 0, 1), (5, 1, 0), (5, 1, 6), (8190, 2, 1), (-1, 1, 1)):
        assert lib.irbfn_ols_workspace_bytes(*bad) == -1, bad
    assert lib.irbfn_ols_workspace_bytes(8190, 1, 8190) > 0
    # host buffers stand in for device ones: every call below is refused before anything could read them
    n = ou.npad(M)
    g, l, d, c, gain = _host(64), _host((k + 1) * n), _host(2 * n), _host(n * O), _host((k + 1) * O)
    sel, count, ws = _host(k + 1, C.c_int32), _host(1, C.c_int32), _host(need // 8 + 2)
    p = lambda b: C.cast(b, C.c_void_p)                               # noqa: E731
    bufs = [p(l), p(d), p(c), p(sel), p(gain), p(count), p(ws)]

    def begin(g_=p(g), M_=M, O_=O, ridge=0.0, tol=1e-13, k_=k, bufs_=bufs, nbytes=need):
        return lib.irbfn_ols_begin(g_, M_, O_, 1, ridge, tol, k_, *bufs_, nbytes, None)

    def steps(g_=p(g), M_=M, O_=O, tol=1e-13, k_=k, bufs_=bufs, nbytes=need, steps_=1):
        return lib.irbfn_ols_steps(g_, M_, O_, 1, tol, k_, *bufs_, nbytes, steps_, None)

    assert steps(steps_=0) == 0                                       # no launch
    for call in (begin, steps):
        assert call(g_=None) == -1
        for i in range(7):
            assert call(bufs_=bufs[:i] + [None] + bufs[i + 1:]) == -1, i
        assert call(M_=0) == -1 and call(O_=0) == -1 and call(k_=0) == -1 and call(k_=M + 1) == -1 and call(M_=8190, O_=2) == -1
        assert call(tol=float("nan")) == -1 and call(tol=-1e-3) == -1
        assert call(nbytes=need - 1) == -1
        assert call(bufs_=bufs[:6] + [C.c_void_p(p(ws).value + 4)]) == -1          # misaligned
    assert begin(ridge=-1.0) == -1 and begin(ridge=float("nan")) == -1
    assert steps(steps_=-1) == -1


def _cfg(K, R=1, O=2):
    if R == 1:
        return wu.e2e_cfg(K=K, O=O)
    return dict(in_features=3, out_features=O, num_kernels=K, basis_func="gaussian", num_regions=4, lower_bounds=[[0.0, 2.0]] * 2,
                upper_bounds=[[2.0, 4.0]] * 2, dimension_ranges=[[0, 0], [0, 1], [1, 0], [1, 1]], activation_idx=[0, 1], delta=[5.0, 5.0])


def test_slice_net_free_frozen_and_gated():
    rng = np.random.default_rng(0)
    idx = np.array([5, 0, 3])
    for R in (1, 4):
        cfg = _cfg(7, R)
        centers = rng.normal(size=(R, 7, 3)).astype(np.float32)
        ls = rng.normal(size=(R, 7))
        free = WCRBFNet(**cfg)
        tree = free.init(seed=1)
        tree["params"]["rbf_list"]["log_sigs"] = ls.astype(np.float32)
        net_k, new = ols.slice_net(free, tree, idx)
        assert net_k.num_kernels == 3 and net_k.num_regions == R and net_k.frozen == ()
        assert np.array_equal(new["rbf_list"]["centers"], tree["params"]["rbf_list"]["centers"][:, idx])
        assert np.array_equal(new["rbf_list"]["log_sigs"], ls.astype(np.float32)[:, idx])
        assert np.array_equal(new["linear"]["kernel"], tree["params"]["linear"]["kernel"][idx])
        net_k._check_shapes(new)
        assert tree["params"]["linear"]["kernel"].shape == (7, 2)     # the input tree is left as it was
        fc = WCRBFNet(**cfg, centers=centers, fixed_centers=True)
        net_k, new = ols.slice_net(fc, fc.init(), idx)
        assert net_k.frozen == ("centers",) and np.array_equal(net_k.centers, centers[:, idx]) and set(new["rbf_list"]) == {"log_sigs"}
        net_k._check_shapes(new)
        fw = WCRBFNet(**cfg, centers=centers, fixed_width=True, log_sigs=ls)
        net_k, new = ols.slice_net(fw, fw.init(), idx)
        assert net_k.frozen == ("centers", "log_sigs") and set(new) == {"linear"}
        assert np.array_equal(net_k.centers, centers[:, idx]) and np.array_equal(net_k.log_sigs, ls[:, idx])
        net_k._check_shapes(new)
        t = {"linear": {k: torch.from_numpy(v) for k, v in fw.init()["params"]["linear"].items()}}     # torch leaves, no wrapper
        _, newt = ols.slice_net(fw, t, idx)
        assert torch.equal(newt["linear"]["kernel"], t["linear"]["kernel"][idx])
    with pytest.raises(ValueError):
        ols.slice_net(free, tree, [7])
    with pytest.raises(ValueError):
        ols.slice_net(free, tree, [])
    with pytest.raises(ValueError, match="use_float64"):
        ols.slice_net(WCRBFNet(**_cfg(7), use_float64=True), tree, idx)
    for cls in (DeeperWCRBFNet, ClusterWCRBFNet):
        with pytest.raises(ValueError, match=cls.__name__):
            ols.slice_net(cls.__new__(cls), tree, idx)


def test_subset_and_subnet_on_a_host_accumulator():
    N, M, O, K = ou.CASES[0]
    H, Y, G = ou.case(N, M, O)
    r = ou.ols_ref(G, M, O, K)
    ne = linear_fit.NormalEquations(lu.Shape(M, O), G=torch.from_numpy(np.array(G)))
    idx = r["sel"][1:]
    sub = ne.subset(idx[:5], lu.Shape(5, O))
    full = np.concatenate([idx[:5], np.arange(M, M + 1 + O)])
    assert np.array_equal(sub.G.numpy(), G[np.ix_(full, full)]) and (sub.K, sub.O) == (5, O) and sub.G.is_contiguous()
    assert np.abs(sub.G.numpy() - lu.stacked_gram(H[:, idx[:5]], Y)).max() <= 1e-13 * np.abs(G).max()
    with pytest.raises(ValueError):
        ne.subset(idx[:5], lu.Shape(4, O))
    with pytest.raises(ValueError):
        ne.subset([0, M], lu.Shape(2, O))
    with pytest.raises(ValueError):
        linear_fit.NormalEquations(lu.Shape(M, O)).subset([0], lu.Shape(1, O))
    # subnet: the first k of the selection, the linear leaves from solve on the subset
    net = WCRBFNet(**wu.e2e_cfg(K=M, O=O))
    yty = np.diagonal(G)[M + 1:]
    res = ols.OLSResult(ne, torch.from_numpy(idx.copy()), torch.from_numpy(r["gain"][1:]),
                        torch.from_numpy(r["objective"][1:]), ou.RIDGE, ou.lam_of(G, M), True)
    assert res.n_selected == K and tuple(res.objective.shape) == (K + 1, O)
    tree = net.init()
    net_k, params_k, fit = res.subnet(net, tree, k=5)
    assert net_k.num_kernels == 5 and params_k["params"]["linear"]["kernel"].shape == (5, O)
    W, b, rss = lu.lstsq_ref(H[:, idx[:5]], Y, fit.ridge_abs, True)
    assert np.abs(fit.kernel.numpy() - W).max() <= 1e-9 * np.abs(W).max() and np.abs(fit.bias.numpy() - b).max() <= 1e-9 * np.abs(W).max()
    assert np.array_equal(params_k["params"]["linear"]["kernel"], fit.kernel.numpy().astype(np.float32))
    assert np.array_equal(params_k["params"]["rbf_list"]["centers"], tree["params"]["rbf_list"]["centers"][:, idx[:5]])
    assert np.abs(fit.rss.numpy() - rss).max() <= 1e-9 * yty.max()
    with pytest.raises(ValueError):
        res.subnet(net, tree, k=K + 1)
    assert res.subnet(net, tree)[0].num_kernels == K


def test_select_has_no_cpu_fallback():
    ne = linear_fit.NormalEquations(lu.Shape(4, 1))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ols.select(ne, 2)
    else:
        with pytest.raises(ValueError, match="no rows"):
            ols.select(ne, 2)
