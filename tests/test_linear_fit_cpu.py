"""CPU checks of the closed-form output-layer fit (irbfn_amd/linear_fit.py, irbfn_net_hidden, irbfn_syrk_f64): the ABI plumbing
and the refusals decided before any HIP call, ``NormalEquations.solve`` on CPU tensors against ``numpy.linalg.lstsq`` of the
stacked system, its refusals, ``merge``, and the margins of the cases the GPU tests rely on (tests/_linear_fit_util.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _linear_fit_util as lu
from irbfn_amd import _lib, build, linear_fit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("irbfn_net_hidden", "irbfn_syrk_f64_workspace_bytes", "irbfn_syrk_f64")
OK, BAD_ARG = 0, -1


def test_new_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "irbfn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} not declared in include/irbfn_hip.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _lib.SIGNATURES
    assert lib.irbfn_abi_version() == 1
    for src, obj in (("rbf_hidden.hip", "rbf_hidden.o"), ("syrk_f64.hip", "syrk_f64.o")):
        assert any(u[0] == src and u[1] == obj for u in build.UNITS)
    assert "no counterpart" in hdr[hdr.index("Closed-form fit of the output layer"):]


def test_status_table_without_gpu():
    lib = _lib.load()
    one = C.c_void_p(8)                  # a non-null, 8-byte aligned pointer that is never dereferenced: every call stops earlier
    good = dict(z=one, ldz=20, rows=100, M=17, g=one, acc=0, ws=one, nbytes=1 << 40)

    def call(**kw):
        a = dict(good, **kw)
        return lib.irbfn_syrk_f64(a["z"], a["ldz"], a["rows"], a["M"], a["g"], a["acc"], a["ws"], a["nbytes"], None)
    assert call(M=0) == BAD_ARG and call(M=-3) == BAD_ARG and call(M=8193, ldz=9000) == BAD_ARG
    assert call(ldz=16) == BAD_ARG and call(rows=-1) == BAD_ARG
    assert call(z=None) == BAD_ARG and call(g=None) == BAD_ARG
    assert call(ws=None) == BAD_ARG and call(ws=C.c_void_p(12)) == BAD_ARG
    assert call(nbytes=lib.irbfn_syrk_f64_workspace_bytes(100, 17) - 1) == BAD_ARG
    assert call(rows=0, acc=1, z=None, ws=None, nbytes=0) == OK          # nothing to add: no launch, no pointer needed
    assert call(rows=0, acc=1, g=None) == BAD_ARG
    # the hidden layer: a NULL net and a negative B are refused before anything is read
    assert lib.irbfn_net_hidden(None, one, one, 8, 4, None) == BAD_ARG


def test_workspace_bytes():
    w = _lib.load().irbfn_syrk_f64_workspace_bytes
    assert w(0, 5) == 0 and w(-1, 5) == BAD_ARG and w(10, 0) == BAD_ARG and w(10, 8193) == BAD_ARG
    tile = 64 * 64 * 8
    assert w(1, 1) == tile and w(256, 64) == tile and w(257, 64) == 2 * tile and w(1000, 17) == 4 * tile
    assert w(1000, 65) == 3 * 4 * tile                                   # three tile pairs
    for M in (1, 64, 1011, 4107, 8192):
        by_rows = [w(n, M) for n in (1, 1000, 65536, 1 << 20, 1 << 33)]
        assert all(v > 0 and v % 8 == 0 and v < 1 << 30 for v in by_rows), (M, by_rows)
        T = (M + 63) // 64
        assert max(by_rows) <= (T * (T + 1) // 2 + 4096) * tile          # fewer slabs for a large M


# ------------------------------------------------------------------ the solve
def _system(seed=0, n=500, K=12, O=3):
    rng = np.random.default_rng(seed)
    Zh = rng.normal(size=(n, K)) + 0.3
    Y = Zh @ rng.normal(size=(K, O)) + 0.7 + 0.1 * rng.normal(size=(n, O))
    return Zh, Y


@pytest.mark.parametrize("fit_bias", (True, False))
@pytest.mark.parametrize("ridge", (0.0, 1e-8, 1e-2))
def test_solve_matches_lstsq_of_the_stacked_system(ridge, fit_bias):
    Zh, Y = _system()
    n, K = Zh.shape
    O = Y.shape[1]
    assert np.linalg.cond(np.hstack([Zh, np.ones((n, 1))])) <= 100
    ne = linear_fit.NormalEquations(lu.Shape(K, O), G=torch.from_numpy(lu.stacked_gram(Zh, Y)))
    fit = ne.solve(ridge=ridge, fit_bias=fit_bias)
    lam = ridge * np.trace(Zh.T @ Zh) / K
    assert fit.ridge_abs == pytest.approx(lam, rel=1e-12) and fit.n == n
    W, b, rss = lu.lstsq_ref(Zh, Y, lam, fit_bias)
    assert fit.kernel.dtype == torch.float64 and tuple(fit.kernel.shape) == (K, O) and tuple(fit.bias.shape) == (O,)
    assert np.abs(fit.kernel.numpy() - W).max() <= 1e-10 * np.abs(W).max()
    if fit_bias:
        assert np.abs(fit.bias.numpy() - b).max() <= 1e-10 * np.abs(b).max()
    else:
        assert (fit.bias.numpy() == 0).all()
    assert (np.abs(fit.rss.numpy() - rss) <= 1e-9 * (Y ** 2).sum(0)).all()
    assert fit.mse == pytest.approx(rss.sum() / (n * O), rel=1e-6)
    if ridge == 1e-2:                    # the ridge is visible in the solution
        W0 = lu.lstsq_ref(Zh, Y, 0.0, fit_bias)[0]
        assert np.abs(fit.kernel.numpy() - W0).max() > 1e-4 * np.abs(W0).max()


def test_singular_system_is_refused_and_a_ridge_solves_it():
    Zh, Y = _system(1)
    Zh[:, 5] = Zh[:, 2]                                                  # a duplicated column
    ne = linear_fit.NormalEquations(lu.Shape(12, 3), G=torch.from_numpy(lu.stacked_gram(Zh, Y)))
    with pytest.raises(ValueError, match="not positive definite at ridge=0; raise ridge"):
        ne.solve(ridge=0.0)
    fit = ne.solve(ridge=1e-6)
    res = np.hstack([Zh, np.ones((500, 1))]) @ np.vstack([fit.kernel.numpy(), fit.bias.numpy()[None]]) - Y
    assert (res ** 2).sum() <= 1.001 * lu.lstsq_ref(Zh, Y, 0.0, True)[2].sum()
    # a zero column (an RBF nobody reaches) has a zero diagonal entry: scaled by 1, refused at ridge 0, weight 0 with a ridge
    Zh[:, 5] = 0.0
    ne = linear_fit.NormalEquations(lu.Shape(12, 3), G=torch.from_numpy(lu.stacked_gram(Zh, Y)))
    with pytest.raises(ValueError, match="not positive definite"):
        ne.solve(ridge=0.0)
    assert (ne.solve(ridge=1e-6).kernel.numpy()[5] == 0).all()


def test_non_finite_gram_is_refused_with_its_count():
    Zh, Y = _system(2)
    G = torch.from_numpy(lu.stacked_gram(Zh, Y))
    G[3, :] = float("nan")
    G[:, 3] = float("nan")
    with pytest.raises(ValueError, match=r"%d non-finite" % (2 * 16 - 1)):
        linear_fit.NormalEquations(lu.Shape(12, 3), G=G).solve()
    with pytest.raises(ValueError, match="no rows"):
        linear_fit.NormalEquations(lu.Shape(12, 3)).solve()


def test_merge_equals_the_accumulator_of_the_concatenated_rows():
    z = lu.integer_rows(700, 8 + 1 + 2, seed=3).astype(np.float64)
    z[:, 8] = 1.0
    parts = [z[:300], z[300:]]
    acc = [linear_fit.NormalEquations(lu.Shape(8, 2), G=torch.from_numpy(p.T @ p)) for p in parts]
    whole = z.T @ z
    merged = linear_fit.NormalEquations(lu.Shape(8, 2)).merge(acc[0]).merge(acc[1])
    assert merged.G.numpy().tobytes() == whole.tobytes()
    assert acc[0].G.numpy().tobytes() == (parts[0].T @ parts[0]).tobytes()        # the merged-in accumulator is left as it was
    assert merged.all_reduce() is merged and merged.solve().n == 700
    with pytest.raises(ValueError):
        merged.merge(linear_fit.NormalEquations(lu.Shape(9, 2)))
    with pytest.raises(ValueError):
        linear_fit.NormalEquations(lu.Shape(8, 2), G=torch.zeros(5, 5, dtype=torch.float64))


def test_float64_nets_are_refused():
    class F64(lu.Shape):
        use_float64 = True
    with pytest.raises(ValueError, match="float64"):
        linear_fit.NormalEquations(F64(4, 1))
    from irbfn_amd.model import WCRBFNet
    net = WCRBFNet.from_config(lu.synthetic_cfg(3, 4, "gaussian"), use_float64=True)
    with pytest.raises(ValueError, match="float64"):
        net.hidden(net.init(), np.zeros((2, 3), np.float32))


def test_host_module_surface():
    import irbfn_amd
    assert irbfn_amd.linear_fit is linear_fit
    for name in ("syrk", "NormalEquations", "LinearFit", "fit_linear"):
        assert hasattr(linear_fit, name)


# ------------------------------------------------------------------ margins of the GPU cases
def test_gram_cases_are_what_the_gpu_tests_assume():
    z = lu.integer_rows(1000, 129, seed=5)
    assert np.abs(z).max() <= 1024 and (z == np.rint(z)).all()
    assert np.abs(z.mean(0)).max() > 50                                  # asymmetric columns: sums do not cancel
    assert np.array_equal(lu.gram_int(z), lu.gram_ref(z))                # float64 holds every sum exactly
    zf = lu.float_rows(1000, 65, seed=6)
    col = np.abs(zf).max(0)
    assert col.max() / col.min() > 2.0 ** 8 and np.isfinite(zf).all()


@pytest.mark.parametrize("basis", lu.BASES)
def test_float32_restatement_of_the_synthetic_nets_stays_inside_0p7_of_the_bound(basis):
    worst = 0.0
    for D in lu.SYN_DIMS:
        for K in lu.SYN_KS:
            cfg, params, x, h64, bound = lu.synthetic_case(D, K, basis)
            lo = 1.0 / lu.DELTA
            assert x.min() >= lo and x.max() <= lu.BOX - lo               # inside the gate's box
            worst = max(worst, lu.ratio(lu.hidden_restated32(cfg, params, x), h64, bound))
    print(f"{basis}: float32 restatement err/bound {worst:.3f}")
    assert worst <= 0.7


def test_fit_case_is_well_conditioned():
    cfg, centers, log_sigs, x, y, h64, gsum = lu.fit_case()
    assert h64.shape == (1500, 48) and y.shape == (1500, 3)
    assert np.linalg.cond(np.hstack([h64, np.ones((1500, 1))])) < 100


def _small_fit(K=4, O=2):
    rng = np.random.default_rng(11)
    W, b = torch.from_numpy(rng.normal(size=(K, O))), torch.from_numpy(rng.normal(size=O))
    return linear_fit.LinearFit(W, b, 10, torch.zeros(O, dtype=torch.float64), 0.0)


def _as_torch(tree):
    return {g: {k: torch.from_numpy(np.array(v)) for k, v in grp.items()} for g, grp in tree.items()}


@pytest.mark.parametrize("wrapped", (True, False))
@pytest.mark.parametrize("flavour", ("numpy", "torch"))
def test_with_fit_replaces_the_linear_leaves_and_nothing_else(flavour, wrapped):
    from irbfn_amd.model import WCRBFNet
    cfg = lu.synthetic_cfg(3, 4, "gaussian")
    centers = np.random.default_rng(0).uniform(0.0, 4.0, size=(4, 3)).astype(np.float32)
    fit = _small_fit()
    fixed = WCRBFNet.from_config(dict(cfg, fixed_centers=True, fixed_width=True), centers=centers)
    assert set(fixed.init()["params"]) == {"linear"}                     # the reduced tree of a fixed-centre net
    for net in (WCRBFNet.from_config(cfg), fixed):
        tree = net.init()["params"]
        if flavour == "torch":
            tree = _as_torch(tree)
        params = {"params": tree} if wrapped else tree
        leaves = {(g, k): (v, np.array(v.numpy() if flavour == "torch" else v)) for g, grp in tree.items() for k, v in grp.items()}
        new = linear_fit.with_fit(params, fit)
        assert set(new) == set(params) and ("params" in new) == wrapped
        inner = new["params"] if wrapped else new
        assert {g: set(v) for g, v in inner.items()} == {g: set(v) for g, v in tree.items()}          # the tree keeps its shape
        assert new is not params and inner is not tree and inner["linear"] is not tree["linear"]
        for (g, k), (leaf, copy) in leaves.items():                       # the input is as it was, and every other leaf is shared
            assert tree[g][k] is leaf and np.array_equal(np.asarray(leaf), copy)
            assert g == "linear" or inner[g][k] is leaf
        for name, t in (("kernel", fit.kernel), ("bias", fit.bias)):
            leaf = inner["linear"][name]
            if flavour == "torch":
                assert isinstance(leaf, torch.Tensor) and leaf.dtype == torch.float32 and leaf.device == tree["linear"][name].device
                assert torch.equal(leaf, t.to(torch.float32))
            else:
                assert isinstance(leaf, np.ndarray) and leaf.dtype == np.float32 and np.array_equal(leaf, t.numpy().astype(np.float32))


@pytest.mark.parametrize("wrapped", (True, False))
@pytest.mark.parametrize("flavour", ("numpy", "torch"))
def test_subnet_gives_the_sliced_tree_the_fit_in_the_flavour_of_the_callers_leaves(flavour, wrapped):
    from irbfn_amd import ols
    from irbfn_amd.model import WCRBFNet
    rng = np.random.default_rng(5)
    net = WCRBFNet.from_config(lu.synthetic_cfg(3, 4, "gaussian"))
    ne = linear_fit.NormalEquations(net, G=torch.from_numpy(lu.stacked_gram(rng.uniform(size=(50, 4)), rng.normal(size=(50, 2)))))
    res = ols.OLSResult(ne, torch.tensor([2, 0, 3], dtype=torch.int32), None, None, 1e-8, 0.0, True)
    tree = net.init()["params"]
    tree["linear"]["kernel"] = rng.normal(size=(4, 2)).astype(np.float32)
    if flavour == "torch":
        tree = _as_torch(tree)
    net_k, new, fit = res.subnet(net, {"params": tree} if wrapped else tree, k=2)
    assert ("params" in new) == wrapped and net_k.num_kernels == 2
    inner = new["params"] if wrapped else new
    want = ne.subset([2, 0], net_k).solve(ridge=1e-8)
    assert fit.kernel.numpy().tobytes() == want.kernel.numpy().tobytes() and tuple(tree["linear"]["kernel"].shape) == (4, 2)
    for name, t in (("kernel", want.kernel), ("bias", want.bias)):
        leaf = inner["linear"][name]
        assert type(leaf) is type(tree["linear"][name]) and tuple(leaf.shape) == tuple(t.shape)
        assert np.asarray(leaf).dtype == np.float32 and np.array_equal(np.asarray(leaf), t.numpy().astype(np.float32))
    c = inner["rbf_list"]["centers"]
    assert type(c) is type(tree["rbf_list"]["centers"]) and np.array_equal(np.asarray(c), np.asarray(tree["rbf_list"]["centers"])[:, [2, 0]])
