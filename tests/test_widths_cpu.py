"""CPU checks of the width stage (irbfn_amd/widths.py, irbfn_knn_d2): the C ABI's declarations and refusals, all decided before
any HIP call, the float64 reference of the GPU tests against scipy's k-d tree, and the margins by which the NumPy statement of the
end-to-end problem meets the three conditions tests/test_gpu_widths.py asserts on the device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _kmeans_util as ku
import _widths_util as wu
from irbfn_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("irbfn_knn_workspace_bytes", "irbfn_knn_d2")
OK, BAD_ARG, UNSUPPORTED = 0, -1, -2


def test_new_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "irbfn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} not declared in include/irbfn_hip.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _lib.SIGNATURES
    assert lib.irbfn_abi_version() == 1
    assert any(u[0] == "knn.hip" and u[1] == "knn.o" for u in build.UNITS)
    block = hdr[hdr.index("The p nearest centres of every row"):hdr.index("irbfn_knn_workspace_bytes(int64_t")]
    assert "unpinned" in block


def test_status_table_without_gpu():
    lib = _lib.load()
    one = C.c_void_p(8)                  # a non-null, 8-byte aligned pointer that is never dereferenced: every call stops earlier
    good = dict(q=one, c=one, N=4, K=300, D=8, p=2, self0=-1, split=0, d2=one, idx=one, ws=one, nbytes=1 << 40)

    def call(**kw):
        a = dict(good, **kw)
        return lib.irbfn_knn_d2(a["q"], a["c"], a["N"], a["K"], a["D"], a["p"], a["self0"], a["split"], a["d2"], a["idx"], a["ws"],
                                a["nbytes"], None)
    for k in ("q", "c", "d2"):
        assert call(**{k: None}) == BAD_ARG, k
    assert call(q=None, c=None, d2=None) == BAD_ARG
    assert call(N=-1) == BAD_ARG
    for k in ("K", "D", "p"):
        assert call(**{k: 0}) == BAD_ARG and call(**{k: -1}) == BAD_ARG, k
    assert call(self0=-2) == BAD_ARG and call(split=-1) == BAD_ARG
    assert call(D=17) == UNSUPPORTED and call(K=65537) == UNSUPPORTED and call(p=17) == UNSUPPORTED
    for big in (dict(D=17), dict(K=65537), dict(p=17)):          # a bad argument wins over an unsupported size
        assert call(q=None, **big) == BAD_ARG and call(self0=-2, **big) == BAD_ARG and call(split=-1, **big) == BAD_ARG
    assert call(D=17, p=0) == BAD_ARG
    assert call(ws=None) == BAD_ARG and call(ws=C.c_void_p(12)) == BAD_ARG
    for big in (dict(D=17), dict(K=65537), dict(p=17)):          # so does a NULL or misaligned workspace; a short one cannot: it has no size
        assert call(ws=None, **big) == BAD_ARG and call(ws=C.c_void_p(12), **big) == BAD_ARG and call(nbytes=0, **big) == UNSUPPORTED
    for split in (0, 1, 2, 1000):
        need = lib.irbfn_knn_workspace_bytes(4, 300, 8, 2, split)
        assert call(split=split, nbytes=need - 1) == BAD_ARG, split
    # no row: no launch, no pointer needed
    assert call(N=0) == OK
    assert call(N=0, q=None, c=None, d2=None, idx=None, ws=None, nbytes=0) == OK
    assert call(N=0, K=0) == BAD_ARG and call(N=0, D=17) == UNSUPPORTED and call(N=0, p=17) == UNSUPPORTED


def test_workspace_bytes():
    lib = _lib.load()
    w = lib.irbfn_knn_workspace_bytes
    Ns, Ks, ps, splits = (0, 1, 1000, 65536, 1 << 22, 1 << 33), (1, 2, 128, 129, 500, 4096, 65536), (1, 2, 3, 4, 5, 8, 9, 16), (1, 2, 3, 5, 1000)
    for split in (0,) + splits:
        for p in ps:
            for K in Ks:
                by_n = [w(N, K, 8, p, split) for N in Ns]
                assert all(v > 0 and v % 8 == 0 for v in by_n) and by_n == sorted(by_n), (split, p, K)
            for N in Ns:
                by_k = [w(N, K, 8, p, split) for K in Ks]
                assert by_k == sorted(by_k), (split, p, N)
        for N in Ns:
            for K in Ks:
                by_p = [w(N, K, 8, p, split) for p in ps]
                assert by_p == sorted(by_p), (split, N, K)
    for N in Ns:
        for K in Ks:
            by_s = [w(N, K, 8, 8, s) for s in splits]
            assert by_s == sorted(by_s), (N, K)
            assert by_s[0] <= w(N, K, 8, 8, 0) <= by_s[-1]        # 0 = the library chooses: between one segment and one per tile
    assert w(1 << 22, 500, 8, 4, 0) < 65 << 20 and w(65536, 65536, 16, 16, 0) < 65 << 20      # split = 0 never asks for more than 64 MiB of lists
    assert w(-1, 5, 2, 1, 0) == BAD_ARG and w(10, 0, 2, 1, 0) == BAD_ARG and w(10, 5, 0, 1, 0) == BAD_ARG
    assert w(10, 5, 2, 0, 0) == BAD_ARG and w(10, 5, 2, 1, -1) == BAD_ARG
    assert w(10, 65537, 2, 1, 0) == UNSUPPORTED and w(10, 5, 17, 1, 0) == UNSUPPORTED and w(10, 5, 2, 17, 0) == UNSUPPORTED
    assert w(10, 65537, 2, 0, 0) == BAD_ARG


def test_reference_matches_scipy_kdtree():
    from scipy.spatial import cKDTree
    for D, N, K, p, seed in ((8, 1000, 257, 3, 0), (3, 500, 65, 8, 1), (1, 300, 40, 2, 2)):
        x, c = ku.uniform_case(N, K, D, seed)
        d2, idx = wu.knn_ref(x, c, p)
        dist, ind = cKDTree(c.astype(np.float64)).query(x.astype(np.float64), k=p)
        dist, ind = dist.reshape(N, p), ind.reshape(N, p)
        assert np.array_equal(idx, ind)
        assert np.allclose(np.sqrt(d2), dist, rtol=1e-12, atol=0)
    # centres against themselves, one centre duplicated: the query's own index is dropped, the duplicate stays at distance 0
    c = wu.duplicate_case()
    d2, idx = wu.knn_ref(c, c, 3, self0=0)
    dist, ind = cKDTree(c.astype(np.float64)).query(c.astype(np.float64), k=4)
    for n in range(len(c)):
        assert n not in idx[n]
        keep = [j for j in range(4) if ind[n, j] != n][:3]
        assert np.allclose(np.sqrt(d2[n]), dist[n, keep], rtol=1e-12, atol=0)
        kept = ind[n, keep]
        assert np.array_equal(idx[n], kept[np.lexsort((kept, dist[n, keep]))])     # the tree leaves the order inside a tie open
    assert idx[2, 0] == 7 and idx[7, 0] == 2 and idx[30, 0] == 31 and idx[31, 0] == 30 and (d2[[2, 7, 30, 31], 0] == 0).all()


def test_reference_rules_for_ties_empty_slots_and_non_finite_values():
    q = np.array([[0, 0], [1, 0], [np.nan, 0], [3.0e38, 0]], np.float32)
    c = np.array([[1, 0], [0, 1], [-1, 0], [np.inf, 0], [0, -1]], np.float32)
    d2, idx = wu.knn_ref(q, c, 5)
    assert idx[0].tolist() == [0, 1, 2, 4, -1] and d2[0, :4].tolist() == [1, 1, 1, 1] and np.isnan(d2[0, 4])       # ties ascend in k
    assert idx[1].tolist() == [0, 1, 4, 2, -1] and d2[1, :4].tolist() == [0, 2, 2, 4]
    assert (idx[2] == -1).all() and np.isnan(d2[2]).all()
    assert np.isfinite(d2[3, :4]).all()                       # finite in float64; the float32 chain overflows (the GPU test says so)
    d2, idx = wu.knn_ref(c[:3], c[:3], 4, self0=0)
    assert idx.tolist() == [[1, 2, -1, -1], [0, 2, -1, -1], [1, 0, -1, -1]]
    d2, idx = wu.knn_ref(c[1:3], c[:3], 1, self0=1)           # the rows are centres 1 and 2
    assert idx.tolist() == [[0], [1]]
    d2, idx = wu.knn_ref(c[:3], c[:3], 1, self0=5)            # self0 + n >= K excludes nothing
    assert idx.tolist() == [[0], [1], [2]] and (d2 == 0).all()


def test_width_rules_and_the_replacement_rule():
    s, rep = wu.nn_widths_ref(np.array([[1.0, 3.0], [4.0, np.nan], [0.0, 0.0], [np.nan, np.nan], [16.0, 16.0]]), scale=2.0)
    assert rep == 2 and s.tolist() == [2 * np.sqrt(2.0), 4.0, 4.0, 4.0, 8.0]      # the median of (sqrt 2, 2, 4) is 2
    with pytest.raises(ValueError):
        wu.nn_widths_ref(np.full((1, 2), np.nan))
    s, rep = wu.spread_widths_ref([1.0, 3.0, 5.0, 9.0, 9.0, 7.0], [0, 0, 1, 2, 2, -1], 4)
    mid = (np.sqrt(2.0) + 3.0) / 2                           # one row, or none, is no cluster: the median of the other two
    assert rep == 2 and s.tolist() == [np.sqrt(2.0), mid, 3.0, mid]
    s, rep = wu.spread_widths_ref([1.0, 3.0, 5.0], [0, 0, 1], 2, min_count=1)
    assert rep == 0 and s.tolist() == [np.sqrt(2.0), np.sqrt(5.0)]


def test_cluster_sums_are_exact_integer_sums():
    """torch operations only, so the host runs them too.  Integer-valued rows below 2^S come out exactly; float rows within
    count 2^(e - S - 1) of the exact sum plus one float64 rounding; any order of the rows gives the same bits."""
    import torch

    from irbfn_amd import widths
    rng = np.random.default_rng(5)
    N, K = 50_000, 37                                         # N < 2^16: S = 46
    lab = rng.integers(-1, K, N)
    lab[lab == 5] = 6                                         # an empty cluster
    ints = rng.integers(0, 1 << 20, N).astype(np.float64)
    ints[0] = float(1 << 20)                                  # the largest value: e = 21, the grid is 2^-25
    ok = lab >= 0
    sums, counts = widths.cluster_sums(torch.from_numpy(ints), torch.from_numpy(lab.astype(np.int32)), K)
    want = np.bincount(lab[ok], weights=ints[ok], minlength=K)
    assert np.array_equal(counts.numpy(), np.bincount(lab[ok], minlength=K)) and counts[5] == 0
    assert np.array_equal(sums.numpy(), want) and sums[5] == 0
    v = (rng.uniform(0, 3, N) ** 2).astype(np.float32).astype(np.float64)
    sums, counts = widths.cluster_sums(torch.from_numpy(v), torch.from_numpy(lab), K)
    exact = np.array([float(np.sum(v[lab == k].astype(np.longdouble))) for k in range(K)])
    e = np.frexp(v[ok].max())[1]
    assert (np.abs(sums.numpy() - exact) <= counts.numpy() * 2.0 ** (e - 46 - 1) + 2.0 ** -52 * exact).all()
    perm = rng.permutation(N)
    again, _ = widths.cluster_sums(torch.from_numpy(v[perm]), torch.from_numpy(lab[perm]), K)
    assert torch.equal(again, sums)
    for scale in (2.0 ** -100, 2.0 ** 60):                    # a power of two moves e and nothing else
        scaled, _ = widths.cluster_sums(torch.from_numpy(v * scale), torch.from_numpy(lab), K)
        assert torch.equal(scaled, sums * scale)
    z, c0 = widths.cluster_sums(torch.zeros(4, dtype=torch.float64), torch.tensor([0, 1, 1, -1]), 3)
    assert z.tolist() == [0, 0, 0] and c0.tolist() == [1, 2, 0]
    z, c0 = widths.cluster_sums(torch.zeros(0, dtype=torch.float64), torch.zeros(0, dtype=torch.int32), 3)
    assert z.tolist() == [0, 0, 0] and c0.tolist() == [0, 0, 0]


@pytest.mark.parametrize("s", (0.05, 20.0))
def test_end_to_end_statement_meets_its_conditions_with_a_factor_two_to_spare(s):
    x, y = wu.e2e_problem(s)
    c = wu.lloyd_centers(x)
    nd2, _ = wu.knn_ref(c, c, 2, self0=0)
    sigma, rep = wu.nn_widths_ref(nd2)
    assert rep == 0
    _, held, best = wu.scale_search_ref(x, y, c, sigma)
    _, unit = wu.price_ref(x, y, c, np.ones(64))             # log_sigs = 0
    print(f"s = {s}: held-out MSE per scale {['%.3e' % h for h in held]}, at log_sigs = 0 {unit:.3e}, best scale {wu.SCALES[best]}")
    assert wu.SCALES[best] in (2.0, 4.0)
    assert 2 * held[best] <= unit / 10
    assert 2 * held[best] <= held[0] / 4 and 2 * held[best] <= held[4] / 4
    # the margin of `best` itself: the scales outside {2, 4} are at least twice as bad as the best
    assert all(h >= 2 * held[best] for i, h in enumerate(held) if wu.SCALES[i] not in (2.0, 4.0))


def test_host_module_surface():
    import torch

    import irbfn_amd
    from irbfn_amd import linear_fit, widths
    assert irbfn_amd.widths is widths and "irbfn_amd.widths" in irbfn_amd.__doc__
    assert hasattr(linear_fit.NormalEquations, "rss_of")

    class Net:
        num_kernels, num_regions = 3, 2
    w = widths.Widths(torch.tensor([1.0, np.e, 0.5]), replaced=1)
    ls = w.log_sigs(Net())
    assert ls.shape == (2, 3) and ls.dtype == np.float32 and np.array_equal(ls[0], ls[1])
    assert np.allclose(ls[0], [0.0, 1.0, np.log(0.5)], rtol=1e-6)
    w2 = w.scaled(4.0)
    assert w2.replaced == 1 and np.array_equal(w2.sigma.numpy(), w.sigma.numpy() * 4)
    Net.num_kernels = 4
    with pytest.raises(ValueError):
        w.log_sigs(Net())
    # rss_of on a host accumulator: the fit's own rss on its own rows, the float64 residual on others
    rng = np.random.default_rng(0)

    class Shape:
        use_float64, num_kernels, out_features = False, 5, 2
    def gram(n):
        h, y = rng.uniform(0, 1, (n, 5)), rng.normal(size=(n, 2))
        Z = np.hstack([h, np.ones((n, 1)), y])
        return h, y, torch.from_numpy(Z.T @ Z)
    h1, y1, G1 = gram(50)
    h2, y2, G2 = gram(30)
    for fit_bias in (True, False):
        ne = linear_fit.NormalEquations(Shape(), G=G1)
        fit = ne.solve(ridge=1e-8, fit_bias=fit_bias)
        assert torch.equal(ne.rss_of(fit), fit.rss)
        W, b = fit.kernel.numpy(), fit.bias.numpy()
        want = ((h2 @ W + b - y2) ** 2).sum(0)
        got = linear_fit.NormalEquations(Shape(), G=G2).rss_of(fit).numpy()
        assert np.abs(got - want).max() <= 1e-9 * (y2 ** 2).sum(0).max()
