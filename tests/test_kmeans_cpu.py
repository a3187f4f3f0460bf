"""CPU checks of the k-means stage (irbfn_amd/kmeans.py, irbfn_kmeans_step): the float64 reference of the GPU tests against
scipy, the margins of the cases the GPU tests rely on (blobs, integer grid, tie grid), the reference's empty-cluster and
non-finite-row rules, and the C ABI's refusals, all decided before any HIP call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _kmeans_util as ku
from irbfn_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("irbfn_kmeans_workspace_bytes", "irbfn_kmeans_step")
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
    assert any(u[0] == "kmeans.hip" and u[1] == "kmeans.o" for u in build.UNITS)
    assert "unpinned" in hdr[hdr.index("k-means on a table"):]


def test_status_table_without_gpu():
    lib = _lib.load()
    one = C.c_void_p(8)                  # a non-null, 8-byte aligned pointer that is never dereferenced: every call stops earlier
    good = dict(x=one, c=one, labels=one, d2=one, new=one, counts=one, stats=one, N=4, K=3, D=8, ws=one, nbytes=1 << 40)

    def call(**kw):
        a = dict(good, **kw)
        return lib.irbfn_kmeans_step(a["x"], a["c"], a["labels"], a["d2"], a["new"], a["counts"], a["stats"], a["N"], a["K"],
                                     a["D"], a["ws"], a["nbytes"], None)
    for k in ("x", "c", "labels", "stats"):
        assert call(**{k: None}) == BAD_ARG, k
    assert call(x=None, c=None, labels=None, stats=None) == BAD_ARG
    assert call(K=0) == BAD_ARG and call(K=-1) == BAD_ARG
    assert call(D=0) == BAD_ARG and call(N=-1) == BAD_ARG
    assert call(D=17) == UNSUPPORTED and call(K=65537) == UNSUPPORTED
    assert call(D=17, x=None) == BAD_ARG                      # a bad argument wins over an unsupported size
    assert call(ws=None) == BAD_ARG and call(ws=C.c_void_p(12)) == BAD_ARG
    assert call(nbytes=lib.irbfn_kmeans_workspace_bytes(4, 3, 8) - 1) == BAD_ARG
    # an empty table: no launch, no pointer needed
    assert call(N=0) == OK
    assert call(N=0, x=None, c=None, labels=None, stats=None, ws=None, nbytes=0) == OK
    assert call(N=0, K=0) == BAD_ARG and call(N=0, D=17) == UNSUPPORTED


def test_workspace_bytes():
    lib = _lib.load()
    w = lib.irbfn_kmeans_workspace_bytes
    sizes = [(0, 1, 1), (1, 1, 1), (1000, 5, 2), (1 << 22, 500, 8), (1 << 22, 4096, 8), (10 ** 8, 5000, 8), (10 ** 8, 65536, 16)]
    vals = [w(*s) for s in sizes]
    assert all(v > 0 and v % 8 == 0 for v in vals)
    for N in (0, 1, 1 << 20, 1 << 33):
        by_k = [w(N, K, 8) for K in (1, 2, 63, 500, 4096, 65536)]
        assert by_k == sorted(by_k)
    for K in (1, 500, 65536):
        by_n = [w(N, K, 8) for N in (0, 1, 1000, 1 << 22, 1 << 33)]
        assert by_n == sorted(by_n)
    assert w(-1, 5, 2) == BAD_ARG and w(10, 0, 2) == BAD_ARG and w(10, 5, 0) == BAD_ARG
    assert w(10, 65537, 2) == UNSUPPORTED and w(10, 5, 17) == UNSUPPORTED
    assert vals[-1] < 16 << 20                                # the largest supported shape: 8.9 MB of cells


def test_reference_matches_scipy_vq():
    from scipy.cluster.vq import vq
    for D, N, K, seed in ((8, 4096, 257, 0), (3, 1000, 65, 1), (1, 500, 7, 2)):
        x, c = ku.uniform_case(N, K, D, seed)
        d2 = ku.d2_ref(x, c)
        code, dist = vq(x.astype(np.float64), c.astype(np.float64))
        lab = ku.labels_of(d2)
        assert np.array_equal(lab, code)
        assert np.allclose(np.sqrt(d2[np.arange(N), lab]), dist, rtol=1e-12, atol=0)


def test_float32_chain_is_inside_gamma_and_the_label_condition_holds():
    x, c = ku.uniform_case(4096, 257, 8, 0)
    d64 = ku.d2_ref(x, c)
    d32 = ku.d2_chain32(x, c).astype(np.float64)             # separate multiply and add: one more rounding per term than the fused chain
    g = ku.gamma(8)
    assert (np.abs(d32 - d64) <= g * d64).all()
    lab = d32.argmin(axis=1)
    assert (d64[np.arange(4096), lab] <= d64.min(axis=1) * (1 + 3 * g)).all()


def test_blob_case_keeps_its_margin_at_every_iteration():
    x, ids, init = ku.blobs()
    c = init.astype(np.float64)
    prev = None
    for it in range(6):
        d2 = np.sort(ku.d2_ref(x, c), axis=1)
        with np.errstate(divide="ignore"):                    # a seed row sits on its centre in the first iteration
            assert (d2[:, 1] / d2[:, 0]).min() > 1 + 1e-3
        s = ku.lloyd_step(x, c, prev)
        assert np.array_equal(s["labels"], ids), it           # the labels are the blob ids from the first iteration
        assert s["moved"] == (2000 if it == 0 else 0)
        c, prev = s["centers"].astype(np.float32).astype(np.float64), s["labels"]
    assert np.abs(c - ku.BLOB_MEANS).max() < 0.2


def test_integer_grid_is_exact_in_float32():
    x, c = ku.integer_case()
    d64 = ku.d2_ref(x, c)
    assert d64.max() < 2 ** 24 and d64.max() > 1.0e6
    assert np.array_equal(ku.d2_chain32(x, c).astype(np.float64), d64)
    x, c = ku.tie_case()
    d64 = ku.d2_ref(x, c)
    assert np.array_equal(ku.d2_chain32(x, c).astype(np.float64), d64)
    tied = (d64 == d64.min(axis=1, keepdims=True)).sum(axis=1) > 1
    assert tied.sum() > 300                                   # the case is about ties


def test_reference_rules_for_empty_clusters_and_non_finite_rows():
    x = np.array([[0, 0], [1, 0], [np.nan, 0], [10, 10], [np.inf, 1], [11, 10]], np.float32)
    c = np.array([[0, 0], [10, 10], [500, 500], [np.nan, 0]], np.float32)
    s = ku.lloyd_step(x, c, prev=np.array([0, 1, 0, 1, 1, -1]))
    assert s["labels"].tolist() == [0, 0, -1, 1, -1, 1]
    assert np.isnan(s["d2"][[2, 4]]).all() and s["d2"][[0, 1, 3, 5]].tolist() == [0.0, 1.0, 0.0, 1.0]
    assert s["counts"].tolist() == [2, 2, 0, 0] and s["finite"] == 4 and s["inertia"] == 2.0
    assert s["moved"] == 2                                    # rows 1 and 5; rows 2 and 4 count nowhere
    assert s["centers"][:2].tolist() == [[0.5, 0.0], [10.5, 10.0]]
    assert s["centers"][2].tolist() == [500.0, 500.0] and np.isnan(s["centers"][3, 0])      # kept as they were
    assert s["shift2"] == 0.25


def test_host_module_surface():
    import irbfn_amd
    from irbfn_amd import kmeans
    assert irbfn_amd.kmeans is kmeans
    assert kmeans.STATS == ("finite", "inertia", "moved", "max_shift2")

    class Net:
        num_kernels, in_features = 5, 2

    class Res(kmeans.KMeansResult):
        pass
    import torch
    r = Res(torch.zeros(5, 2), None, None, torch.zeros(0, 4, dtype=torch.float64), 0)
    assert r.as_centers(Net()).shape == (5, 2) and r.as_centers(Net()).dtype == np.float32
    Net.num_kernels = 6
    with pytest.raises(ValueError):
        r.as_centers(Net())
