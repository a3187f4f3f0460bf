"""K2 (`rbf_vjp_kernel<D, OP, BC, GATED>`, rbf_vjp.hip) on its own: the query packing, the kernel, the slab reduce, the region reduce
and the bias column sums against the float64 restatement of tests/_k2_util.py, at the edges of its shapes -- every padded D and O,
the four basis classes with both gate forms, partly filled centre groups, the launches above 64 KiB of LDS, regions around the
wave width of the region reduce, caller-provided region weights, batches that leave waves without queries, the switch of the bias
partials, a reused workspace, non-finite inputs and queries on centres.  The cases are tests/_k2_util.py::TABLE.

K2 is forced (vjp_kernel=VJP_K2) unless the case is about AUTO.  Every run states the launch it expects from the restated layout
rules (name, grid = centre groups x slabs), writes the leaves into views of one NaN-filled buffer with 64 guard words around each,
and runs twice: the two buffers must be bit-identical and the guards still NaN.

Bounds, on every leaf (tests/_k2_util.py): max|got - ref| <= 5e-5 max|ref| + 1e-7, and element-wise |got - ref| <= C_S S + 1e-30
with S the sum of the absolute per-query terms of that element and C_S = 4 x the worst error of a plain float32 evaluation of the
same formulas (6.8e-6).  Each run prints, per leaf, the kernel's and the float32 yardstick's worst |err| / S and the kernel's
max-norm ratio (profiles/k2_parity.txt)."""
import numpy as np
import pytest

import _k2_util as k2
import _vjp_guard_util as guarded
from _vjp_guard_util import make_net
from irbfn_amd import _lib

pytestmark = pytest.mark.gpu

BY_TAG = {s["tag"]: s for s in k2.TABLE}


def run_twice(torch, net, case, x=None, g=None, option=_lib.VJP_K2, B=None):
    """Two runs, bit-identical; the launch is the one the restated rules give."""
    plan = case.plan() if B is None else k2.k2_plan(case.N, B, case.D, case.O, case.basis, case.gated)

    def expect(launch):
        assert launch["kernel"] == plan["name"] and launch["grid"] == plan["grid"] and launch["block"] == 256, (case.tag, launch, plan)

    return guarded.run_twice(torch, net, case, expect, x, g, option)


def check(case, got):
    """Both bounds on the four stage leaves; non-finite elements exactly where the reference has them."""
    ref, yard = case.reference(), case.yardstick()
    bad = []
    for leaf in k2.LEAVES:
        r, S = ref[leaf]
        assert got[leaf].dtype == np.float32 and got[leaf].shape == r.shape
        ys, _ = k2.ratios(yard[leaf], r, S)
        if ys > 5e-5:
            pytest.fail(f"test inputs, not the code under test: {case.tag} {leaf} needs {ys:.2e} S in plain float32")
        es, em = k2.ratios(got[leaf], r, S)
        print(f"K2PARITY {case.tag:32s} {leaf:9s} kernel {es:.2e}  yardstick {ys:.2e}  max-norm ratio {em:.3f}")
        if not k2.same_nonfinite(got[leaf], r):
            bad.append(f"{leaf}: non-finite elements differ from the reference's")
        if not es <= k2.C_S:
            bad.append(f"{leaf}: |err| / S {es:.2e} > {k2.C_S:.2e}")
        if not em <= 1.0:
            bad.append(f"{leaf}: max-norm ratio {em:.3f}")
    assert not bad, (case.tag, bad)
    return ref


def run_case(torch, tag):
    case = k2.Case(BY_TAG[tag])
    got, _ = run_twice(torch, make_net(case), case)
    return case, got, check(case, got)


@pytest.mark.parametrize("tag", [s["tag"] for s in k2.SHAPES])
def test_padded_shapes_and_basis_classes(gpu, tag):
    run_case(gpu, tag)


@pytest.mark.parametrize("tag", [s["tag"] for s in k2.WIDE])
def test_wide_rows_above_64_kib_of_lds(gpu, tag):
    torch = gpu
    case = k2.Case(BY_TAG[tag])
    assert case.plan()["lds"] > 64 * 1024
    net = make_net(case)
    got, bits = run_twice(torch, net, case)
    check(case, got)
    _, auto = run_twice(torch, net, case, option=_lib.VJP_AUTO)              # O > 16: AUTO has no other kernel
    assert np.array_equal(auto, bits)
    B = 2100                                                                 # nor from 2048 queries, where narrow nets leave K2
    rng = np.random.default_rng(B)
    x, g = rng.uniform(-0.9, 1.5, size=(B, case.D)).astype(np.float32), rng.normal(size=(B, case.O)).astype(np.float32)
    _, forced = run_twice(torch, net, case, x, g, B=B)
    _, auto = run_twice(torch, net, case, x, g, option=_lib.VJP_AUTO, B=B)
    assert np.array_equal(auto, forced)


@pytest.mark.parametrize("tag", [s["tag"] for s in k2.REGIONS if s["kind"] == "regions" and "rows" not in s])
def test_regions_around_the_wave_width_of_the_region_reduce(gpu, tag):
    case, _, _ = run_case(gpu, tag)
    assert case.gated and case.R == int(tag[1:])


def test_regions_without_a_range_get_exact_zeros(gpu):
    case, got, ref = run_case(gpu, "r6_rows4")
    if not (ref["centers"][1][:4] > 0).all():
        pytest.fail("test inputs, not the code under test: a region with a range has no weight")
    assert (got["centers"][4:] == 0).all() and (got["log_sigs"][4:] == 0).all()


def test_regions_with_tiny_weights(gpu):
    """Five of six regions weigh less than 1e-6 for every query: their gradients are 1e-6 of the leaf's largest element and less,
    out of sight of the max-norm bound."""
    case = k2.Case(BY_TAG["r6_tiny"])
    gam = case.gamma()
    if not ((gam[:, 1:] < 1e-6).all() and (case.gamma(np.float32)[:, 1:] > 0).all() and (gam[:, 0] > 0.99).all()):
        pytest.fail("test inputs, not the code under test: the weights are not what the case is about")
    got, _ = run_twice(gpu, make_net(case), case)
    ref = check(case, got)
    assert np.abs(ref["centers"][0][1:]).max() < 1e-5 * np.abs(ref["centers"][0][0]).max()
    assert (got["centers"][1:] != 0).any(axis=(1, 2)).all()


@pytest.mark.parametrize("tag", [s["tag"] for s in k2.CLUSTER])
def test_caller_provided_region_weights(gpu, tag):
    case, got, _ = run_case(gpu, tag)
    assert np.isfinite(got["ckernel"]).all() and np.isfinite(got["cbias"]).all()


@pytest.mark.parametrize("B", k2.BATCH_EDGES)
def test_batch_edges(gpu, B):
    for tag in (f"b{B}_r1", f"b{B}_r4"):
        case, _, _ = run_case(gpu, tag)
        plan = case.plan()
        assert plan["QSB"] == (1 if B <= 256 else {257: 2, 513: 3, 1021: 4}[B])
        if B == 5:
            assert plan["per_wave"] == 2 and 3 * plan["per_wave"] > B          # wave 3 of the only slab starts behind the batch


@pytest.mark.parametrize("B", k2.BIAS_EDGES)
def test_bias_partials_switch_at_16384_rows(gpu, B):
    case, _, _ = run_case(gpu, f"bias_b{B}")
    assert case.plan()["bias_blocks"] == 256 and case.plan()["QSB"] == (64 if B <= 16384 else 65)


def test_workspace_reuse_after_a_larger_batch(gpu):
    """B = 4096 (16 slabs), then B = 65 (one) on the same net and workspace: the bits of a fresh net's B = 65 call."""
    torch = gpu
    case = k2.Case(BY_TAG["reuse_b65"])
    rng = np.random.default_rng(4096)
    xb, gb = rng.uniform(-0.9, 1.5, size=(4096, case.D)).astype(np.float32), rng.normal(size=(4096, case.O)).astype(np.float32)
    used = make_net(case)
    assert k2.k2_plan(case.N, 4096, case.D, case.O, case.basis, False)["QSB"] == 16 and case.plan()["QSB"] == 1
    run_twice(torch, used, case, xb, gb, B=4096)
    got, bits = run_twice(torch, used, case)
    _, fresh = run_twice(torch, make_net(case), case)
    assert np.array_equal(bits, fresh)
    check(case, got)


@pytest.mark.parametrize("tag", [s["tag"] for s in k2.NONFINITE])
def test_non_finite_inputs(gpu, tag):
    case, got, ref = run_case(gpu, tag)                 # check(): the non-finite elements are the reference's, the rest in bounds
    poison = case.spec["poison"]
    if poison == "nan_g":                               # g[17, 1]: column 1 of d kernel and d bias, every centre and width
        others = [o for o in range(case.O) if o != 1]
        assert np.isnan(got["kernel"][:, 1]).all() and np.isnan(got["bias"][1])
        assert np.isfinite(got["kernel"][:, others]).all() and np.isfinite(got["bias"][others]).all()
        assert np.isnan(got["centers"]).all() and np.isnan(got["log_sigs"]).all()
    elif poison == "nan_x":
        assert np.isnan(got["centers"]).all() and np.isnan(got["log_sigs"]).all() and np.isnan(got["kernel"]).all()
        assert np.isfinite(got["bias"]).all()
    else:                                               # g[40, 2] = +inf
        others = [o for o in range(case.O) if o != 2]
        assert (got["kernel"][:, 2] == np.inf).all() and got["bias"][2] == np.inf
        assert np.isfinite(got["kernel"][:, others]).all() and np.isfinite(got["bias"][others]).all()
        assert np.isinf(got["centers"]).all() and np.isinf(got["log_sigs"]).all()


@pytest.mark.parametrize("tag", [s["tag"] for s in k2.ON_CENTRES])
def test_queries_on_centres(gpu, tag):
    case, got, _ = run_case(gpu, tag)
    cc = case.params["params"]["rbf_list"]["centers"]
    if not all((case.x[b] == cc[0, k]).all() for b, k in ((5, 3), (20, 17), (case.B - 1, case.K - 1))):
        pytest.fail("test inputs, not the code under test: the three queries are not centres")
    assert all(np.isfinite(got[leaf]).all() for leaf in k2.LEAVES)


@pytest.mark.parametrize("tag", [s["tag"] for s in k2.ON_CENTRES_D])
def test_queries_on_centres_of_a_basis_in_d(gpu, tag):
    """The bases that depend on d = sqrt(d2) itself, three of 65 queries ON the three centres: d centers is NaN as jax.grad's (sqrt
    has no derivative at 0), d log_sigs finite (the width does not go through the sqrt); check() holds the non-finite elements to
    the reference's and the finite ones to the bounds."""
    case, got, ref = run_case(gpu, tag)
    cc = case.params["params"]["rbf_list"]["centers"]
    if not (all((case.x[b] == cc[0, k]).all() for b, k in ((5, 0), (20, 1), (64, 2))) and np.isnan(ref["centers"][0]).all()
            and np.isfinite(ref["log_sigs"][0]).all()):
        pytest.fail("test inputs, not the code under test: the three queries are not centres, or the reference's NaN are elsewhere")
    assert np.isnan(got["centers"]).all() and np.isfinite(got["log_sigs"]).all()
