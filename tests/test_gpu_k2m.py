"""K2m (`rbf_vjp_mfma<D, OW, BC, CT>`, rbf_vjp_mfma.hip) on its own: the record pre-pass with its gate, the kernel and the shared slab
reduce and bias column sums against the float64 restatement of tests/_k2_util.py, at the edges of its shapes -- every compiled
(padded D, OW, basis class), every real D, O at both ends of OW and OP, centre counts around the centre tile, the five fast bases
(the Gaussian scales 0.1 and 0.01 among them), a gate that is really between 0 and 1, read from the second range column, an exact
float32 zero, or absent, batches around the 16 zero records, the 64-query pack block and the second slab, a slab count that the
centre groups cap and whose last slab has no tile, a workspace reused after a larger batch and after a K2 call, non-finite inputs
beside the zero padding of the two MFMA contractions, and queries on centres.  The cases are tests/_k2m_util.py::TABLE.

K2m is forced (vjp_kernel = VJP_K2M).  Every run states the launch it expects from the restated rules (k2m_plan: name with the slab
count, grid = centre groups x slabs, block 256), writes the leaves into views of one NaN-filled buffer with 64 guard words around
each and runs twice: the two buffers must be bit-identical and the guards still NaN.  Once per kind of gate a forced K2 on the same
inputs must pass the same bounds and differ in some bit.

Bounds, on every leaf (tests/_k2m_util.py): max|got - ref| <= 5e-5 max|ref| + 1e-7, and element-wise |got - ref| <= C_M S + 1e-30
with S the sum of the absolute per-query terms of that element and C_M = 4 x the worst error of a plain float32 evaluation of the
same formulas (6.0e-6).  Each run prints, per leaf, the kernel's and the float32 yardstick's worst |err| / S and the kernel's
max-norm ratio (profiles/k2m_parity.txt).  On the MI355X the worst are d centers 3.24e-6 and d log_sigs 3.12e-6 (both m_b1: one
query, where the yardstick's own 1.45e-6 sets C_M), d kernel 4.40e-7 (m_b2), d bias 5.86e-8; from 15 queries on nothing above
2.8e-7, and no max-norm ratio above 0.043."""
import numpy as np
import pytest

import _k2_util as k2
import _k2m_util as km
import _vjp_guard_util as guarded
from _vjp_guard_util import make_net
from irbfn_amd import _lib

pytestmark = pytest.mark.gpu

INPUTS = "test inputs, not the code under test: "


def run_k2m(torch, net, case, x=None, g=None):
    """Two guarded runs of a forced K2m, the launch the restated rules give -> (leaves, bits)."""
    B = case.B if x is None else x.shape[0]
    plan = km.k2m_plan(case.N, B, case.D, case.O, case.basis)

    def expect(launch):
        assert launch["kernel"] == plan["name"] and launch["grid"] == plan["grid"] and launch["block"] == plan["block"] == 256, \
            (case.tag, launch, plan)

    return guarded.run_twice(torch, net, case, expect, x, g, _lib.VJP_K2M)


def run_k2(torch, net, case, x=None, g=None):
    """One guarded run of a forced K2 -> (leaves, bits)."""
    got, launch, bits = guarded.vjp_guarded(torch, net, case, x, g, _lib.VJP_K2)
    assert launch["kernel"].startswith("rbf_vjp_kernel<"), launch
    return got, bits


def check(case, got, who="kernel"):
    """Both bounds on the four leaves; non-finite elements exactly where the reference has them."""
    ref, yard = case.reference(), case.yardstick()
    bad = []
    for leaf in k2.LEAVES:
        r, S = ref[leaf]
        assert got[leaf].dtype == np.float32 and got[leaf].shape == r.shape
        ys, _ = km.ratios_m(yard[leaf], r, S)
        if ys > 5e-5:
            pytest.fail(INPUTS + f"{case.tag} {leaf} needs {ys:.2e} S in plain float32")
        es, em = km.ratios_m(got[leaf], r, S)
        print(f"K2MPARITY {case.tag:36s} {leaf:9s} {who} {es:.2e}  yardstick {ys:.2e}  max-norm ratio {em:.3f}")
        if not km.same_nonfinite(got[leaf], r):
            bad.append(f"{leaf}: non-finite elements differ from the reference's ({int(np.isnan(got[leaf]).sum())} NaN, "
                       f"{int(np.isinf(got[leaf]).sum())} Inf of {got[leaf].size}; reference {int(np.isnan(r).sum())}, {int(np.isinf(r).sum())})")
        if not es <= km.C_M:
            bad.append(f"{leaf}: |err| / S {es:.2e} > {km.C_M:.2e}")
        if not em <= 1.0:
            bad.append(f"{leaf}: max-norm ratio {em:.3f}")
    assert not bad, (case.tag, who, bad)
    return ref


def run_case(torch, tag):
    case = km.CaseM(km.BY_TAG[tag])
    net = make_net(case)
    assert _lib.load().irbfn_net_vjp_kernel_supported(net._handle(torch), _lib.VJP_K2M, case.B) == 1
    got, bits = run_k2m(torch, net, case)
    return case, got, check(case, got), bits


@pytest.mark.parametrize("tag", [s["tag"] for s in km.SHAPES])
def test_compiled_instances_shapes_bases_and_gated_coordinates(gpu, tag):
    case, got, _, _ = run_case(gpu, tag)
    p, spec = case.plan(), case.spec
    assert (p["DC"], p["OW"], p["BC"]) == (k2.padded_D(case.D), km.vjpm_ow(case.O), k2.FAST[case.basis]) and p["CW"] == 16 * p["CT"]
    assert p["groups"] == -(-case.K // p["CW"]) and p["S"] in (1, 2) and spec["ns"] == case.ns <= case.D
    assert all(np.isfinite(got[leaf]).all() and (got[leaf] != 0).any() for leaf in k2.LEAVES)


@pytest.mark.parametrize("tag", ["m_gate_column_ns1", "m_gate_column_ns3", "m_gate_sharp", "m_d8_o32_n65_gaussian"])
def test_gate_kinds_and_a_forced_k2_that_differs(gpu, tag):
    """The second range column (one and three gated coordinates, the columns 1, 0, 1), a gate with exact float32 zeros, and the
    mid gate of the shape rows: K2m in bounds, and a forced K2 on the same net in the same bounds with other bits -- the launch
    name and the bits both say which kernel ran."""
    torch = gpu
    case, got, ref, bits = run_case(torch, tag)
    k2got, k2bits = run_k2(torch, make_net(case), case)
    check(case, k2got, who="K2    ")
    if np.array_equal(bits, k2bits):
        pytest.fail(INPUTS + f"{tag}: K2 and K2m give bit-identical leaves, the case distinguishes nothing")
    if case.gate == "sharp":
        dead = case.gamma(np.float32)[:, 0] == 0
        if not (dead.any() and (case.gamma()[dead, 0] > 0).all()):
            pytest.fail(INPUTS + f"{tag}: no query with an exact float32 zero")


def test_a_card_without_a_range_row_gets_exact_zeros(gpu):
    """gamma = 0 for every query: every leaf but the bias an exact zero (K2 gives the same bits there: the name alone says which
    ran)."""
    case, got, _, _ = run_case(gpu, "m_gate_none")
    assert all((got[leaf] == 0).all() for leaf in ("centers", "log_sigs", "kernel")) and (got["bias"] != 0).all()


EDGE = {1: (1, 1, [1, 2, 3]), 2: (1, 1, [1, 2, 3]), 15: (1, 1, [1, 2, 3]), 16: (1, 1, [1, 2, 3]), 17: (1, 1, [2, 3]), 63: (1, 1, []),
        64: (1, 1, []), 65: (1, 2, [3]), 255: (1, 4, []), 256: (1, 4, []), 257: (2, 3, [6, 7]), 513: (3, 3, [11]), 1021: (4, 4, [])}


@pytest.mark.parametrize("B", km.BATCH_EDGES)
def test_batch_edges(gpu, B):
    """N = 40: two centre groups.  Slabs, tiles per wave, waves without a tile; B = 1 .. 15 leave zero records in the only tile,
    17 one query in the second, 65 the second pack block with one query, 257 the second slab with one tile."""
    case, _, _, _ = run_case(gpu, f"m_b{B}")
    p = case.plan()
    assert (p["S"], p["tiles_per_wave"], p["idle_waves"]) == EDGE[B] and p["grid"] == 2 * p["S"]


def test_slabs_capped_by_the_centre_groups_and_a_slab_without_a_tile(gpu):
    """N = 1000, O = 100 (OP = 100 under OW = 128): 63 groups, so ceil(512 / 63) = 9 slabs where the batch of 2305 would allow 10;
    145 tiles at 5 a wave end in wave 28: the four waves of the ninth slab walk no tile, write zeros, and the reduce adds them."""
    case = km.CaseM(km.BY_TAG["m_slab_cap"])
    p = case.plan()
    assert p["S"] == p["by_groups"] == 9 < min(p["by_batch"], p["QSB"]) and p["groups"] == 63
    assert set(range(4 * (p["S"] - 1), 4 * p["S"])) <= set(p["idle_waves"]) and p["OP"] == 100 and p["OW"] == 128
    got, _ = run_k2m(gpu, make_net(case), case)
    check(case, got)


def test_workspace_reuse_after_a_larger_batch(gpu):
    """B = 4096 (16 slabs), then B = 65 (one) on the same net and workspace: the bits of a fresh net's call."""
    torch = gpu
    case = km.CaseM(km.BY_TAG["m_reuse_b65"])
    rng = np.random.default_rng(4096)
    xb, gb = rng.uniform(-0.9, 1.5, size=(4096, case.D)).astype(np.float32), rng.normal(size=(4096, case.O)).astype(np.float32)
    assert km.k2m_plan(case.N, 4096, case.D, case.O, case.basis)["S"] == 16 and case.plan()["S"] == 1
    used = make_net(case)
    run_k2m(torch, used, case, xb, gb)
    got, bits = run_k2m(torch, used, case)
    _, fresh = run_k2m(torch, make_net(case), case)
    assert np.array_equal(bits, fresh)
    check(case, got)


def test_workspace_reuse_after_a_k2_call_with_more_slabs(gpu):
    """A forced K2 at B = 4096 fills 16 slabs of the shared partial sums, then K2m at B = 300 runs with two: the bits of a fresh
    net's call."""
    torch = gpu
    case = km.CaseM(km.BY_TAG["m_reuse_b300"])
    rng = np.random.default_rng(300)
    xb, gb = rng.uniform(-0.9, 1.5, size=(4096, case.D)).astype(np.float32), rng.normal(size=(4096, case.O)).astype(np.float32)
    assert k2.k2_plan(case.N, 4096, case.D, case.O, case.basis, False)["QSB"] == 16 and case.plan()["S"] == 2
    used = make_net(case)
    run_k2(torch, used, case, xb, gb)
    got, bits = run_k2m(torch, used, case)
    _, fresh = run_k2m(torch, make_net(case), case)
    assert np.array_equal(bits, fresh)
    check(case, got)


@pytest.mark.parametrize("tag", [s["tag"] for s in km.NONFINITE])
def test_non_finite_inputs(gpu, tag):
    """One NaN or +Inf cotangent element, or one NaN coordinate (ungated, or gated: gamma itself is NaN), at O = 18 and B = 130:
    the poison shares its MFMAs with the zero padding of g and W and with the zero tail records.  The non-finite elements are the
    reference's, everything else stays in bounds."""
    case, got, _, _ = run_case(gpu, tag)
    poison = case.spec["poison"]
    if poison == "nan_g":                               # g[17, 1]: column 1 of d kernel and d bias, every centre and width
        others = [o for o in range(case.O) if o != 1]
        assert np.isnan(got["kernel"][:, 1]).all() and np.isnan(got["bias"][1])
        assert np.isfinite(got["kernel"][:, others]).all() and np.isfinite(got["bias"][others]).all()
        assert np.isnan(got["centers"]).all() and np.isnan(got["log_sigs"]).all()
    elif poison in ("nan_x", "nan_xg"):                 # x[23, 3] ungated, x[23, 0] gated
        assert np.isnan(got["centers"]).all() and np.isnan(got["log_sigs"]).all() and np.isnan(got["kernel"]).all()
        assert np.isfinite(got["bias"]).all()
    else:                                               # g[40, 2] = +inf
        others = [o for o in range(case.O) if o != 2]
        assert (got["kernel"][:, 2] == np.inf).all() and got["bias"][2] == np.inf
        assert np.isfinite(got["kernel"][:, others]).all() and np.isfinite(got["bias"][others]).all()
        assert np.isinf(got["centers"]).all() and np.isinf(got["log_sigs"]).all()


@pytest.mark.parametrize("tag", [s["tag"] for s in km.ON_CENTRES])
def test_queries_on_centres(gpu, tag):
    case, got, _, _ = run_case(gpu, tag)
    cc = case.params["params"]["rbf_list"]["centers"]
    if not all((case.x[b] == cc[0, k]).all() for b, k in ((5, 3), (20, 17), (case.B - 1, case.K - 1))):
        pytest.fail(INPUTS + "the three queries are not centres")
    assert all(np.isfinite(got[leaf]).all() for leaf in k2.LEAVES)


REFUSED = {
    "two_regions": k2._reg("m_refused_r2", (2, 1), 3, 33, 5, "gaussian", 70),
    "generic_basis": k2._one("m_refused_generic", 4, 33, 20, "multiquadric", 70),
    "o16": k2._one("m_refused_o16", 4, 16, 20, "gaussian", 70),
    "o129": k2._one("m_refused_o129", 4, 129, 20, "gaussian", 70),            # no compiled output padding: the descriptor refuses
    "d9": k2._one("m_refused_d9", 9, 33, 20, "gaussian", 70),                 # no compiled padded D: the descriptor refuses
    "cluster": k2._clu("m_refused_cluster", 4, 10, 1, 20, "gaussian", 70),    # caller-provided region weights (and O <= 16)
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_refusals_leave_the_output_untouched(gpu, what):
    torch = gpu
    case = k2.Case(REFUSED[what])
    guarded.vjp_refused(torch, case, _lib.VJP_K2M)
    if what in ("two_regions", "generic_basis", "o16"):      # K2 takes the same net
        net = make_net(case)
        assert _lib.load().irbfn_net_vjp_kernel_supported(net._handle(torch), _lib.VJP_K2M, case.B) == 0
        assert _lib.load().irbfn_net_vjp_kernel_supported(net._handle(torch), _lib.VJP_K2, case.B) == 1
