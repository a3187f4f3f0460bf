"""K2h (`rbf_vjp_f16mfma<DC, BC, 2>`, rbf_vjp_f16.hip) on its own: the block pre-pass, the kernel and the shared slab reduce and bias
column sums against the float64 restatement of tests/_k2_util.py, at the edges of its shapes -- every padded D and O, centre counts
around the 16-centre tile, the 32-centre block and the 64-centre group, the five eligible bases, batches that leave waves without
a query block, a last block of one query, an odd number of blocks per wave, a reused workspace, operands at the ends of the
documented range of an (hi, lo) pair, a scaled cotangent and non-finite inputs.  The cases are tests/_k2h_util.py::TABLE.

K2h is forced (vjp_kernel = VJP_K2H) at B >= 2048; below, the option is a preference and K2 runs.  K2h records no launch name: a
one-row forward goes first and its name must still stand after the VJP (K2, K2g and K2m would each have recorded their own), and
once per net a forced K2 must differ from the result in some bit.  Every run writes the leaves into views of one NaN-filled buffer
with 64 guard words around each and runs twice: the two buffers must be bit-identical and the guards still NaN.  A test states
the slices, grid and idle waves it is about from the restated rules (k2h_plan).

Bounds, on every leaf (tests/_k2h_util.py): max|got - ref| <= 5e-5 max|ref| + 1e-7, and element-wise |got - ref| <= C_H S + 1e-30
with S the sum of the absolute per-query terms of that element and C_H = 4 x the worst error of the float32 restatement with K2h's
operand pairs (1.36e-6).  Each run prints, per leaf, the kernel's and that yardstick's worst |err| / S and the kernel's max-norm
ratio (profiles/k2h_parity.txt)."""
import numpy as np
import pytest

import _k2_util as k2
import _k2h_util as kh
import _vjp_guard_util as guarded
from _vjp_guard_util import make_net
from irbfn_amd import _lib

pytestmark = pytest.mark.gpu


def run_k2h(torch, net, case, x=None, g=None, option=_lib.VJP_K2H, distinct=False):
    """Two guarded runs of a forced K2h behind a one-row forward whose name must stand -> (leaves, bits).  distinct: the
    precondition that a forced K2 gives other bits on these inputs."""
    xs = case.x if x is None else x
    assert xs.shape[0] >= 2048
    assert _lib.load().irbfn_net_vjp_kernel_supported(net._handle(torch), _lib.VJP_K2H, xs.shape[0]) == 1
    net.apply(case.params, torch.from_numpy(np.ascontiguousarray(xs[:1])).cuda())
    fwd = net.last_launch()
    assert fwd["kernel"].startswith("rbf_fwd_"), fwd

    def expect(launch):
        assert launch == fwd, (case.tag, "a VJP kernel with a name of its own ran", launch)

    got, bits = guarded.run_twice(torch, net, case, expect, x, g, option)
    if distinct:
        _, launch, other = guarded.vjp_guarded(torch, net, case, x, g, _lib.VJP_K2)
        assert launch["kernel"].startswith("rbf_vjp_kernel<"), launch
        if np.array_equal(bits, other):
            pytest.fail(f"test inputs, not the code under test: {case.tag}: K2 and K2h give bit-identical leaves, the case distinguishes nothing")
    return got, bits


def check(case, got):
    """Both bounds on the four leaves; non-finite elements exactly where the reference has them."""
    ref, yard = case.reference(), case.yardstick_h()
    bad = []
    for leaf in k2.LEAVES:
        r, S = ref[leaf]
        assert got[leaf].dtype == np.float32 and got[leaf].shape == r.shape
        ys, _ = kh.ratios_h(yard[leaf], r, S)
        if ys > 5e-5:
            pytest.fail(f"test inputs, not the code under test: {case.tag} {leaf} needs {ys:.2e} S in float32 with the operand pairs")
        es, em = kh.ratios_h(got[leaf], r, S)
        print(f"K2HPARITY {case.tag:24s} {leaf:9s} kernel {es:.2e}  yardstick {ys:.2e}  max-norm ratio {em:.3f}")
        if not kh.same_nonfinite(got[leaf], r):
            bad.append(f"{leaf}: non-finite elements differ from the reference's ({int(np.isnan(got[leaf]).sum())} NaN, "
                       f"{int(np.isinf(got[leaf]).sum())} Inf of {got[leaf].size}; reference {int(np.isnan(r).sum())}, {int(np.isinf(r).sum())})")
        if not es <= kh.C_H:
            bad.append(f"{leaf}: |err| / S {es:.2e} > {kh.C_H:.2e}")
        if not em <= 1.0:
            bad.append(f"{leaf}: max-norm ratio {em:.3f}")
    assert not bad, (case.tag, bad)
    return ref


def run_case(torch, tag, distinct=True):
    case = kh.CaseH(kh.BY_TAG[tag])
    got, _ = run_k2h(torch, make_net(case), case, distinct=distinct)
    return case, got, check(case, got)


@pytest.mark.parametrize("tag", [s["tag"] for s in kh.SHAPES])
def test_padded_shapes_bases_and_gates(gpu, tag):
    case, _, _ = run_case(gpu, tag)
    p, spec = case.plan(), case.spec
    assert p["grid"] == (-(-case.N // 32), p["S"]) and p["DC"] == k2.padded_D(case.D) and p["RFQ"] == {3: 4, 4: 8, 7: 8, 8: 12}[p["DC"]]
    assert p["S"] == 9 and p["bpw"] == 2 and p["empty_waves"] in (2, 3) and p["last_block_queries"] == case.B - 32 * (p["nqb"] - 1)
    assert spec["ns"] == case.ns <= case.D


def test_a_region_without_a_range_row_gets_exact_zeros(gpu):
    """The weight of the only region is 0 for every query: K2 and K2h cannot differ, so the standing forward name alone says
    which ran."""
    case, got, ref = run_case(gpu, "h_norange", distinct=False)
    assert all((got[leaf] == 0).all() for leaf in ("centers", "log_sigs", "kernel")) and (got["bias"] != 0).all()


EDGE = {2048: (8, 2, 0, 2, 32), 2049: (9, 2, 3, 1, 1), 2079: (9, 2, 3, 1, 31), 2080: (9, 2, 3, 1, 32), 2081: (9, 2, 3, 2, 1),
        2304: (9, 2, 0, 2, 32), 2305: (10, 2, 3, 1, 1), 4097: (17, 2, 3, 1, 1)}


@pytest.mark.parametrize("B", kh.BATCH_EDGES)
def test_batch_edges(gpu, B):
    """N = 100: a grid of 4 x S blocks.  Slices, blocks per wave, waves without a block, blocks of the last working wave (one: its
    ring ends on the first half), queries of the last block."""
    case, _, _ = run_case(gpu, f"h_b{B}")
    p = case.plan()
    assert (p["S"], p["bpw"], p["empty_waves"], p["last_wave_blocks"], p["last_block_queries"]) == EDGE[B] and p["grid"] == (4, p["S"])


@pytest.mark.parametrize("B", kh.BIG_EDGES)
def test_three_blocks_per_wave_and_eighteen_idle_waves(gpu, B):
    """N = 3072: K2h's own rule caps the slices (q = 16 < QSB = 17, 18); an odd number of blocks per wave, the last working wave with
    one block (B = 4352) or two, the second of one query (4353)."""
    case, _, _ = run_case(gpu, f"h_n3072_b{B}")
    p = case.plan()
    assert (p["q"], p["QSB"], p["S"], p["bpw"], p["empty_waves"]) == (16, 17 if B == 4352 else 18, 16, 3, 18) and p["grid"] == (96, 16)
    assert (p["last_wave_blocks"], p["last_block_queries"]) == ((1, 32) if B == 4352 else (2, 1))


def test_below_2048_queries_the_option_is_a_preference(gpu):
    torch = gpu
    case = kh.CaseH(dict(kh.BY_TAG["h_b2048"], tag="h_b2047", B=2047))
    net = make_net(case)
    assert _lib.load().irbfn_net_vjp_kernel_supported(net._handle(torch), _lib.VJP_K2H, 2047) == 1
    _, launch, bits = guarded.vjp_guarded(torch, net, case, option=_lib.VJP_K2H)
    assert launch["kernel"].startswith("rbf_vjp_kernel<"), launch
    _, launch2, forced = guarded.vjp_guarded(torch, net, case, option=_lib.VJP_K2)
    assert launch2 == launch and np.array_equal(bits, forced)


def test_workspace_reuse_after_a_larger_batch(gpu):
    """B = 4352 (17 slices), then B = 2049 (9) on the same net and workspace: the bits of a fresh net's B = 2049 call."""
    torch = gpu
    case = kh.CaseH(kh.BY_TAG["h_reuse_b2049"])
    rng = np.random.default_rng(4352)
    xb, gb = rng.uniform(-0.9, 1.5, size=(4352, case.D)).astype(np.float32), rng.normal(size=(4352, case.O)).astype(np.float32)
    assert kh.k2h_plan(case.N, 4352, case.D, case.O, case.basis)["S"] == 17 and case.plan()["S"] == 9
    used = make_net(case)
    run_k2h(torch, used, case, xb, gb)
    got, bits = run_k2h(torch, used, case, distinct=True)
    _, fresh = run_k2h(torch, make_net(case), case)
    assert np.array_equal(bits, fresh)
    check(case, got)


@pytest.mark.parametrize("tag", ["h_wcols_spread", "h_grows_spread", "h_zero_col", "h_on_centres", "h_outside"])
def test_operands_at_the_ends_of_the_documented_range(gpu, tag):
    case, got, ref = run_case(gpu, tag)
    assert all(np.isfinite(got[leaf]).all() for leaf in k2.LEAVES)
    if tag == "h_zero_col":
        assert (got["kernel"][:, 1] != 0).any()                # d kernel of a zero column is (gamma phi)^T g all the same
    if tag == "h_on_centres":
        cc = case.params["params"]["rbf_list"]["centers"]
        if not all((case.x[b] == cc[0, k]).all() for b, k in ((5, 3), (20, 17), (case.B - 1, case.K - 1))):
            pytest.fail("test inputs, not the code under test: the three queries are not centres")
    if tag == "h_outside":
        if not (case.gamma()[::3] == 0).all():
            pytest.fail("test inputs, not the code under test: a query 1e3 outside the box has a weight")


def test_zero_kernel_and_zero_cotangent_give_exact_zeros(gpu):
    """All weights zero: every column scale is 1, hbar = 0, d centers and d log_sigs exact zeros.  All cotangents zero: the batch
    scale is 1 and every leaf an exact zero -- K2 gives the same bits there, so the precondition runs on the net's drawn batch."""
    torch = gpu
    case, got, _ = run_case(torch, "h_zero_kernel")
    assert (got["centers"] == 0).all() and (got["log_sigs"] == 0).all() and (got["kernel"] != 0).any()
    case = kh.CaseH(kh.BY_TAG["h_zero_g"])
    net = make_net(case)
    drawn = k2.Case(kh.BY_TAG["h_zero_g"]).g
    assert (drawn != 0).all()
    run_k2h(torch, net, case, g=drawn, distinct=True)
    got, _ = run_k2h(torch, net, case)
    check(case, got)
    assert all((got[leaf] == 0).all() for leaf in k2.LEAVES)


@pytest.mark.parametrize("tag", [s["tag"] for s in kh.SCALING])
def test_a_cotangent_scaled_by_a_power_of_two_scales_every_bit(gpu, tag):
    """Both operand scales are powers of two taken from the batch: vjp(x, 2^k g) is 2^k vjp(x, g) in every bit."""
    torch = gpu
    case = kh.CaseH(kh.BY_TAG[tag])
    net = make_net(case)
    got, _ = run_k2h(torch, net, case, distinct=True)
    check(case, got)
    for k in (-20, 20):
        scaled, _ = run_k2h(torch, net, case, g=np.ldexp(case.g, k))
        for leaf in k2.LEAVES:
            want = np.ldexp(got[leaf], k)
            assert np.isfinite(want).all() and (np.abs(want[want != 0]) >= 2.0 ** -100).all()           # no under- or overflow in the way
            diff = scaled[leaf].view(np.uint32) != want.view(np.uint32)
            assert not diff.any(), (tag, k, leaf, int(diff.sum()), scaled[leaf][diff][:4], want[diff][:4])


@pytest.mark.parametrize("tag", [s["tag"] for s in kh.NONFINITE])
def test_non_finite_inputs(gpu, tag):
    """One NaN or +Inf cotangent element, or one NaN coordinate, in a batch whose every column holds a finite |g| >= 2: the
    non-finite elements are the reference's, everything else stays in bounds.  (With the batch scale taken from a maximum that
    NaN and Inf won, the batch was packed unscaled and every finite |g| >= 2 overflowed its f16 pair: nan_g returned all 210
    elements of d kernel as NaN instead of column 1's 70, inf_g NaN in all of d kernel, d centers and d log_sigs where the reference
    has +Inf in column 2, finite columns beside it and +-Inf in the other two leaves.  profiles/k2h_parity.txt.)"""
    case = kh.CaseH(kh.BY_TAG[tag])
    if not (np.abs(np.nan_to_num(case.g, nan=0.0, posinf=0.0)).max(axis=0) >= 2).all():
        pytest.fail("test inputs, not the code under test: a cotangent column without an element of |g| >= 2")
    got, _ = run_k2h(gpu, make_net(case), case, distinct=True)
    check(case, got)
    poison = case.spec["poison"]
    if poison == "nan_g":                               # g[17, 1]: column 1 of d kernel and d bias, every centre and width
        others = [o for o in range(case.O) if o != 1]
        assert np.isnan(got["kernel"][:, 1]).all() and np.isnan(got["bias"][1])
        assert np.isfinite(got["kernel"][:, others]).all() and np.isfinite(got["bias"][others]).all()
        assert np.isnan(got["centers"]).all() and np.isnan(got["log_sigs"]).all()
    elif poison == "nan_x":                             # x[23, 3], an ungated coordinate
        assert np.isnan(got["centers"]).all() and np.isnan(got["log_sigs"]).all() and np.isnan(got["kernel"]).all()
        assert np.isfinite(got["bias"]).all()
    else:                                               # g[40, 2] = +inf
        others = [o for o in range(case.O) if o != 2]
        assert (got["kernel"][:, 2] == np.inf).all() and got["bias"][2] == np.inf
        assert np.isfinite(got["kernel"][:, others]).all() and np.isfinite(got["bias"][others]).all()
        assert np.isinf(got["centers"]).all() and np.isinf(got["log_sigs"]).all()
