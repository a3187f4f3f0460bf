"""K2g (`rbf_vjp_f16gram<DC, BC, OC, MODE>`, rbf_vjp_gram.hip) on its own: the block pre-pass, the kernel, the hand-over to K2h
and the shared slab reduce against the float64 restatement of tests/_k2_util.py, at the edges of its shapes -- every padded D, O on
both sides of the switch of hbar from one MFMA to two, centre counts around the 16-centre tile, the 32-centre chunk and the
128-centre block, the five eligible bases, last slices of 1, 2, 3 and 4 query blocks around the three-slot LDS ring, empty slices,
the frozen-leaf modes, a reused workspace, operands at the ends of the documented ranges, a scaled cotangent, every way a call is
handed over to K2h, the 64-word ring of the hand-over flag, and the refusals.  The cases are tests/_k2g_util.py::TABLE.

Which kernel computed: the launch name `rbf_vjp_f16gram<` is recorded before the device decides.  Behind a raised flag K2h runs
with K2g's slices; where K2h's own rule gives the same number (asserted from the restated plans), a forced VJP_K2H call has the
bits of a call K2g handed over, and a call K2g computed must differ from it in some bit.  Every run writes the leaves into views
of one NaN-filled buffer with 64 guard words around each and runs twice: bit-identical, the guards still NaN.

Bounds, on every leaf (tests/_k2g_util.py): max|got - ref| <= 5e-5 max|ref| + 1e-7, and element-wise |got - ref| <= C_G S + A +
1e-30 with S the sum of the absolute per-query terms, A the absolute floor K2g documents and C_G = 4 x the worst error of the
float32 restatement with K2g's operand treatment.  A handed-over call is held to K2h's bound C_H S instead.  Each run prints, per
leaf, the kernel's and the yardstick's worst (|err| - A)+ / S and the kernel's max-norm ratio (profiles/k2g_parity.txt)."""
import numpy as np
import pytest

import _k2_util as k2
import _k2h_util as kh
import _k2g_util as kg
import _vjp_guard_util as guarded
from _vjp_guard_util import make_net
from irbfn_amd import _lib
from irbfn_amd.model import WCRBFNet

pytestmark = pytest.mark.gpu
NOTHING = "test inputs, not the code under test: {}: K2g and the forced K2h give bit-identical leaves, the case distinguishes nothing"


def supported(torch, net, option, B):
    return _lib.load().irbfn_net_vjp_kernel_supported(net._handle(torch), option, B)


def same_slabs(case, B=None):
    B = case.B if B is None else B
    return kg.k2g_plan(case.N, B, case.D, case.O, case.basis)["S"] == kh.k2h_plan(case.N, B, case.D, case.O, case.basis)["S"]


def forced_k2h(torch, net, case, x=None, g=None):
    """The bits of a forced K2h call; K2h records no name, so the one that stood before must still stand."""
    before = net.last_launch()
    _, launch, bits = guarded.vjp_guarded(torch, net, case, x, g, _lib.VJP_K2H)
    assert launch == before, (case.tag, "the forced K2h recorded a name", launch)
    return bits


def run_k2g(torch, net, case, x=None, g=None, computed=True, option=_lib.VJP_K2G):
    """Two guarded runs under VJP_K2G -> (leaves, bits).  computed: True -- K2g did the work: the bits differ from a forced K2h's;
    False -- it handed over: they are the forced K2h's; None -- not asked (exact zeros, or K2h would run with other slices)."""
    B = (case.x if x is None else x).shape[0]
    net.bind(case.params)                                       # the pack's verdict is part of the answer
    assert B >= 2048 and supported(torch, net, _lib.VJP_K2G, B) == 1

    def expect(launch):
        assert launch["kernel"].startswith("rbf_vjp_f16gram<"), (case.tag, launch)

    got, bits = guarded.run_twice(torch, net, case, expect, x, g, option)
    if computed is not None:
        assert same_slabs(case, B), (case.tag, "K2h alone would run with other slices: its bits say nothing here")
        other = forced_k2h(torch, net, case, x, g)
        if computed and np.array_equal(bits, other):
            pytest.fail(NOTHING.format(case.tag))
        if not computed:
            assert np.array_equal(bits, other), (case.tag, "a handed-over call differs from the forced K2h in some bit")
    return got, bits


def check(case, got, leaves=k2.LEAVES, yard=True):
    """Both bounds on the leaves; non-finite elements exactly where the reference has them."""
    ref, A = case.reference(), case.floor()
    y = case.yardstick_g() if yard else None
    bad = []
    for leaf in leaves:
        r, S = ref[leaf]
        assert got[leaf].dtype == np.float32 and got[leaf].shape == r.shape
        ys = kg.ratios_g(y[leaf], r, S, A[leaf])[0] if yard else float("nan")
        es, em = kg.ratios_g(got[leaf], r, S, A[leaf])
        print(f"K2GPARITY {case.tag:20s} {leaf:9s} kernel {es:.2e}  yardstick {ys:.2e}  max-norm ratio {em:.3f}")
        if not kg.same_nonfinite(got[leaf], r):
            bad.append(f"{leaf}: non-finite elements differ from the reference's ({int(np.isnan(got[leaf]).sum())} NaN, "
                       f"{int(np.isinf(got[leaf]).sum())} Inf of {got[leaf].size}; reference {int(np.isnan(r).sum())}, {int(np.isinf(r).sum())})")
        if not es <= kg.C_G:
            bad.append(f"{leaf}: (|err| - A)+ / S {es:.2e} > {kg.C_G:.2e}")
        if not em <= 1.0:
            bad.append(f"{leaf}: max-norm ratio {em:.3f}")
    assert not bad, (case.tag, bad)
    return ref


def check_h(case, got):
    """A handed-over call: K2h's own bounds (tests/_k2h_util.py)."""
    ref = case.reference()
    bad = []
    for leaf in k2.LEAVES:
        r, S = ref[leaf]
        es, em = kh.ratios_h(got[leaf], r, S)
        print(f"K2GPARITY {case.tag:20s} {leaf:9s} handed over {es:.2e}  max-norm ratio {em:.3f}")
        if not (kg.same_nonfinite(got[leaf], r) and es <= kh.C_H and em <= 1.0):
            bad.append(f"{leaf}: |err| / S {es:.2e} (C_H {kh.C_H:.2e}), max-norm ratio {em:.3f}, non-finite as the reference {kg.same_nonfinite(got[leaf], r)}")
    assert not bad, (case.tag, bad)


def run_case(torch, tag, computed=True):
    case = kg.CaseG(kg.BY_TAG[tag])
    got, _ = run_k2g(torch, make_net(case), case, computed=computed)
    return case, got, check(case, got)


# ------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("tag", [s["tag"] for s in kg.SHAPES])
def test_padded_shapes_bases_and_gates(gpu, tag):
    case, _, _ = run_case(gpu, tag)
    p, spec = case.plan(), case.spec
    assert (p["S"], p["bpb"], p["empty"]) == (9, 8, 0) and p["last_slice_blocks"] in (1, 2, 3) and p["grid"] == (-(-case.N // 128), 9)
    assert p["idle_waves"] == 4 * p["gb"] - (-(-case.N // 32)) and p["DC"] == k2.padded_D(case.D) and p["OC"] == (case.O <= 10)
    assert p["last_block_queries"] == case.B - 32 * (p["nqb"] - 1) and spec["ns"] == case.ns <= case.D


def test_a_region_without_a_range_row_gets_exact_zeros(gpu):
    """The weight of the only region is 0 for every query: K2g and K2h cannot differ."""
    case, got, _ = run_case(gpu, "g_norange", computed=None)
    assert all((got[leaf] == 0).all() for leaf in ("centers", "log_sigs", "kernel")) and (got["bias"] != 0).all()


# ------------------------------------------------------------------------------------------------ batch edges
#       B: S, bpb, working slices, empty slices, blocks of the last working slice, queries of the last block, bias blocks
EDGE = {2048: (8, 8, 8, 0, 8, 32, 32), 2049: (9, 8, 9, 0, 1, 1, 33), 2080: (9, 8, 9, 0, 1, 32, 33), 2081: (9, 8, 9, 0, 2, 1, 33),
        2113: (9, 8, 9, 0, 3, 1, 34), 2145: (9, 8, 9, 0, 4, 1, 34), 2305: (10, 8, 10, 0, 1, 1, 37), 16384: (64, 8, 64, 0, 8, 32, 256),
        16385: (64, 9, 57, 7, 9, 1, 256)}


@pytest.mark.parametrize("B", kg.BATCH_EDGES)
def test_batch_edges(gpu, B):
    """N = 100: one block of centres, S slices.  A last slice of 1, 2 or 3 blocks ends inside the ring's first round; of 4, its
    stage(0 + 3) is the first reuse of slot 0.  From 16385 queries seven slices find no block: their slabs must still be zeros.
    At 16385 K2h alone would cut 65 slices, so its bits say nothing there; the reference does."""
    case = kg.CaseG(kg.BY_TAG[f"g_b{B}"])
    p = case.plan()
    assert (p["S"], p["bpb"], p["working"], p["empty"], p["last_slice_blocks"], p["last_block_queries"], p["bias_blocks"]) == EDGE[B]
    assert p["grid"] == (1, p["S"]) and same_slabs(case) == (B != 16385)
    got, _ = run_k2g(gpu, make_net(case), case, computed=True if B != 16385 else None)
    check(case, got)


def _frozen(case, mode):
    rl = case.params["params"]["rbf_list"]
    kw = {"log_sigs": rl["log_sigs"]} if mode == "fixed_width" else {}
    net = WCRBFNet(**case.cfg, centers=rl["centers"], **{mode: True}, **kw)
    red = {"params": {"linear": case.params["params"]["linear"]}}
    if mode == "fixed_centers":
        red["params"]["rbf_list"] = {"log_sigs": rl["log_sigs"]}
    return net, red


@pytest.mark.parametrize("B", kg.FROZEN_EDGES)
@pytest.mark.parametrize("mode,suffix,m", [("fixed_centers", "/no_centres", 1), ("fixed_width", "/linear", 2)])
def test_frozen_modes_at_the_ring_edges(gpu, mode, suffix, m, B):
    """The frozen-leaf instances stage 10 and 7 of the 12 pieces of a block image, LINEAR with its pieces remapped: a last slice
    of one block and of four, the live leaves against the reference."""
    import torch
    case = kg.CaseG(kg.BY_TAG[f"g_b{B}"])
    p = case.plan(m)
    assert (p["S"], p["bpb"], p["last_slice_blocks"], p["pieces"]) == (9, 8, 1 if B == 2049 else 4, 10 if m == 1 else 7)
    net, red = _frozen(case, mode)
    net.set_options(vjp_kernel=_lib.VJP_K2G)
    try:
        xt, gt = torch.from_numpy(case.x).cuda(), torch.from_numpy(case.g).cuda()
        runs = [net.vjp(red, xt, gt)["params"] for _ in range(2)]
    finally:
        net.set_options(vjp_kernel=_lib.VJP_AUTO)
    assert net.last_launch()["kernel"].startswith("rbf_vjp_f16gram" + suffix + "<"), net.last_launch()
    live = [leaf for leaf in k2.LEAVES if not (leaf == "centers" or (m == 2 and leaf == "log_sigs"))]
    got = {}
    for leaf in live:
        grp, name = k2.LEAF_PATH[leaf]
        assert torch.equal(runs[0][grp][name], runs[1][grp][name]), (mode, B, leaf)
        got[leaf] = runs[0][grp][name].cpu().numpy()
    assert set(runs[0]) == {k2.LEAF_PATH[leaf][0] for leaf in live}
    check(case, got, leaves=live)


@pytest.mark.parametrize("O", [10, 11])
def test_seventeen_centre_blocks_with_one_active_wave_in_the_last(gpu, O):
    """N = 2049, B = 11777: 65 chunks in 17 blocks, the last block's waves 1 - 3 idle.  O = 10 runs 47 slices of 8 blocks (the last
    one block of one query), O = 11 46 slices of 9 of which five are empty.  The reference alone: no yardstick at this size."""
    case = kg.CaseG(kg.BY_TAG[f"g_n2049_o{O}"])
    p = case.plan()
    assert (p["gb"], p["idle_waves"], p["S"], p["bpb"], p["empty"], p["last_slice_blocks"], p["last_block_queries"]) == \
        ((17, 3, 47, 8, 0, 1, 1) if O == 10 else (17, 3, 46, 9, 5, 9, 1))
    got, _ = run_k2g(gpu, make_net(case), case, computed=None)
    check(case, got, yard=False)


def test_workspace_reuse_after_a_larger_batch_and_after_k2h(gpu):
    """B = 4352 (17 slices), then B = 2049 (9) on the same net and workspace: the bits of a fresh net's B = 2049 call.  Then a forced
    K2h call -- its block images lie where K2g's do (off_qblk) -- and K2g again: the same bits."""
    torch = gpu
    case = kg.CaseG(kg.BY_TAG["g_reuse_b2049"])
    rng = np.random.default_rng(4352)
    xb, gb = rng.uniform(-0.9, 1.5, size=(4352, case.D)).astype(np.float32), rng.normal(size=(4352, case.O)).astype(np.float32)
    assert kg.k2g_plan(case.N, 4352, case.D, case.O, case.basis)["S"] == 17 and case.plan()["S"] == 9
    used = make_net(case)
    run_k2g(torch, used, case, xb, gb)
    got, bits = run_k2g(torch, used, case)                    # ends with a forced K2h call on this workspace
    _, fresh = run_k2g(torch, make_net(case), case, computed=None)
    assert np.array_equal(bits, fresh)
    _, again = run_k2g(torch, used, case, computed=None)
    assert np.array_equal(again, fresh)
    check(case, got)


# ------------------------------------------------------------------------------------------------ operand ranges
@pytest.mark.parametrize("tag", ["g_wcols_gauss", "g_wcols_iq", "g_wcols_imq", "g_grows_spread", "g_zero_col", "g_on_centres", "g_far"])
def test_operands_at_the_ends_of_the_documented_range(gpu, tag):
    case, got, ref = run_case(gpu, tag)
    assert all(np.isfinite(got[leaf]).all() for leaf in k2.LEAVES)
    if tag == "g_zero_col":
        assert (got["kernel"][:, 1] != 0).any()
    if tag == "g_on_centres":
        cc = case.params["params"]["rbf_list"]["centers"]
        if not all((case.x[b] == cc[0, k]).all() for b, k in ((5, 3), (20, 17), (case.B - 1, case.K - 1))):
            pytest.fail("test inputs, not the code under test: the three queries are not centres")
    if tag == "g_far":                                          # phi below 2^-52: nothing of it reaches an ungained pair
        assert (got["kernel"] == 0).all() and (got["centers"] == 0).all() and (got["log_sigs"] != 0).all()


@pytest.mark.parametrize("option", ["K2G", "AUTO"])
@pytest.mark.parametrize("tag", [s["tag"] for s in kh.RANGES])
def test_k2h_s_range_cases_under_k2g_and_auto(gpu, tag, option):
    """What K2h meets on its operand-range cases, a forced K2g and the automatic choice meet as well, by computing or by handing
    over: the project's max-norm bound and the element-wise one with K2g's floor."""
    torch = gpu
    case = kg.CaseG(kh.BY_TAG[tag])
    net = make_net(case)
    if option == "K2G":
        got, _ = run_k2g(torch, net, case, computed=None)
    else:
        got, _, _ = guarded.vjp_guarded(torch, net, case, option=_lib.VJP_AUTO)
    if tag == "h_outside":
        check_h(case, got)
    else:
        check(case, got)


def test_zero_kernel_and_zero_cotangent_give_exact_zeros(gpu):
    torch = gpu
    case, got, _ = run_case(torch, "g_zero_kernel")
    assert (got["centers"] == 0).all() and (got["log_sigs"] == 0).all() and (got["kernel"] != 0).any()
    case = kg.CaseG(kg.BY_TAG["g_zero_g"])
    net = make_net(case)
    drawn = k2.Case(kg.BY_TAG["g_zero_g"]).g
    assert (drawn != 0).all()
    run_k2g(torch, net, case, g=drawn)                         # the precondition runs on the net's drawn batch
    got, _ = run_k2g(torch, net, case, computed=None)
    check(case, got)
    assert all((got[leaf] == 0).all() for leaf in k2.LEAVES)


@pytest.mark.parametrize("tag", [s["tag"] for s in kg.SCALING])
def test_a_cotangent_scaled_by_a_power_of_two_scales_every_bit(gpu, tag):
    """Both operand scales are powers of two taken from the batch: vjp(x, 2^k g) is 2^k vjp(x, g) in every bit."""
    torch = gpu
    case = kg.CaseG(kg.BY_TAG[tag])
    net = make_net(case)
    got, _ = run_k2g(torch, net, case)
    check(case, got)
    for k in (-20, 20):
        scaled, _ = run_k2g(torch, net, case, g=np.ldexp(case.g, k))
        for leaf in k2.LEAVES:
            want = np.ldexp(got[leaf], k)
            assert np.isfinite(want).all() and (np.abs(want[want != 0]) >= 2.0 ** -100).all()
            diff = scaled[leaf].view(np.uint32) != want.view(np.uint32)
            assert not diff.any(), (tag, k, leaf, int(diff.sum()), scaled[leaf][diff][:4], want[diff][:4])


# ------------------------------------------------------------------------------------------------ hand-over
def _hand(edit, **kw):
    case = kg.CaseG(dict(kg.BY_TAG["g_hand"], net="g_hand", **kw))
    r, lim = kg.box_limit(case.params["params"]["rbf_list"]["centers"][0])
    assert case.B == 2049 and case.plan()["last_block_queries"] == 1 and case.ns == 2 and lim == np.float32(1.998)
    edit(case, r)
    return case


def _edge(case, r, factor):
    """The last query -- alone in its block -- with its ungated coordinate 3 at r_3 + factor * 2^ex."""
    case.x[-1, 3] = np.float32(r[3] + np.float32(factor) * np.float32(2.0))
    return np.abs(np.float32(case.x[-1, 3] - r[3]))


HAND = {
    "outside_gate_1e3": lambda c, r: None,                                     # CaseH's `outside`: every third row 1e3 above the gate's box
    "last_query_outside": lambda c, r: _edge(c, r, 1.0),
    "nan_coordinate": lambda c, r: c.x.__setitem__((100, 2), np.nan),
    "posinf_coordinate": lambda c, r: c.x.__setitem__((200, 3), np.inf),
    "neginf_coordinate": lambda c, r: c.x.__setitem__((300, 2), -np.inf),
}


@pytest.mark.parametrize("what", sorted(HAND))
def test_a_query_outside_the_box_hands_the_call_to_k2h(gpu, what):
    """One coordinate of one query outside the expansion's box -- 1e3 above the gate's box, just past the limit in the single
    query of the last block, NaN, +Inf, -Inf -- raises the flag: the call has the bits of a forced K2h and meets K2h's bound."""
    case = _hand(HAND[what], tag=f"g_hand_{what}", **({"outside": True} if what == "outside_gate_1e3" else {}))
    if what == "last_query_outside":
        r, lim = kg.box_limit(case.params["params"]["rbf_list"]["centers"][0])
        assert np.abs(np.float32(case.x[-1, 3] - r[3])) >= lim and (np.abs(case.x[:-1] - r[None]) < lim).all()
    got, _ = run_k2g(gpu, make_net(case), case, computed=False)
    check_h(case, got)


def test_a_query_just_inside_the_box_does_not_hand_over(gpu):
    """|x' _3| = 0.998 * 2^ex in the single query of the last block: below the limit 0.999 * 2^ex of gram_query_parts, K2g computes."""
    case = _hand(lambda c, r: None, tag="g_hand_inside")
    r, lim = kg.box_limit(case.params["params"]["rbf_list"]["centers"][0])
    d = _edge(case, r, 0.998)
    assert np.float32(0.997) * 2 < d < lim
    got, _ = run_k2g(gpu, make_net(case), case, computed=True)
    check(case, got)


@pytest.mark.parametrize("poison", ["nan_g", "inf_g"])
def test_a_non_finite_cotangent_hands_the_call_to_k2h(gpu, poison):
    """The operand pairs of K2g cannot carry a NaN or an infinity through the sums: the pre-pass hands the call over, and the
    non-finite elements are the reference's, column by column, as for K2h (tests/test_gpu_k2h.py::test_non_finite_inputs)."""
    case = kg.CaseG(kg.BY_TAG[f"g_nonfinite_{poison}"])
    if not (np.abs(np.nan_to_num(case.g, nan=0.0, posinf=0.0)).max(axis=0) >= 2).all():
        pytest.fail("test inputs, not the code under test: a cotangent column without an element of |g| >= 2")
    got, _ = run_k2g(gpu, make_net(case), case, computed=False)
    check_h(case, got)
    col = 1 if poison == "nan_g" else 2
    others = [o for o in range(case.O) if o != col]
    assert np.isfinite(got["kernel"][:, others]).all() and np.isfinite(got["bias"][others]).all()
    if poison == "nan_g":
        assert np.isnan(got["kernel"][:, 1]).all() and np.isnan(got["bias"][1])
        assert np.isnan(got["centers"]).all() and np.isnan(got["log_sigs"]).all()
    else:
        assert (got["kernel"][:, 2] == np.inf).all() and got["bias"][2] == np.inf
        assert np.isinf(got["centers"]).all() and np.isinf(got["log_sigs"]).all()


def test_the_flag_ring_of_64_generations(gpu):
    """70 consecutive K2g calls on one net: call n raises word n % 64 to n when it hands over, nobody resets a word.  Calls 3 and 67
    hand over and share word 3; every other call finds a stale generation there or elsewhere and must compute."""
    torch = gpu
    case = kg.CaseG(kg.BY_TAG["g_ring"])
    assert (case.N, case.B) == (40, 2049) and same_slabs(case)
    net = make_net(case)
    xo = case.x.copy()
    xo[77, 2] = np.float32(1.0e3)                              # an ungated coordinate far outside the box
    assert case.ns == 1
    net.apply(case.params, torch.from_numpy(case.x[:1]).cuda())
    k2h_clean, k2h_out = forced_k2h(torch, net, case), forced_k2h(torch, net, case, x=xo)
    first = None
    for n in range(1, 71):
        out = n in (3, 67)
        _, launch, bits = guarded.vjp_guarded(torch, net, case, x=xo if out else None, option=_lib.VJP_K2G)
        assert launch["kernel"].startswith("rbf_vjp_f16gram<"), launch
        if out:
            assert np.array_equal(bits, k2h_out), (n, "the call did not hand over")
            continue
        first = bits if first is None else first
        assert np.array_equal(bits, first), (n, "a clean call differs from call 1")
    if np.array_equal(first, k2h_clean):
        pytest.fail(NOTHING.format(case.tag))
    got, _ = run_k2g(torch, net, case)                          # calls 71, 72: still computing, still in bounds
    check(case, got)


# ------------------------------------------------------------------------------------------------ refusals
def _refused(torch, case, B=None):
    net = make_net(case)
    net.bind(case.params)
    B = case.B if B is None else B
    assert supported(torch, net, _lib.VJP_K2G, B) == 0, case.tag
    net.set_options(vjp_kernel=_lib.VJP_K2G)
    try:
        with pytest.raises(ValueError, match="UNSUPPORTED"):
            net.vjp(case.params, torch.from_numpy(case.x[:B]).cuda(), torch.from_numpy(case.g[:B]).cuda())
    finally:
        net.set_options(vjp_kernel=_lib.VJP_AUTO)


def test_refusals(gpu):
    """VJP_K2G is no preference: below 2048 queries, above 16 outputs, on a generic basis, on two regions, and on a net the pack's
    verdict rejects -- widths of 1e-3, or a single centre, whose box is a point -- the query and the forced call refuse."""
    torch = gpu
    base = kg.BY_TAG["g_b2049"]
    _refused(torch, kg.CaseG(base), B=2047)
    assert supported(torch, make_net(kg.CaseG(base)), _lib.VJP_K2G, 2047) == 0
    _refused(torch, kg.CaseG(dict(base, tag="g_o17", O=17)))
    _refused(torch, kg.CaseG(dict(base, tag="g_generic", basis="multiquadric")))
    _refused(torch, k2.Case(k2._reg("g_two_regions", (2, 1), 3, 5, 50, "gaussian", 2049)))
    narrow = kg.CaseG(dict(base, tag="g_narrow"))
    ls = narrow.params["params"]["rbf_list"]["log_sigs"]
    ls[:] = -7.0
    ls[0, :32] = 0.5
    _refused(torch, narrow)
    one = kg.CaseG(kg.ONE_CENTRE)
    assert kg.header(one.params["params"]["rbf_list"]["centers"][0])[2] == 0.0
    _refused(torch, one)
    ok = make_net(kg.CaseG(base))
    ok.bind(kg.CaseG(base).params)
    assert supported(torch, ok, _lib.VJP_K2G, 2049) == 1 and supported(torch, ok, _lib.VJP_K2G, 2048) == 1
