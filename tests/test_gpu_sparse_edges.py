"""The region-sparse kernels (rbf_sparse.hip: K1r `rbf_fwd_sparse`, its tick, the pair-list pass, the scan and K2r `rbf_vjp_sparse`)
at their list and shape edges, on the tiny nets of tests/_sparse_util.py::TABLE -- every padded D and O, the second index word of the
gate, the five fast bases and two generic ones, region counts around a hit word, a transposed mask and the 16-bit lists, lists at
their capacity, queries on the float32 neighbours of the gate's exact zero, rows of dimension_ranges that repeat, region lists
longer than two register chunks, every number of search steps, a block without pairs inside a region's list, a reused workspace,
non-finite inputs, the tick's other instances, and the set-up's limits from both sides.

Every forward goes through _small_util.forward_guarded (NaN rows behind row B) under the forced K1r and the forced dense K1 and
states the launch it expects (_sparse_util.k1r_launch).  Bounds (tests/_sparse_util.py): the forward element-wise against the float64
reference with the kernels' exact zeros and against K1; every element of every gradient leaf within C_S S of the float64 reference,
for K2r and for the dense K2 on the same case, plus the max-norm bound; K2r twice with identical bits.  Each run prints a line
`SPARSEPARITY ...` (profiles/sparse_parity.txt)."""
import numpy as np
import pytest

import _k2_util as k2
import _sparse_util as su
from _small_util import forward_guarded
from irbfn_amd import _lib, configs, dynamics, planner
from irbfn_amd.model import WCRBFNet

pytestmark = pytest.mark.gpu

_CARDS = {}


def card(tag):
    if tag not in _CARDS:
        _CARDS[tag] = su.Card(su.BY_TAG[tag])
    return _CARDS[tag]


def tags(group):
    return [s["tag"] for s in group]


# ------------------------------------------------------------------------------------------------ forward
def forward_both(c, net=None, x=None):
    """K1r and K1 on x (default: the case's batch): the launches are the restated ones, the guard rows untouched."""
    net = net or WCRBFNet.from_config(c.cfg)
    x = c.x if x is None else x
    sp, launch = forward_guarded(net, c.params, x, _lib.FWD_K1R)
    assert launch == su.k1r_launch(c.cfg, len(x)), (c.tag, launch)
    dn, dense = forward_guarded(net, c.params, x, _lib.FWD_K1)
    assert dense["kernel"].startswith("rbf_fwd_qlane<") and "GATED=1" in dense["kernel"], (c.tag, dense)
    return sp, dn


def check_forward(c, sp, dn, ref=None, scale=None):
    if ref is None:
        ref, scale = c.forward_reference()
    assert sp.shape == ref.shape and sp.dtype == np.float32
    if c.basis not in k2.FAST:
        e = float(np.abs(sp - ref).max() / np.abs(ref).max())
        ed = float(np.abs(sp.astype(np.float64) - dn).max() / np.abs(ref).max())
        print(f"SPARSEPARITY {c.tag:22s} forward  max|err|/max|ref| {e:.2e}, against K1 {ed:.2e} (bound 2e-5)")
        assert e <= 2e-5 and ed <= 2e-5, c.tag
        return
    e = float((np.abs(sp - ref) / (1e-5 * np.abs(ref) + 3e-6 * scale)).max())
    ed = float((np.abs(sp.astype(np.float64) - dn) / (2e-6 * scale + 1e-7 * np.abs(ref))).max())
    print(f"SPARSEPARITY {c.tag:22s} forward  err/bound {e:.3f}, against K1 {ed:.3f} of its bound")
    assert e <= 1.0 and ed <= 1.0, (c.tag, e, ed)


# ------------------------------------------------------------------------------------------------ VJP
def vjp(torch, net, c, option, x=None, g=None):
    """-> ({leaf: float32 array}, the kernel name standing after the call).  A one-row forward goes first (K1s under AUTO): K2r
    records no name and leaves that one standing."""
    xt = torch.from_numpy(c.x if x is None else x).cuda()
    gt = torch.from_numpy(c.g if g is None else g).cuda()
    net.apply(c.params, xt[:1].contiguous())
    net.set_options(vjp_kernel=option)
    try:
        got = net.vjp(c.params, xt, gt)["params"]
    finally:
        net.set_options(vjp_kernel=_lib.VJP_AUTO)
    return {n: got[a][b].cpu().numpy() for n, (a, b) in su.LEAF_PATH.items()}, net.last_launch()["kernel"]


def same_bits(a, b):
    return all(np.array_equal(a[n].view(np.uint32), b[n].view(np.uint32)) for n in su.LEAVES)


def supported(torch, net, option, B):
    return _lib.load().irbfn_net_vjp_kernel_supported(net._handle(torch), option, B)


def check_leaves(c, got, ref, which):
    bad = []
    for leaf in su.LEAVES:
        r, S = ref[leaf]
        assert got[leaf].dtype == np.float32 and got[leaf].shape == r.shape
        es, em = su.ratios(got[leaf], r, S)
        print(f"SPARSEPARITY {c.tag:22s} {which:3s} {leaf:9s} |err|/S {es:.2e} (C_S {su.C_S:.2e}, r32 {su.R32:.1e})  max-norm ratio {em:.3f}")
        if not k2.same_nonfinite(got[leaf], r):
            bad.append(f"{which} {leaf}: non-finite elements differ from the reference's")
        if not es <= su.C_S:
            bad.append(f"{which} {leaf}: |err| / S {es:.2e} > {su.C_S:.2e}")
        if not em <= 1.0:
            bad.append(f"{which} {leaf}: max-norm ratio {em:.3f}")
    return bad


def check_vjp(torch, c, net=None):
    """K2r (twice, identical bits) and K2 on the case, both within the bounds -> K2r's leaves."""
    net = net or WCRBFNet.from_config(c.cfg)
    net.bind(c.params)
    SL = su.vjp_slices(c.cfg, c.B)
    Lr = c.live().sum(axis=0)
    longest = max(b - a for n in Lr for a, b in su.slice_bounds(int(n), SL))
    s = su.setup(c.cfg)
    print(f"SPARSEPARITY {c.tag:22s} plan     E {s['E']} cap {s['cap']} SL {SL} longest slice {longest} pairs {int(Lr.sum())}")
    assert su.vjp_eligible(c.cfg) and su.vjp_lds_fits(c.cfg) and supported(torch, net, _lib.VJP_K2R, c.B) == 1, c.tag
    a, name = vjp(torch, net, c, _lib.VJP_K2R)
    assert not name.startswith("rbf_vjp_kernel<"), (c.tag, name)
    b, _ = vjp(torch, net, c, _lib.VJP_K2R)
    assert same_bits(a, b), f"{c.tag}: two runs of K2r differ in some bit"
    d, name = vjp(torch, net, c, _lib.VJP_K2)
    assert name.startswith("rbf_vjp_kernel<") and "GATED=1" in name, (c.tag, name)
    ref = c.reference()
    bad = check_leaves(c, a, ref, "K2r") + check_leaves(c, d, ref, "K2")
    assert not bad, (c.tag, bad)
    return a


def run_case(torch, tag):
    c = card(tag)
    net = WCRBFNet.from_config(c.cfg)
    check_forward(c, *forward_both(c, net))
    return c, check_vjp(torch, c, net)


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("tag", tags(su.INSTANCES))
def test_compiled_instances(gpu, tag):
    run_case(gpu, tag)


@pytest.mark.parametrize("tag", tags(su.GENERIC))
def test_generic_bases_run_the_forward_and_refuse_k2r(gpu, tag):
    torch = gpu
    c = card(tag)
    net = WCRBFNet.from_config(c.cfg)
    check_forward(c, *forward_both(c, net))
    net.bind(c.params)
    assert supported(torch, net, _lib.VJP_K2R, c.B) == 0
    with pytest.raises(ValueError, match="UNSUPPORTED"):
        vjp(torch, net, c, _lib.VJP_K2R)
    auto, name = vjp(torch, net, c, _lib.VJP_AUTO)
    dense, name2 = vjp(torch, net, c, _lib.VJP_K2)
    assert name == name2 and name.startswith("rbf_vjp_kernel<") and same_bits(auto, dense), (name, name2)


@pytest.mark.parametrize("tag", tags(su.REGION_COUNTS))
def test_region_counts(gpu, tag):
    c, got = run_case(gpu, tag)
    if tag == "nr12_of_16":                                      # regions without a row: exact zeros
        assert not got["centers"][12:].any() and not got["log_sigs"][12:].any() and got["centers"][:12].any(axis=(1, 2)).all()


@pytest.mark.parametrize("tag", tags(su.CAPACITY))
def test_lists_at_their_capacity(gpu, tag):
    c, got = run_case(gpu, tag)
    if tag == "repeated_rows":                                   # rows 4 and 5 repeat rows 2 and 1: live, not dropped
        assert got["centers"][4:].any(axis=(1, 2)).all()


@pytest.mark.parametrize("tag", tags(su.LISTS))
def test_region_lists(gpu, tag):
    run_case(gpu, tag)


def test_workspace_reuse(gpu):
    """B = 3000, then 70, then 3000 on one net and workspace: the third result has the bits of the first, the second those of a
    fresh net."""
    torch = gpu
    big, small = card("reuse_b3000"), card("reuse_b70")
    net = WCRBFNet.from_config(big.cfg)
    first = check_vjp(torch, big, net)
    second = check_vjp(torch, small, net)
    third, _ = vjp(torch, net, big, _lib.VJP_K2R)
    assert same_bits(first, third)
    fresh, _ = vjp(torch, WCRBFNet.from_config(small.cfg), small, _lib.VJP_K2R)
    assert same_bits(second, fresh)


def test_forward_is_independent_of_the_batch_on_an_overlapping_card(gpu):
    c = card("perm")
    net = WCRBFNet.from_config(c.cfg)
    sp, dn = forward_both(c, net)
    check_forward(c, sp, dn)
    perm = np.random.default_rng(1).permutation(c.B)
    a, _ = forward_guarded(net, c.params, np.ascontiguousarray(c.x[perm]), _lib.FWD_K1R)
    assert np.array_equal(sp[perm].view(np.uint32), a.view(np.uint32))
    b, _ = forward_guarded(net, c.params, np.ascontiguousarray(c.x[:257]), _lib.FWD_K1R)
    assert np.array_equal(sp[:257].view(np.uint32), b.view(np.uint32))
    check_vjp(gpu, c, net)


def test_non_finite_inputs(gpu):
    """A NaN in an ungated coordinate of query 23, +Inf in the cotangent of query 40."""
    torch = gpu
    c = card("nonfinite")
    qa, qb, ob = 23, 40, 2
    h = c.live()
    la, lb = h[qa], h[qb]
    rest = ~(la | lb)
    if not (la.any() and lb.any() and (lb & ~la).any() and rest.sum() >= 4):
        pytest.fail("test inputs, not the code under test: the two queries do not leave live regions of their own")
    x, g = c.x.copy(), c.g.copy()
    x[qa, 3] = np.nan
    g[qb, ob] = np.inf
    net = WCRBFNet.from_config(c.cfg)
    clean, _ = forward_both(c, net)
    sp, _ = forward_both(c, net, x)
    others = np.arange(c.B) != qa
    assert np.isnan(sp[qa]).all() and np.array_equal(sp[others].view(np.uint32), clean[others].view(np.uint32))
    got, _ = vjp(torch, net, c, _lib.VJP_K2R, x, g)
    assert np.isnan(got["kernel"]).all()                         # the NaN query's basis values reach every centre's row
    assert np.isnan(got["centers"][la]).all() and np.isnan(got["log_sigs"][la]).all()
    only_b = lb & ~la
    assert not np.isfinite(got["centers"][only_b]).any() and not np.isfinite(got["log_sigs"][only_b]).any()
    keep = np.ones(c.B, bool)
    keep[[qa, qb]] = False
    ref = k2.vjp_reference(c.basis, c.params, x[keep], g[keep], su.gamma(c.cfg, x[keep]))
    for leaf in ("centers", "log_sigs"):
        r, S = ref[leaf]
        es, em = su.ratios(got[leaf][rest], r[rest], S[rest])
        print(f"SPARSEPARITY {c.tag:22s} K2r {leaf:9s} |err|/S {es:.2e} on the regions of the finite queries")
        assert es <= su.C_S and em <= 1.0, (leaf, es, em)
    bias_ref = k2.vjp_reference(c.basis, c.params, c.x, g, c.gamma())["bias"]
    fin = np.arange(c.O) != ob
    assert got["bias"][ob] == np.inf and su.ratios(got["bias"][fin], bias_ref[0][fin], bias_ref[1][fin])[0] <= su.C_S


# ------------------------------------------------------------------------------------------------ the tick
TICKS = [  # tag, D, O, mode
    ("tick_d8_o2_frenet", 8, 2, _lib.ROLLOUT_FRENET_LS),
    ("tick_d7_o16_ks", 7, 16, _lib.ROLLOUT_ST_KS),
    ("tick_d8_o16_frenet", 8, 16, _lib.ROLLOUT_FRENET_LS),      # T S = 64: the whole staging row
    ("tick_d7_o12_select", 7, 12, _lib.ROLLOUT_ST_SELECT),      # O < OPS = 16
    ("tick_d7_o6_fullint", 7, 6, _lib.ROLLOUT_FULLINT),         # O < OPS = 10
]


def tick_card(tag, D, O, basis="inverse_quadratic", B=300):
    spec = su._grid(tag, (3, 3), D, O, 3, basis, B)
    c = su.Card(spec)
    # controls of a size the vehicle models integrate without leaving their range
    c.params["params"]["linear"]["kernel"] *= np.float32(0.2)
    c.params["params"]["linear"]["bias"] *= np.float32(0.2)
    return c


def state0(c, mode, B):
    rng = np.random.default_rng(B)
    if mode == _lib.ROLLOUT_FULLINT:
        return rng.uniform(0, 7, size=(B, 1)).astype(np.float32)
    if mode == _lib.ROLLOUT_FRENET_LS:
        return (rng.normal(size=(B, 8)) * [1, .2, .2, 1, .1, .1, .15, .08] + [0, 0, 0, 4, 0, 0, 0, 0]).astype(np.float32)
    st = rng.normal(size=(B, 7)) * [2, 2, .3, 1, 1, .4, .1]
    st[:, 3] = rng.uniform(0.2, 7.5, B)
    return st.astype(np.float32)


@pytest.mark.parametrize("tag,D,O,mode", TICKS, ids=[t[0] for t in TICKS])
def test_tick_equals_forward_then_rollout(gpu, tag, D, O, mode):
    """plan_tick under the forced K1r == K1r forward -> flip of the mirrored rows -> the stand-alone roll-out, bit for bit
    (tests/test_gpu_sparse.py::test_sparse_tick_equals_forward_then_rollout), B = 300 and 257, with and without mirror flags."""
    torch = gpu
    c = tick_card(tag, D, O)
    T = O // 2
    net = WCRBFNet.from_config(c.cfg)
    net.set_options(fwd_kernel=_lib.FWD_K1R)
    for B in (300, 257):
        x = torch.from_numpy(c.x[:B]).cuda()
        s0 = torch.from_numpy(state0(c, mode, B)).cuda()
        mirror = torch.from_numpy((np.random.default_rng(4).random(B) < 0.4).astype(np.int32)).cuda()
        for m in (None, mirror):
            ctrl, states = planner.plan_tick(net, c.params, x, m, s0, configs.DYN_PARAMS, mode=mode)
            assert net.last_launch() == su.k1r_launch(c.cfg, B, roll=True), net.last_launch()
            u = net.apply(c.params, x).clone()
            assert net.last_launch() == su.k1r_launch(c.cfg, B), net.last_launch()
            if m is not None:
                u[m.bool(), T:] *= -1.0
            assert torch.equal(ctrl, u), tag
            if mode == _lib.ROLLOUT_FULLINT:
                ref = dynamics.rollout_fullint(s0.reshape(-1), u)
            elif mode == _lib.ROLLOUT_ST_KS:
                ref = dynamics.integrate_st_ks_mult(torch.cat([s0, u], dim=1), configs.DYN_PARAMS)
            elif mode == _lib.ROLLOUT_FRENET_LS:
                ref = dynamics.integrate_frenet_mult(torch.cat([s0, u], dim=1), configs.DYN_PARAMS)
            else:
                ref = dynamics.integrate_st_mult(torch.cat([s0, u], dim=1), configs.DYN_PARAMS)
            assert torch.isfinite(states).all() and torch.equal(states, ref.reshape(states.shape)), tag
    got = ctrl.cpu().numpy()
    refc, scale = su.forward_reference(c.cfg, c.params, c.x[:257])
    refc[mirror.cpu().numpy() != 0, T:] *= -1.0
    assert (np.abs(got - refc) <= 1e-5 * np.abs(refc) + 3e-6 * scale).all(), tag


def test_ticks_without_a_k1r_instance(gpu):
    """OPS = 5 and the generic basis have no tick instance of K1r (sparse_geometry).  The forward's option is not the tick's: with
    K1r forced, the fast basis runs the dense K1 with the roll-out in its epilogue, the generic basis has no one-launch tick at
    all and the call raises UNSUPPORTED."""
    torch = gpu
    mode = _lib.ROLLOUT_ST_KS
    c = tick_card("tick_o4", 7, 4, "gaussian")
    net = WCRBFNet.from_config(c.cfg)
    net.set_options(fwd_kernel=_lib.FWD_K1R)
    x, s0 = torch.from_numpy(c.x).cuda(), torch.from_numpy(state0(c, mode, c.B)).cuda()
    ctrl, states = planner.plan_tick(net, c.params, x, None, s0, configs.DYN_PARAMS, mode=mode)
    name = net.last_launch()["kernel"]
    assert name.startswith("rbf_fwd_qlane<") and "ROLL=1" in name, name
    ref, scale = c.forward_reference()
    assert (np.abs(ctrl.cpu().numpy() - ref) <= 1e-5 * np.abs(ref) + 3e-6 * scale).all() and torch.isfinite(states).all()
    c = tick_card("tick_generic", 7, 10, "multiquadric")
    net = WCRBFNet.from_config(c.cfg)
    net.set_options(fwd_kernel=_lib.FWD_K1R)
    x, s0 = torch.from_numpy(c.x).cuda(), torch.from_numpy(state0(c, mode, c.B)).cuda()
    with pytest.raises(ValueError, match="UNSUPPORTED"):
        planner.plan_tick(net, c.params, x, None, s0, configs.DYN_PARAMS, mode=mode)


# ------------------------------------------------------------------------------------------------ refusals and AUTO
def limit_pairs():
    (f150, o150), (f60, o60) = su.lds_limit_specs()
    pairs = [(su.LIMIT_BY_TAG[a], su.LIMIT_BY_TAG[b], True) for a, b in su.LIMIT_PAIRS]
    return pairs + [(f150, o150, True), (f60, o60, False)]


@pytest.mark.parametrize("i", range(6), ids=["E32_33", "cap96_100", "nr1024_1025", "O16_17", "lds150", "lds60"])
def test_limits_run_on_one_side_and_refuse_on_the_other(gpu, i):
    """Under the forced K1r and K2r the card inside the limit runs (within the bounds) and the one outside raises UNSUPPORTED;
    AUTO on the latter gives the dense kernels' bits.  lds60 is K2r's limit alone: the forward runs on both sides."""
    torch = gpu
    fits, over, forward_refuses = limit_pairs()[i]
    c = su.Card(fits)
    assert su.setup(c.cfg)["ok"] and su.vjp_eligible(c.cfg)
    net = WCRBFNet.from_config(c.cfg)
    check_forward(c, *forward_both(c, net))
    check_vjp(torch, c, net)
    c = su.Card(over)
    assert not su.vjp_eligible(c.cfg) and su.setup(c.cfg)["ok"] == (not forward_refuses)
    net = WCRBFNet.from_config(c.cfg)
    dn, launch = forward_guarded(net, c.params, c.x, _lib.FWD_K1)
    assert launch["kernel"].startswith("rbf_fwd_qlane<")
    if forward_refuses:
        with pytest.raises(ValueError, match="UNSUPPORTED"):
            forward_guarded(net, c.params, c.x, _lib.FWD_K1R)
        au, launch = forward_guarded(net, c.params, c.x, _lib.FWD_AUTO)
        assert not launch["kernel"].startswith("rbf_fwd_sparse<")
        if launch["kernel"].startswith("rbf_fwd_qlane<"):
            assert np.array_equal(au.view(np.uint32), dn.view(np.uint32))
        ref, scale = c.forward_reference()
        assert (np.abs(dn - ref) <= 1e-5 * np.abs(ref) + 3e-6 * scale).all()
        assert np.abs(au - ref).max() <= 1e-4 * np.abs(ref).max()     # whichever dense kernel AUTO took: its own tests bound it
    else:
        check_forward(c, *forward_both(c, net))
    net.bind(c.params)
    assert supported(torch, net, _lib.VJP_K2R, c.B) == 0
    with pytest.raises(ValueError, match="UNSUPPORTED"):
        vjp(torch, net, c, _lib.VJP_K2R)
    auto, name = vjp(torch, net, c, _lib.VJP_AUTO)
    dense, name2 = vjp(torch, net, c, _lib.VJP_K2)
    assert name == name2 and name.startswith("rbf_vjp_kernel<") and same_bits(auto, dense), (name, name2)


@pytest.mark.parametrize("tag", ["nr64", "nr12_of_16", "i_d5_o5_k5", "cap96", "repeated_rows", "i_d3_o16_k9"])
def test_auto_takes_the_restated_preference(gpu, tag):
    """AUTO == sparse_preferred restated, at B = 64 and 65 and at the case's batch: the forward by name (K1s up to 64 queries), the
    VJP by bits, K2r's and K2's differing at that batch."""
    torch = gpu
    c = card(tag)
    net = WCRBFNet.from_config(c.cfg)
    for B in (64, 65, c.B):
        want = su.sparse_preferred(c.cfg, B)
        assert want == (B > 64 and su.setup(c.cfg)["mean"] <= 0.25 * su.setup(c.cfg)["nr"])
        x, g = np.ascontiguousarray(c.x[:B]), np.ascontiguousarray(c.g[:B])
        out, launch = forward_guarded(net, c.params, x, _lib.FWD_AUTO)
        if B <= 64:
            assert launch["kernel"].startswith("rbf_fwd_clane<"), launch
        else:
            assert launch["kernel"].startswith("rbf_fwd_sparse<") == want, (tag, B, launch, want)
        sparse, _ = vjp(torch, net, c, _lib.VJP_K2R, x, g)
        dense, _ = vjp(torch, net, c, _lib.VJP_K2, x, g)
        if same_bits(sparse, dense):
            pytest.fail(f"test inputs, not the code under test: K2r and K2 give identical bits at B = {B}")
        auto, _ = vjp(torch, net, c, _lib.VJP_AUTO, x, g)
        assert same_bits(auto, sparse if want else dense), (tag, B, want)
