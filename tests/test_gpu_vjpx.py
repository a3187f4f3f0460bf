"""The query VJP on the GPU: K5 (rbf_vjpx_qlane), K5m (rbf_vjpx_mfma), the float64 kernel and every Python surface on top.

Reference: torch.autograd of the float64 restatement (tests/_vjpx_util.py::ref_gx), never another kernel of this library.
float32 bound per entry: |gx - ref| <= 1e-5 |ref| + C_S S, S the sum of the absolute terms of the gradient and C_S = 4 x the
error of the same formula in NumPy float32 (tests/_vjpx_util.py, profiles/vjp_x_parity.txt).  Every test asserts the kernel
name from last_launch(), so a silent fall-back cannot pass.  Each float32 case prints its own max |gx - ref| / S.

Row independence: K5 and K5m give one lane one query, so a row never sees another row's data; the waves of a workgroup split the
centres and their number depends on the batch size, so row i of a large batch equals the B = 1 call on that row to the bound
above, not bitwise (bitwise holds between calls of one batch size, and is asserted there).
"""
import numpy as np
import pytest
import torch

import _vjpx_util as vx
from _cluster_util import cluster_case, row_chunk
from conftest import load_ckpt_fixture, load_deeper_fixture
from irbfn_amd import _lib, autograd, configs
from irbfn_amd.model import ClusterWCRBFNet, DeeperWCRBFNet, WCRBFNet
from oracle import irbfn_oracle as orc

pytestmark = pytest.mark.gpu
K5_CASES, K5M_CASES = vx.k5_cases(), vx.k5m_cases()
HIGHK = "dnmpc_1regions_newdata_oldintloss_nomirror_highk"


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(net, params, x, g, kernel, prefix):
    net.set_options(vjpx_kernel=kernel)
    gx = net.vjp_x(params, _cuda(x), _cuda(g))
    name = net.last_launch()["kernel"]
    assert name.startswith(prefix), name
    return gx


def _check(what, gx, cfg, params, x, g, ref=None):
    ref = vx.ref_gx(cfg, params, x, g) if ref is None else ref
    _, S = vx.hand_gx(cfg, params, x, g, np.float64)
    got = gx.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), what
    ok, worst = vx.within(got, ref, S)
    print(f"[vjpx] {what}: max |gx - ref| / S = {worst:.2e} (C_S = {vx.C_S:.2e}), max |ref| = {np.abs(ref).max():.3e}")
    assert ok, (what, worst, vx.C_S)
    return ref


# ---- 1. K5 against the float64 reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(K5_CASES))
def test_k5_matches_reference(gpu, name):
    cfg, params, x, g = K5_CASES[name]()
    net = WCRBFNet.from_config(cfg)
    gx = _run(net, params, x, g, _lib.VJPX_K5, "rbf_vjpx_qlane<")
    ref = _check(f"K5 {name}", gx, cfg, params, x, g)
    if name == "B4097":                          # the batches around one 64-row tile are its prefixes
        for B in (1, 63, 64, 65):
            _check(f"K5 {name}[:{B}]", _run(net, params, x[:B], g[:B], _lib.VJPX_K5, "rbf_vjpx_qlane<"), cfg, params, x[:B], g[:B],
                   ref=ref[:B])
    if name == "one_region_far_inside":          # the gate term is ~0 there; AUTO stays on K5 for O = 10
        assert torch.equal(gx, _run(net, params, x, g, _lib.VJPX_AUTO, "rbf_vjpx_"))


# ---- 2. K5m, forced ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(K5M_CASES))
def test_k5m_matches_reference(gpu, name):
    cfg, params, x, g = K5M_CASES[name]()
    net = WCRBFNet.from_config(cfg)
    gx = _run(net, params, x, g, _lib.VJPX_K5M, "rbf_vjpx_mfma<")
    ref = _check(f"K5m {name}", gx, cfg, params, x, g)
    _check(f"K5 {name}", _run(net, params, x, g, _lib.VJPX_K5, "rbf_vjpx_qlane<"), cfg, params, x, g, ref=ref)
    # automatic selection: K5m for O > 16 (profiles/vjp_x.txt), the forced kernel's result bit for bit
    auto = _run(net, params, x, g, _lib.VJPX_AUTO, "rbf_vjpx_mfma<" if cfg["out_features"] > 16 else "rbf_vjpx_qlane<")
    if cfg["out_features"] > 16:
        assert torch.equal(auto, gx)


@pytest.mark.parametrize("name", ["basis_matern32", "grid_300_regions"])
def test_k5m_forced_on_a_net_it_does_not_take(gpu, name):
    """Generic basis / several regions: IRBFN_ERR_UNSUPPORTED -> ValueError, nothing is launched in its place."""
    cfg, params, x, g = K5_CASES[name]()
    net = WCRBFNet.from_config(cfg)
    net.set_options(vjpx_kernel=_lib.VJPX_K5M)
    with pytest.raises(ValueError, match="IRBFN_ERR_UNSUPPORTED"):
        net.vjp_x(params, _cuda(x), _cuda(g))
    net.set_options(vjpx_kernel=_lib.VJPX_AUTO)
    assert net.vjp_x(params, _cuda(x), _cuda(g)).shape == x.shape
    assert net.last_launch()["kernel"].startswith("rbf_vjpx_qlane<")


# ---- 3. float64 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", ["dnmpc_1regions_newdata_oldintloss_nomirror_highk", "dnmpc_128regions",
                                 "dnmpc_1regions_newnewdata_1stepst_l1_newarch_ksint_iq", "dnmpc_12regions_frenet_l1_bigdata"])
def test_float64_fixtures(gpu, run):
    cfg, params, x, *_ = load_ckpt_fixture(run)
    g = vx.cotangent(3, x.shape[0], cfg["out_features"]).astype(np.float64)
    ref = vx.ref_gx(cfg, params, x, g)
    net = WCRBFNet.from_config(cfg, use_float64=True)
    gx = net.vjp_x(params, x, g)                 # use_float64 nets route vjp_x to vjp_x64
    assert gx.dtype == np.float64 and np.array_equal(gx, net.vjp_x64(params, x, g))
    assert np.abs(gx - ref).max() <= 1e-12 * np.abs(ref).max(), np.abs(gx - ref).max() / np.abs(ref).max()


@pytest.mark.parametrize("basis", vx.BASES)
def test_float64_all_bases(gpu, basis):
    cfg, params, x, g = K5_CASES[f"basis_{basis}"]()
    ref = vx.ref_gx(cfg, params, x, g)
    gx = WCRBFNet.from_config(cfg, use_float64=True).vjp_x(params, x.astype(np.float64), g.astype(np.float64))
    assert np.abs(gx - ref).max() <= 1e-12 * np.abs(ref).max(), np.abs(gx - ref).max() / np.abs(ref).max()


def test_float64_wide_output_and_central_difference(gpu):
    """vjp_x64 against an on-device central difference of apply64 (step 1e-6 (hi - lo) per coordinate) on the 64 stored queries
    of the 1000-centre fixture; and the O > 16 path of the float64 kernel (cotangent rows read per centre)."""
    cfg, params, x, *_ = load_ckpt_fixture(HIGHK)
    net = WCRBFNet.from_config(cfg, use_float64=True)
    g = vx.cotangent(4, x.shape[0], cfg["out_features"]).astype(np.float64)
    gx = net.vjp_x64(params, x, g)
    ref = vx.ref_gx(cfg, params, x, g)
    fd = np.zeros_like(gx)
    for d in range(cfg["in_features"]):
        h = 1e-6 * (cfg["upper_bounds"][d][0] - cfg["lower_bounds"][d][0])
        e = np.zeros(cfg["in_features"])
        e[d] = h
        fd[:, d] = ((net.apply64(params, x + e) - net.apply64(params, x - e)) * g).sum(1) / (2 * h)
    assert np.abs(fd - gx).max() <= 1e-6 * np.abs(ref).max(), np.abs(fd - gx).max() / np.abs(ref).max()
    cfg, params, x, g = K5_CASES["O100_gaussian"]()
    gx = WCRBFNet.from_config(cfg, use_float64=True).vjp_x(params, x.astype(np.float64), g.astype(np.float64))
    ref = vx.ref_gx(cfg, params, x, g)
    assert np.abs(gx - ref).max() <= 1e-12 * np.abs(ref).max()


# ---- 4. properties of the float32 kernels --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,prefix,name", [(_lib.VJPX_K5, "rbf_vjpx_qlane<", "B4097"), (_lib.VJPX_K5, "rbf_vjpx_qlane<", "grid_300_regions"),
                                                (_lib.VJPX_K5, "rbf_vjpx_qlane<", "basis_spline"), (_lib.VJPX_K5M, "rbf_vjpx_mfma<", "cfg2"),
                                                (_lib.VJPX_K5M, "rbf_vjpx_mfma<", "cfg4_O100")])
def test_float32_properties(gpu, kernel, prefix, name):
    cases = K5M_CASES if kernel == _lib.VJPX_K5M else K5_CASES
    cfg, params, x, g = cases[name]()
    net = WCRBFNet.from_config(cfg)
    run = lambda xx, gg: _run(net, params, xx, gg, kernel, prefix)
    gx = run(x, g)
    assert torch.equal(gx, run(x, g)), "not bitwise repeatable"
    assert torch.equal(run(x, 2.0 * g), 2.0 * gx), "vjp_x(2 g) != 2 vjp_x(g) bitwise"
    z = run(x, np.zeros_like(g))
    assert not z.any(), "zero cotangent"
    # rows are independent: row i alone (another number of waves per workgroup: to the bound, not bitwise)
    ref = vx.ref_gx(cfg, params, x, g)
    for i in (0, x.shape[0] // 2, x.shape[0] - 1):
        _check(f"{name} row {i} alone", run(x[i:i + 1], g[i:i + 1]), cfg, params, x[i:i + 1], g[i:i + 1], ref=ref[i:i + 1])
    # NaN in one query reaches that row only; the others do not change by a bit
    xn = x.copy()
    xn[3, cfg["in_features"] - 1] = np.nan
    gn = net.vjp_x(params, _cuda(xn), _cuda(g))
    assert torch.isnan(gn[3]).any()
    keep = torch.ones(x.shape[0], dtype=torch.bool, device="cuda")
    keep[3] = False
    assert torch.equal(gn[keep], gx[keep])


@pytest.mark.parametrize("basis", vx.BASES)
def test_query_on_a_centre(gpu, basis):
    """Queries placed exactly on centres (float32 values of the bound parameters): finite rows equal to the float64 formula;
    linear / poisson_one / poisson_two return the convention (that pair contributes 0), where autograd of the restatement is NaN."""
    cfg, params, x, g = K5_CASES[f"basis_{basis}"]()
    c = vx.inner(params)["rbf_list"]["centers"]
    x = x[:64].copy()
    g = g[:64]
    x[:40] = c.reshape(-1, cfg["in_features"])[:40]
    hand, S = vx.hand_gx(cfg, params, x, g, np.float64)
    assert np.isfinite(hand).all()
    assert np.isnan(vx.ref_gx(cfg, params, x, g)[:40]).any()
    net = WCRBFNet.from_config(cfg)
    kernels = [(_lib.VJPX_K5, "rbf_vjpx_qlane<")]
    for kernel, prefix in kernels:
        got = _run(net, params, x, g, kernel, prefix).cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all()
        ok, worst = vx.within(got, hand, S)
        print(f"[vjpx] on a centre {basis}: max |gx - hand64| / S = {worst:.2e}")
        assert ok, (basis, worst)
    g64 = WCRBFNet.from_config(cfg, use_float64=True).vjp_x(params, x.astype(np.float64), g.astype(np.float64))
    assert np.abs(g64 - hand).max() <= 1e-12 * np.abs(hand).max()


def test_query_on_a_centre_k5m(gpu):
    cfg, params, x, g = K5M_CASES["d8_O16"]()
    x = x.copy()
    x[:40] = vx.inner(params)["rbf_list"]["centers"].reshape(-1, 8)[:40]
    hand, S = vx.hand_gx(cfg, params, x, g, np.float64)
    got = _run(WCRBFNet.from_config(cfg), params, x, g, _lib.VJPX_K5M, "rbf_vjpx_mfma<").cpu().numpy().astype(np.float64)
    ok, worst = vx.within(got, hand, S)
    assert np.isfinite(got).all() and ok, worst


# ---- 5. input_jacobian ---------------------------------------------------------------------------------------------------------
def test_input_jacobian(gpu):
    cfg, params, x, _ = K5_CASES[f"ckpt_{HIGHK}"]()
    net = WCRBFNet.from_config(cfg)
    jac = net.input_jacobian(params, x)
    assert isinstance(jac, np.ndarray) and jac.shape == (64, 10, 7)
    assert net.last_launch()["kernel"].startswith("rbf_vjpx_")
    for o in range(10):
        g = np.zeros((64, 10), np.float32)
        g[:, o] = 1.0
        _, S = vx.hand_gx(cfg, params, x, g, np.float64)
        ok, worst = vx.within(jac[:, o, :], vx.ref_gx(cfg, params, x, g), S)
        assert ok, (o, worst)


# ---- 6. one batch past 2^21 rows -----------------------------------------------------------------------------------------------
def test_past_2p21_rows(gpu):
    B = (1 << 21) + 5
    cfg, params = vx.synth_net(601, D=8, O=10, K=64, grid=(2, 2))
    rng = np.random.default_rng(602)             # not the net's seed: its first draw would put row 0 on a centre
    x = rng.uniform(-2, 2, size=(B, 8)).astype(np.float32)
    g = rng.normal(size=(B, 10)).astype(np.float32)
    net = WCRBFNet.from_config(cfg)
    gx = _run(net, params, x, g, _lib.VJPX_K5, "rbf_vjpx_qlane<")
    assert net.last_launch()["grid"] == (B + 63) // 64
    rows = np.unique(np.concatenate([[0, B - 1], rng.integers(0, B, size=64)]))
    _check("K5 past 2^21 rows", gx[torch.from_numpy(rows).cuda()], cfg, params, x[rows], g[rows])
    assert torch.isfinite(gx).all()


# ---- 7. variants ---------------------------------------------------------------------------------------------------------------
def test_deeper_vjp_x(gpu):
    cfg, params, x, _ = load_deeper_fixture()
    params = {"params": {k: {n: np.asarray(v, np.float32) for n, v in d.items()} for k, d in params["params"].items()}}
    x = np.asarray(x, np.float32)
    g = vx.cotangent(7, x.shape[0], cfg["out_features"])
    ref = vx.ref_gx(cfg, params, x, g, apply=orc.deeper_wcrbfnet_apply)
    net = DeeperWCRBFNet.from_config(cfg)
    gx = net.vjp_x(params, x, g)
    assert net.stage.last_launch()["kernel"].startswith("rbf_vjpx_")
    # the bound of the stage, with the head's cotangent of the stage output as the stage's cotangent (float64, from the reference)
    p = vx.inner(params)
    tp = {k: {n: torch.tensor(np.asarray(v, np.float64)) for n, v in d.items()} for k, d in p.items()}
    stage_cfg = dict(cfg, out_features=DeeperWCRBFNet.HIDDEN)
    stage = {"params": {"rbf_list": p["rbf_list"], "linear": p["linear_pre1"]}}
    h1 = torch.tensor(orc.wcrbfnet_apply(stage_cfg, {"params": {"rbf_list": tp["rbf_list"], "linear": tp["linear_pre1"]}},
                                         torch.tensor(np.asarray(x, np.float64))).numpy(), requires_grad=True)
    out = torch.relu(torch.relu(h1) @ tp["linear_pre2"]["kernel"] + tp["linear_pre2"]["bias"]) @ tp["linear"]["kernel"]
    (gh1,) = torch.autograd.grad((out * torch.tensor(np.asarray(g, np.float64))).sum(), h1)
    _, S = vx.hand_gx(stage_cfg, stage, x, gh1.numpy(), np.float64)
    ok, worst = vx.within(gx, ref, S)
    print(f"[vjpx] deeper: max |gx - ref| / S = {worst:.2e}")
    assert ok, worst


def _cluster_ref(cfg, params, x, g, gl):
    """autograd of the float64 restatement of ClusterWCRBFNet w.r.t. x, both cotangents, in row chunks."""
    tp = {"params": {k: {n: torch.tensor(np.asarray(v, np.float64)) for n, v in d.items()} for k, d in params["params"].items()}}
    out = np.empty(x.shape, np.float64)
    c = row_chunk(cfg)
    for i in range(0, x.shape[0], c):
        xt = torch.tensor(np.asarray(x[i:i + c], np.float64), requires_grad=True)
        o, lg = orc.cluster_wcrbfnet_apply(cfg, tp, xt)
        loss = (o * torch.tensor(np.asarray(g[i:i + c], np.float64))).sum()
        if gl is not None:
            loss = loss + (lg * torch.tensor(np.asarray(gl[i:i + c], np.float64))).sum()
        (gx,) = torch.autograd.grad(loss, xt)
        out[i:i + c] = gx.numpy()
    return out


def _cluster_scale(cfg, params, x, g, gl):
    """S of the cluster net: the RBF term's S at the softmax weights, plus the absolute terms of the gate chain
    |dlogits| |Wc|^T with dlogits = gamma (dgamma - <gamma, dgamma>) (+ glogits), every product taken in absolute value."""
    p = {k: {n: np.asarray(v, np.float64) for n, v in d.items()} for k, d in params["params"].items()}
    lg = x.astype(np.float64) @ p["cluster"]["kernel"] + p["cluster"]["bias"]
    e = np.exp(lg - lg.max(1, keepdims=True))
    gam = e / e.sum(1, keepdims=True)
    S = np.zeros(x.shape)
    c = row_chunk(cfg)
    for i in range(0, x.shape[0], c):
        sl = slice(i, i + c)
        _, Sr, q = vx.hand_gx(cfg, {"params": {"rbf_list": p["rbf_list"], "linear": p["linear"]}}, x[sl], g[sl], np.float64, gamma=gam[sl])
        dl = gam[sl] * (np.abs(q) + (gam[sl] * np.abs(q)).sum(1, keepdims=True))
        if gl is not None:
            dl = dl + np.abs(gl[sl])
        S[sl] = Sr + dl @ np.abs(p["cluster"]["kernel"]).T
    return S


@pytest.mark.parametrize("R,K,B,basis", [(11, 20, 400, "gaussian"), (64, 16, 257, "inverse_quadratic"), (16, 20, 130, "matern52"),
                                         (500, 10, 256, "gaussian")])
def test_cluster_vjp_x(gpu, R, K, B, basis):
    rng, cfg, params, x = cluster_case(R + K, R=R, K=K, O=10, B=B, D=8, basis=basis)
    g = rng.normal(size=(B, 10)).astype(np.float32)
    gl = rng.normal(size=(B, R)).astype(np.float32)
    net = ClusterWCRBFNet(**cfg)
    for gl_in in (None, gl):
        gx = net.vjp_x(params, _cuda(x), _cuda(g), glogits=None if gl_in is None else _cuda(gl_in))
        name = net.stage.last_launch()["kernel"]
        assert name.startswith("rbf_vjpx_qlane<") and "EXT=1" in name, name
        ref = _cluster_ref(cfg, params, x, g, gl_in)
        ok, worst = vx.within(gx.cpu().numpy(), ref, _cluster_scale(cfg, params, x, g, gl_in))
        print(f"[vjpx] cluster R={R} K={K} {basis} glogits={gl_in is not None}: max |gx - ref| / S = {worst:.2e}")
        assert ok, (R, K, basis, worst)
    assert torch.equal(gx, net.vjp_x(params, _cuda(x), _cuda(g), glogits=_cuda(gl)))


# ---- 8. / 9. through torch.autograd --------------------------------------------------------------------------------------------
def _tick_net(seed=8):
    """64 gaussian centres in the config-2 box, O = 10 (T = 5), W ~ N(0, 0.3); queries from the central 40 % of the box."""
    card = dict(configs.model_card(2), num_kernels=64)
    rng = np.random.default_rng(seed)
    lo, hi = np.array([b[0] for b in card["lower_bounds"]]), np.array([b[0] for b in card["upper_bounds"]])
    params = {"params": {"rbf_list": {"centers": rng.uniform(lo, hi, size=(1, 64, 7)).astype(np.float32),
                                      "log_sigs": rng.uniform(0.0, 1.0, size=(1, 64)).astype(np.float32)},
                         "linear": {"kernel": (rng.normal(size=(64, 10)) * 0.3).astype(np.float32),
                                    "bias": np.zeros(10, np.float32)}}}
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    x = rng.uniform(mid - 0.4 * half, mid + 0.4 * half, size=(96, 7)).astype(np.float32)
    return card, params, x


def _state0(x):
    z = torch.zeros_like(x[:, 0])
    return torch.stack([z, z, z, x[:, 0], z, x[:, 6], x[:, 5]], 1)     # scripts/train_nmpc.py:260-266


def _leaves_cuda(params, requires_grad):
    return {"params": {k: {n: torch.tensor(v, device="cuda", requires_grad=requires_grad) for n, v in d.items()}
                       for k, d in params["params"].items()}}


def test_planning_tick_is_differentiable_end_to_end(gpu):
    """query -> net -> ST_KS roll-out -> loss on the last position, d loss / d x against the same composition of the float64
    restatements.  No clip of the roll-out sits on a bound (asserted on the reference's own values), so the tie rule cannot
    decide the comparison.  Bound: 2e-4 of max |ref|, the bound tests/test_gpu_parity.py::
    test_autograd_train_step_matches_oracle_grad uses for gradients through the same float32 chain."""
    card, params, x = _tick_net()
    DP = configs.DYN_PARAMS
    tp = orc.torch_params(params, torch.float64)
    xr = torch.tensor(np.asarray(x, np.float64), requires_grad=True)
    u = orc.wcrbfnet_apply(card, tp, xr)
    states = orc.integrate_st_ks_mult(torch.hstack((_state0(xr), u)), DP)
    (states[:, -1, :2] ** 2).sum().backward()
    ref = xr.grad.numpy()
    assert np.isfinite(ref).all() and (np.abs(ref).max(0) > 0).all()
    with torch.no_grad():                        # every clipped quantity strictly inside its bounds
        sv_max, a_max, s_max, v_max = DP[9], DP[10], DP[11], DP[12]
        st, ud = torch.cat([_state0(xr)[:, None, :], states], 1).detach(), u.detach()
        assert float(st[:, :, 2].abs().max()) < s_max - 1e-3 and float(st[:, :, 3].abs().max()) < v_max - 1e-3
        assert float(ud[:, :5].abs().max()) < a_max - 1e-3 and float(ud[:, 5:].abs().max()) < sv_max - 1e-3

    net = WCRBFNet.from_config(card)
    grads = []
    for need_x in (True, False):
        P = _leaves_cuda(params, True)
        xt = torch.tensor(x, device="cuda", requires_grad=need_x)
        y = autograd.wcrbf_apply(net, P, xt)
        s = autograd.integrate_st_ks_mult(torch.hstack((_state0(xt), y)), DP)
        s[:, -1, :2].square().sum().backward()
        last = net.last_launch()["kernel"]
        if need_x:
            assert last.startswith("rbf_vjpx_"), last
            got = xt.grad.cpu().numpy().astype(np.float64)
            err = np.abs(got - ref).max() / np.abs(ref).max()
            print(f"[vjpx] end to end: max |x.grad - ref| / max |ref| = {err:.2e}")
            assert err <= 2e-4, err
        else:
            assert xt.grad is None and last.startswith("rbf_vjp_"), last     # 9: the parameter VJP is the last launch, as before
        grads.append([P["params"][g_][n_].grad.clone() for g_, n_ in (("rbf_list", "centers"), ("rbf_list", "log_sigs"),
                                                                        ("linear", "kernel"), ("linear", "bias"))])
    for a, b in zip(*grads):                     # the parameter gradients of the same backward are unchanged, bit for bit
        assert torch.equal(a, b)


def test_backward_without_query_gradient_launches_what_it_launched(gpu):
    """x.requires_grad == False: the backward's last launch is the net's parameter-VJP kernel, the one net.vjp runs."""
    cfg, params, x, g = K5_CASES[f"ckpt_{HIGHK}"]()
    net = WCRBFNet.from_config(cfg)
    P = _leaves_cuda(params, True)
    net.vjp(P, _cuda(x), _cuda(g))
    want = net.last_launch()["kernel"]
    assert want.startswith("rbf_vjp_") and not want.startswith("rbf_vjpx_"), want
    out = autograd.wcrbf_apply(net, P, _cuda(x))
    assert net.last_launch()["kernel"].startswith("rbf_fwd_")
    (out * _cuda(g)).sum().backward()
    assert net.last_launch()["kernel"] == want
    xt = _cuda(x).requires_grad_()
    (autograd.wcrbf_apply(net, P, xt) * _cuda(g)).sum().backward()
    assert net.last_launch()["kernel"].startswith("rbf_vjpx_")
    ok, worst = vx.within(xt.grad.cpu().numpy(), vx.ref_gx(cfg, params, x, g), vx.hand_gx(cfg, params, x, g, np.float64)[1])
    assert ok, worst
