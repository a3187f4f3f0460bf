"""The region-weighted forward on the matrix cores: ``rbf_fwd_f16gram_gamma`` / ``rbf_tick_f16gram_gamma``, selected by
``fwd_gamma_kernel = FWDG_K1G`` for ``irbfn_net_forward_gamma`` / ``irbfn_plan_tick_gamma``.

Every case runs against the float64 statement of tests/_cluster_gram_util.py (sum_r gamma_br sum_k phi_brk W_ko + bias for
arbitrary gamma) with two bounds of the project: per element 1e-5 |ref| + 3e-6 sum |gamma phi W| (tests/test_gpu_fullsize.py) and
``_assert_forward`` of tests/test_gpu_cluster_scale.py.  The parity cases carry a kernel axis {FWDG_K1, FWDG_K1G}: the K1 leg
shows that today's kernel meets the same bound on the same inputs.  Inputs follow ``cluster_case`` / ``_forward_case``: centres
and queries in [-2, 2]^d, log sigma in [0, 1] -- by the formulas of gram_header (pack_all.hip) ex = 2, ec = 3, so the pack's
verdict is "ok" and every query is inside the expansion's box.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from _cluster_gram_util import assert_elementwise, gamma_forward64, softmax_gamma
from _cluster_util import cluster_case
from _rollout_util import RTOL, assert_states_close
from conftest import load_ckpt_fixture
from irbfn_amd import _lib, configs, planner
from irbfn_amd import dynamics as dyn
from irbfn_amd.model import ClusterWCRBFNet, WCRBFNet, _ptr, _stream_ptr
from oracle import irbfn_oracle as orc

pytestmark = pytest.mark.gpu
FAST = ("gaussian", "inverse_quadratic", "inverse_multiquadric")
KERNELS = {"k1": _lib.FWDG_K1, "k1g": _lib.FWDG_K1G}
NAME = {"k1": "rbf_fwd_qlane<", "k1g": "rbf_fwd_f16gram_gamma<"}
OK, UNSUPPORTED, NO_PARAMS = 0, -2, -4
DP = np.array(configs.DYN_PARAMS)


def test_status_numbers():
    lib = _lib.load()
    assert b"outside the compiled" in lib.irbfn_strerror(UNSUPPORTED) and b"set_params" in lib.irbfn_strerror(NO_PARAMS)


def _case(seed, R, K, basis, B, D=8, O=10, wide_w=False):
    """``_forward_case`` of test_gpu_cluster_scale.py for any d and O; wide_w: Dense weights of 1e4 next to 1e-2."""
    rng, cfg, params, x = cluster_case(seed, R=R, K=K, O=O, B=B, D=D, basis=basis)
    p = params["params"]
    p["rbf_list"]["log_sigs"] = rng.uniform(0.0, 1.0, size=(R, K)).astype(np.float32)
    w = rng.normal(size=(K, O))
    if wide_w:
        w = w * np.where(rng.uniform(size=(K, O)) < 0.5, 1e4, 1e-2)
    p["linear"]["kernel"] = w.astype(np.float32)
    p["linear"]["bias"] = rng.normal(size=(O,)).astype(np.float32)
    p["cluster"]["kernel"] = rng.normal(size=(D, R)).astype(np.float32) * 2.0
    return rng, cfg, params, x


def _rbf(params):
    p = params["params"]
    return {"rbf_list": p["rbf_list"], "linear": p["linear"]}


def _fwd(stage, xt, gt, expect=OK):
    """irbfn_net_forward_gamma on device tensors -> out (or None where a status other than OK is expected)."""
    lib = _lib.load()
    out = torch.full((xt.shape[0], stage.out_features), 7.0, dtype=torch.float32, device=xt.device)
    st = lib.irbfn_net_forward_gamma(stage._handle(torch), _ptr(xt), _ptr(gt), _ptr(out), xt.shape[0], _stream_ptr(torch))
    assert st == expect, (st, expect)
    return out if st == OK else None


def _assert_forward_out(out, ref_out, what):
    """The output half of ``_assert_forward`` (tests/test_gpu_cluster_scale.py); the logits come from the gate kernel."""
    out = np.asarray(out, np.float64)
    assert np.isfinite(out).all(), what
    eo = np.abs(out - ref_out).max()
    assert eo <= 2e-5 * np.abs(ref_out).max() + 1e-5, (what, eo, np.abs(ref_out).max())


def _check(out, ref, scale, what):
    _assert_forward_out(out, ref, what)
    return assert_elementwise(out, ref, scale, what)


# ---- 1. chunk map and padding ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _padding_case(basis, D, K, R):
    """One set of inputs and one float64 reference per shape, shared by the two kernel legs."""
    _, cfg, params, x = _case(1000 * K + 10 * R + D, R, K, basis, 4097, D=D, wide_w=True)
    gamma = softmax_gamma(params, x).astype(np.float32)
    ref, scale = gamma_forward64(cfg, params, x, gamma)
    return cfg, params, x, gamma, ref, scale


@pytest.mark.parametrize("kern", list(KERNELS))
@pytest.mark.parametrize("D", [7, 8])
@pytest.mark.parametrize("basis", FAST)
def test_chunk_map_and_padding(gpu, basis, D, kern):
    """K in {10, 32, 33, 50} (a part chunk, a whole chunk, one centre into the second, two part-filled) x R in {1, 2, 3, 11}, batches
    around the 32-query wave tile; Dense weights of 1e4 next to 1e-2, so a padding row that picked up a neighbour's weights
    shows; with a zero Dense kernel the output is the bias exactly."""
    for K in (10, 32, 33, 50):
        for R in (1, 2, 3, 11):
            cfg, params, x, gamma, ref, scale = _padding_case(basis, D, K, R)
            stage = ClusterWCRBFNet(**cfg).stage.set_options(fwd_gamma_kernel=KERNELS[kern])
            stage.bind(_rbf(params))
            xt, gt = torch.from_numpy(x).cuda(), torch.from_numpy(gamma).cuda()
            for B in (1, 31, 32, 33, 65, 4097):
                out = _fwd(stage, xt[:B].contiguous(), gt[:B].contiguous())
                assert stage.last_launch()["kernel"].startswith(NAME[kern]), stage.last_launch()
                _check(out.cpu().numpy(), ref[:B], scale[:B], (basis, D, K, R, B, kern))
            zero = _rbf(params)
            zero["linear"] = {"kernel": np.zeros_like(zero["linear"]["kernel"]), "bias": zero["linear"]["bias"]}
            stage.bind(zero)
            out = _fwd(stage, xt[:65].contiguous(), gt[:65].contiguous()).cpu().numpy()
            assert np.array_equal(out, np.broadcast_to(zero["linear"]["bias"], out.shape)), (basis, D, K, R, kern)


# ---- 2. slices ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,QG", [(1, 8), (2, 4), (4, 2), (4, 1)])
@pytest.mark.parametrize("R,K", [(3, 50), (1, 10)])
def test_forced_slices(gpu, R, K, S, QG):
    """R = 3, K = 50: six chunks, slice boundaries inside a region; R = 1, K = 10: one chunk, empty slices."""
    _, cfg, params, x = _case(S * 10 + QG + R, R, K, "gaussian", 333)
    gamma = softmax_gamma(params, x).astype(np.float32)
    ref, scale = gamma_forward64(cfg, params, x, gamma)
    stage = ClusterWCRBFNet(**cfg).stage.set_options(fwd_gamma_kernel=_lib.FWDG_K1G, fwd_f16_s=S, fwd_f16_qg=QG)
    stage.bind(_rbf(params))
    xt, gt = torch.from_numpy(x).cuda(), torch.from_numpy(gamma).cuda()
    out = _fwd(stage, xt, gt)
    ll = stage.last_launch()
    assert ll["kernel"].startswith(NAME["k1g"]) and ll["kernel"].endswith(f"S={S},QG={QG}>") and ll["block"] == 64 * S * QG, ll
    _check(out.cpu().numpy(), ref, scale, (R, K, S, QG))
    assert torch.equal(out, _fwd(stage, xt, gt))


# ---- 3. gamma values ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern", list(KERNELS))
def test_gamma_values(gpu, kern):
    """Hand-made region weights through the C ABI: whole regions at exact 0, one-hot rows, rows of 1e-30, uniform in [-1, 1]; a
    NaN in one gamma row gives a NaN output row and leaves the other 31 rows of its wave within the bound."""
    R, K, B = 11, 33, 200
    rng, cfg, params, x = _case(33, R, K, "gaussian", B)
    stage = ClusterWCRBFNet(**cfg).stage.set_options(fwd_gamma_kernel=KERNELS[kern])
    stage.bind(_rbf(params))
    xt = torch.from_numpy(x).cuda()
    soft = softmax_gamma(params, x).astype(np.float32)
    zeros = soft.copy(); zeros[:, [0, 4, 5, 10]] = 0.0
    onehot = np.zeros((B, R), np.float32); onehot[np.arange(B), rng.integers(0, R, size=B)] = 1.0
    tiny = soft.copy(); tiny[::3] = 1e-30
    signed = rng.uniform(-1, 1, size=(B, R)).astype(np.float32)
    for what, g in (("zero regions", zeros), ("one-hot", onehot), ("rows of 1e-30", tiny), ("uniform [-1, 1]", signed),
                    ("all zero", np.zeros((B, R), np.float32))):
        ref, scale = gamma_forward64(cfg, params, x, g)
        out = _fwd(stage, xt, torch.from_numpy(g).cuda())
        _check(out.cpu().numpy(), ref, scale, (what, kern))
    nan = signed.copy(); nan[37, 6] = np.nan                        # row 37: wave 1 of the batch (rows 32..63)
    ref, scale = gamma_forward64(cfg, params, x, nan)
    out = _fwd(stage, xt, torch.from_numpy(nan).cuda()).cpu().numpy()
    assert np.isnan(out[37]).all(), out[37]
    keep = np.arange(B) != 37
    _check(out[keep], ref[keep], scale[keep], ("NaN row", kern))


# ---- 4. reference shape ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [50, 10])
def test_reference_shape(gpu, K):
    """R = 500, D = 8, O = 10 at B = 65 536 through ``ClusterWCRBFNet.apply``: 512 sampled rows and the last 77 against float64;
    bitwise repeat; a row permutation gives the same rows bit for bit; back on FWDG_AUTO the gated K1 returns the bits it
    returned before the option was ever set."""
    B, R = 65536, 500
    rng, cfg, params, x = _case(K, R, K, "gaussian", B)
    net = ClusterWCRBFNet(**cfg)
    xt = torch.from_numpy(x).cuda()
    before, logits0 = net.apply(params, xt)
    assert net.stage.last_launch()["kernel"].startswith("rbf_fwd_qlane<")
    assert net.set_options(fwd_gamma_kernel=_lib.FWDG_K1G) is net
    out, logits = net.apply(params, xt)
    assert net.stage.last_launch()["kernel"].startswith("rbf_fwd_f16gram_gamma<D=8,BC=0,"), net.stage.last_launch()
    assert torch.equal(logits, logits0)
    rows = np.unique(np.concatenate([rng.choice(B - 77, size=512, replace=False), np.arange(B - 77, B)]))
    _, gamma = net._bind_and_gate(params, xt, torch, _lib.load())
    ref, scale = gamma_forward64(cfg, params, x[rows], gamma.cpu().numpy()[rows])
    _check(out.cpu().numpy()[rows], ref, scale, ("reference shape", K, "k1g"))
    _check(before.cpu().numpy()[rows], ref, scale, ("reference shape", K, "k1"))
    assert torch.equal(out, net.apply(params, xt)[0])
    perm = torch.from_numpy(rng.permutation(B)).cuda()
    assert torch.equal(net.apply(params, xt[perm])[0], out[perm])
    net.set_options(fwd_gamma_kernel=_lib.FWDG_AUTO)
    again, _ = net.apply(params, xt)
    assert net.stage.last_launch()["kernel"].startswith("rbf_fwd_qlane<")
    assert torch.equal(again, before)


# ---- 5. outside the box ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("basis", FAST)
def test_queries_outside_the_box(gpu, basis):
    """Queries at +-3 (beyond 1.25 x the centres' box: their waves take the VALU distances) and +-Inf / NaN rows mixed into
    in-box batches: the bound on finite rows; non-finite rows as the gated K1 has them."""
    R, K, B = 11, 50, 500
    rng, cfg, params, x = _case(55, R, K, basis, B)
    far = np.arange(5, B, 41)
    x[far] = rng.choice([-3.0, 3.0], size=(far.size, 8)).astype(np.float32)
    x[far[::2], 3:] = rng.uniform(-2, 2, size=(far[::2].size, 5)).astype(np.float32)       # some coordinates out, some in
    finite = x.copy()
    odd = np.array([70, 71, 200, 333])
    x[70, 2], x[71, 5], x[200, 0], x[333, 7] = np.inf, -np.inf, np.nan, np.inf
    gamma = softmax_gamma(params, finite).astype(np.float32)
    outs = {}
    for kern in KERNELS:
        stage = ClusterWCRBFNet(**cfg).stage.set_options(fwd_gamma_kernel=KERNELS[kern])
        stage.bind(_rbf(params))
        outs[kern] = _fwd(stage, torch.from_numpy(x).cuda(), torch.from_numpy(gamma).cuda()).cpu().numpy()
    ok = np.setdiff1d(np.arange(B), odd)
    ref, scale = gamma_forward64(cfg, params, x[ok], gamma[ok])
    for kern in KERNELS:
        _check(outs[kern][ok], ref, scale, ("outside the box", basis, kern))
    a, b = outs["k1g"][odd], outs["k1"][odd]
    assert np.array_equal(np.isnan(a), np.isnan(b)), (a, b)
    m = ~np.isnan(a)
    assert np.isfinite(a[m]).all() and np.abs(a[m] - b[m]).max(initial=0.0) <= 1e-5 * (1 + np.abs(b[m]).max(initial=0.0))


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------
def _tick(stage, mode, xt, gt, mt, st, ctrl, states, T, expect=OK):
    lib = _lib.load()
    null = C.c_void_p(None)
    opt = lambda t: _ptr(t) if t is not None else null
    keep, pp = dyn._dyn(configs.DYN_PARAMS)                          # keep: the host array behind pp
    rc = lib.irbfn_plan_tick_gamma(stage._handle(torch), mode, _ptr(xt), _ptr(gt), opt(mt), opt(st), pp, opt(ctrl), opt(states),
                                   xt.shape[0], T, _stream_ptr(torch))
    assert rc == expect, (rc, expect)


@pytest.mark.parametrize("what", ["narrow widths", "generic basis", "O = 18"])
def test_refusals(gpu, what):
    """Parameters outside the expansion's budget (log sigma = -7), a generic basis, O = 18: IRBFN_ERR_UNSUPPORTED from both entry
    points, nothing launched in its place, and the default path still answers."""
    basis = "matern52" if what == "generic basis" else "gaussian"
    O = 18 if what == "O = 18" else 10
    R, K, B, T = 3, 40, 100, O // 2
    rng, cfg, params, x = _case(6, R, K, basis, B, O=O)
    if what == "narrow widths":
        params["params"]["rbf_list"]["log_sigs"][:] = -7.0
    stage = ClusterWCRBFNet(**cfg).stage
    stage.bind(_rbf(params))
    xt = torch.from_numpy(x).cuda()
    gt = torch.from_numpy(softmax_gamma(params, x).astype(np.float32)).cuda()
    st = torch.zeros((B, 8), dtype=torch.float32, device="cuda"); st[:, 3] = 2.0
    ctrl = torch.empty((B, O), dtype=torch.float32, device="cuda")
    states = torch.empty((B, T, 8), dtype=torch.float32, device="cuda")
    base = _fwd(stage, xt, gt)
    stage.set_options(fwd_gamma_kernel=_lib.FWDG_K1G)
    stage.bind(_rbf(params))
    _fwd(stage, xt, gt, expect=UNSUPPORTED)
    _tick(stage, _lib.ROLLOUT_FRENET_LS, xt, gt, None, st, ctrl, states, T, expect=UNSUPPORTED)
    _tick(stage, _lib.ROLLOUT_FRENET_LS, xt, gt, None, None, ctrl, None, T, expect=UNSUPPORTED)
    stage.set_options(fwd_gamma_kernel=_lib.FWDG_AUTO)
    assert torch.equal(_fwd(stage, xt, gt), base)
    assert stage.last_launch()["kernel"].startswith("rbf_fwd_qlane<")
    _tick(stage, _lib.ROLLOUT_FRENET_LS, xt, gt, None, st, ctrl, states, T)


def test_option_needs_a_bind(gpu):
    """The option selected after a bind: IRBFN_ERR_NO_PARAMS from C until the next irbfn_net_set_params; the Python classes bind
    again by themselves; two binds with different parameters give the second parameters' result."""
    lib = _lib.load()
    R, K, B = 5, 40, 300
    _, cfg, params, x = _case(7, R, K, "gaussian", B)
    _, _, params2, _ = _case(8, R, K, "gaussian", B)
    net = ClusterWCRBFNet(**cfg)
    xt = torch.from_numpy(x).cuda()
    net.apply(params, xt)
    gt = torch.from_numpy(softmax_gamma(params, x).astype(np.float32)).cuda()
    h = net.stage._handle(torch)
    assert lib.irbfn_net_set_option(h, _lib.OPTIONS["fwd_gamma_kernel"], _lib.FWDG_K1G) == OK          # behind Python's back
    got = C.c_int(-1)
    assert lib.irbfn_net_get_option(h, _lib.OPTIONS["fwd_gamma_kernel"], C.byref(got)) == OK and got.value == _lib.FWDG_K1G
    assert lib.irbfn_net_set_option(h, _lib.OPTIONS["fwd_gamma_kernel"], 3) == -1
    _fwd(net.stage, xt, gt, expect=NO_PARAMS)
    ctrl = torch.empty((B, 10), dtype=torch.float32, device="cuda")
    _tick(net.stage, _lib.ROLLOUT_FRENET_LS, xt, gt, None, None, ctrl, None, 5, expect=NO_PARAMS)
    net.set_options(fwd_gamma_kernel=_lib.FWDG_K1G)                  # forgets the bind: apply packs again
    for p in (params, params2, params):
        out, _ = net.apply(p, xt)
        assert net.stage.last_launch()["kernel"].startswith(NAME["k1g"])
        g = softmax_gamma(p, x)
        _, gam = net._bind_and_gate(p, xt, torch, lib)
        ref, scale = gamma_forward64(cfg, p, x, gam.cpu().numpy())
        np.testing.assert_allclose(gam.cpu().numpy(), g, rtol=2e-5, atol=1e-6)
        _check(out.cpu().numpy(), ref, scale, "rebind")
    # switched off, the images are not packed: selecting the kernel again asks for a bind again
    net.set_options(fwd_gamma_kernel=_lib.FWDG_AUTO)
    net.apply(params2, xt)
    assert lib.irbfn_net_set_option(h, _lib.OPTIONS["fwd_gamma_kernel"], _lib.FWDG_K1G) == OK
    _fwd(net.stage, xt, gt, expect=NO_PARAMS)


# ---- 7. tick --------------------------------------------------------------------------------------------------------------
def _state0(rng, frenet, B):
    if frenet:
        return np.hstack([rng.normal(size=(B, 1)) * 0.2, rng.normal(size=(B, 1)) * 0.2, rng.normal(size=(B, 1)) * 0.1,
                          rng.uniform(1, 6, size=(B, 1)), rng.normal(size=(B, 3)) * 0.1, rng.normal(size=(B, 1)) * 0.05]).astype(np.float32)
    return np.hstack([rng.normal(size=(B, 3)) * 0.3, rng.uniform(0.5, 7.0, size=(B, 1)), rng.normal(size=(B, 3)) * 0.2]).astype(np.float32)


@pytest.mark.parametrize("T", [1, 5, 8])
@pytest.mark.parametrize("D,mode", [(8, _lib.ROLLOUT_FRENET_LS), (7, _lib.ROLLOUT_ST_KS)])
def test_tick(gpu, D, mode, T):
    """irbfn_plan_tick_gamma with the option, ragged B, with and without mirror flags and a controls buffer: bit-equal to
    irbfn_net_forward_gamma (same option) -> sign flip -> irbfn_rollout_forward; states against the oracle roll-out."""
    R, K, B, O = 7, 50, 333, 2 * T
    rng, cfg, params, x = _case(70 + T + D, R, K, "gaussian", B, D=D, O=O)
    params["params"]["linear"]["kernel"] *= 0.1                       # controls of a size the dynamics are tested at
    params["params"]["linear"]["bias"] *= 0.1
    frenet = mode == _lib.ROLLOUT_FRENET_LS
    S = 8 if frenet else 7
    stage = ClusterWCRBFNet(**cfg).stage.set_options(fwd_gamma_kernel=_lib.FWDG_K1G)
    stage.bind(_rbf(params))
    xt = torch.from_numpy(x).cuda()
    gt = torch.from_numpy(softmax_gamma(params, x).astype(np.float32)).cuda()
    st = torch.from_numpy(_state0(rng, frenet, B)).cuda()
    mt = torch.from_numpy((rng.uniform(size=B) < 0.4).astype(np.int32)).cuda()
    plain = _fwd(stage, xt, gt)
    ref, scale = gamma_forward64(cfg, params, x, gt.cpu().numpy())
    _check(plain.cpu().numpy(), ref, scale, ("tick forward", D, T))
    for flags in (mt, None):
        u = plain.clone()
        if flags is not None:
            u[:, T:] = torch.where(flags[:, None] != 0, -u[:, T:], u[:, T:])
        two = dyn.rollout_forward(mode, torch.cat([st, u], dim=1), configs.DYN_PARAMS, T)
        for with_ctrl in (True, False):
            ctrl = torch.full((B, O), 9.0, dtype=torch.float32, device="cuda") if with_ctrl else None
            states = torch.full((B, T, S), 9.0, dtype=torch.float32, device="cuda")
            _tick(stage, mode, xt, gt, flags, st, ctrl, states, T)
            kern = stage.last_launch()["kernel"]
            assert kern.startswith(f"rbf_tick_f16gram_gamma<D={D},BC=0,MODE={mode},"), kern
            assert torch.equal(states, two), (D, T, flags is not None, with_ctrl)
            if with_ctrl:
                assert torch.equal(ctrl, u)
        ctrl = torch.empty((B, O), dtype=torch.float32, device="cuda")
        _tick(stage, mode, xt, gt, flags, None, ctrl, None, T)       # controls only
        assert torch.equal(ctrl, u)
    xu = np.hstack([st.cpu().numpy(), u.cpu().numpy()])
    integ = orc.integrate_frenet_mult if frenet else orc.integrate_st_ks_mult
    assert_states_close(states.cpu().numpy(), integ(xu.astype(np.float64), DP), integ(xu, DP.astype(np.float32)))
    # the composed form (IRBFN_OPT_TICK_FUSED = 0) goes through the controls buffer with the same forward
    stage.set_options(tick_fused=0)
    ctrl = torch.empty((B, O), dtype=torch.float32, device="cuda")
    states2 = torch.empty((B, T, S), dtype=torch.float32, device="cuda")
    _tick(stage, mode, xt, gt, None, st, ctrl, states2, T)
    assert torch.equal(states2, states) and torch.equal(ctrl, plain)
    _tick(stage, mode, xt, gt, None, st, None, states2, T, expect=-1)


def test_tick_through_planner(gpu):
    """``planner.plan_tick`` of a ClusterWCRBFNet with the option: the one-launch tick, equal to apply -> flip -> roll-out."""
    R, K, B, T = 11, 50, 1000, 5
    rng, cfg, params, x = _case(77, R, K, "gaussian", B)
    params["params"]["linear"]["kernel"] *= 0.1
    net = ClusterWCRBFNet(**cfg).set_options(fwd_gamma_kernel=_lib.FWDG_K1G)
    xt, st = torch.from_numpy(x).cuda(), torch.from_numpy(_state0(rng, True, B)).cuda()
    plain, _ = net.apply(params, xt)
    ctrl, states = planner.plan_tick(net, params, xt, None, st, configs.DYN_PARAMS, mode=_lib.ROLLOUT_FRENET_LS)
    assert net.stage.last_launch()["kernel"].startswith("rbf_tick_f16gram_gamma<D=8,")
    assert torch.equal(ctrl, plain)
    assert torch.equal(states, dyn.rollout_forward(_lib.ROLLOUT_FRENET_LS, torch.cat([st, plain], dim=1), configs.DYN_PARAMS, T))


# ---- 8. trained net -------------------------------------------------------------------------------------------------------
def test_trained_12_region_planner(gpu):
    """The golden 12-region Frenet checkpoint (K = 100: four chunks per region, 28 padding centres each) through irbfn_net_gate ->
    irbfn_net_forward_gamma with the option, its 64 stored queries tiled to B = 4096, against the fixture's float64 outputs at
    the bound tests/test_gpu_parity.py::test_forward_trained_checkpoints uses."""
    cfg, params, x, out64, h64, _ = load_ckpt_fixture("dnmpc_12regions_frenet_l1_bigdata")
    net = WCRBFNet.from_config(cfg).set_options(fwd_gamma_kernel=_lib.FWDG_K1G)
    net.bind(params)
    reps = 4096 // x.shape[0]
    xt = torch.from_numpy(np.tile(x.astype(np.float32), (reps, 1))).cuda()
    gt = net.gate(xt)
    out = _fwd(net, xt, gt if isinstance(gt, torch.Tensor) else torch.from_numpy(np.asarray(gt)).cuda())
    assert net.last_launch()["kernel"].startswith("rbf_fwd_f16gram_gamma<D=8,"), net.last_launch()
    scale = np.tile(np.abs(h64) @ np.abs(np.asarray(params["params"]["linear"]["kernel"], np.float64)), (reps, 1))
    ref = np.tile(out64, (reps, 1))
    err = np.abs(out.cpu().numpy().astype(np.float64) - ref)
    print(f"cluster_gram trained 12-region net: max err / bound = {(err / (RTOL * np.abs(ref) + 3e-6 * scale)).max():.3f}")
    assert (err <= RTOL * np.abs(ref) + 3e-6 * scale).all(), (err.max(), scale.max())
