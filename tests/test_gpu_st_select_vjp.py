"""The ST_SELECT roll-out VJP (irbfn_rollout_vjp_select: rollout_vjp_regs_kernel<ST_SELECT, 8 / 50> up to T = 50,
rollout_vjp_park_kernel<ST_SELECT> up to T = 120) against the float64 NumPy statement of its formulas (_st_select_util.py, held to
torch.autograd by test_st_select_reference_cpu.py), and its torch.autograd surface.  The bound is the one
test_gpu_parity.test_rollout_vjps_match_hand_adjoints applies to ST_KS: 5e-5 max|ref| + 1e-6 (>= 13 x the error of the float32
evaluation of the same lines on these inputs)."""
import numpy as np
import pytest

from irbfn_amd import _lib, configs
from irbfn_amd import dynamics as dyn

import _st_select_util as su

pytestmark = pytest.mark.gpu
DP = np.array(configs.DYN_PARAMS, np.float32).astype(np.float64)      # what the kernels get, widened: exact bounds stay exact
F32 = np.float32
SHAPES = [(1, 1), (63, 5), (64, 8), (65, 9), (257, 50),              # K4: both instances, their boundary at T = 8, B around a wave and a block
          (64, 51), (70, 120)]                                        # the park kernel, up to its last horizon
_cache = {}


def _case(B, T):
    if (B, T) not in _cache:
        xu = su.grid_inputs(B, T, seed=100 * T + B)
        gs = su._f32(np.random.default_rng(T + B).normal(size=(B, T, 7)))
        ref = su.vjp_st_select(xu, DP, gs)
        for a in (xu, gs, ref):
            a.setflags(write=False)
        _cache[(B, T)] = (xu, gs, ref)
    return _cache[(B, T)]


def _close(got, ref):
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all()
    err, tol = np.abs(got - ref).max(), 5e-5 * np.abs(ref).max() + 1e-6
    print(f"[st_select_vjp] err {err:.3e} bound {tol:.3e} max|ref| {np.abs(ref).max():.3e}")
    assert err <= tol, (err, tol)


def _vjp(xu, gs, T, tie=0.5):
    return dyn.rollout_vjp_select(np.asarray(xu, F32), DP, np.asarray(gs, F32), T, clip_tie=tie)


@pytest.mark.parametrize("B,T", SHAPES, ids=lambda v: str(v))
def test_matches_the_float64_statement(gpu, B, T):
    xu, gs, ref = _case(B, T)
    got = _vjp(xu, gs, T)
    _close(got, ref)
    np.testing.assert_array_equal(_vjp(xu, gs, T), got)               # repeats are bit-equal


def test_horizon_limits(gpu):
    with pytest.raises(ValueError):
        _vjp(np.zeros((4, 7 + 2 * 121)), np.zeros((4, 121, 7)), 121)
    x0 = su.grid_inputs(9, 0, seed=1)
    got = _vjp(x0, np.zeros((9, 0, 7)), 0)
    assert got.shape == x0.shape and (got == 0).all()
    assert _vjp(np.zeros((0, 17)), np.zeros((0, 5, 7)), 5).shape == (0, 17)
    with pytest.raises(ValueError):                                    # irbfn_rollout_vjp is what the reference differentiates
        dyn.rollout_vjp(_lib.ROLLOUT_ST_SELECT, np.zeros((4, 17), F32), DP, np.zeros((4, 5, 7), F32), 5)


@pytest.mark.parametrize("B,T", [(65, 9), (64, 51)], ids=lambda v: str(v))
def test_linear_in_the_cotangent(gpu, B, T):
    xu, g1, _ = _case(B, T)
    g2 = su._f32(np.random.default_rng(7).normal(size=g1.shape))
    a, b = 0.75, -1.5
    lhs = _vjp(xu, su._f32(a * g1 + b * g2), T).astype(np.float64)
    rhs = a * _vjp(xu, g1, T).astype(np.float64) + b * _vjp(xu, g2, T).astype(np.float64)
    assert np.abs(lhs - rhs).max() <= 1e-4 * np.abs(rhs).max()


@pytest.mark.parametrize("B,T", [(65, 9), (130, 50), (64, 51)], ids=lambda v: str(v))
def test_kinematic_only_batch_agrees_with_st_ks(gpu, B, T):
    """v0 <= 2 and a <= 0: no step is dynamic, and every lane runs ST_KS's expressions in ST_KS's order.  The two kernels agree
    to the bound, not bit for bit (measured: max difference 1e-6 .. 2e-4 at max|ref| 2e1 .. 1e3): the compiler contracts
    multiply-adds of the same expressions differently inside the two instances."""
    rng = np.random.default_rng(B + T)
    xu = np.array(su.grid_inputs(B, T, seed=3 * T))
    xu[:, 3] = 0.1 + 0.25 * (np.arange(B) % 8)                         # 0.1 .. 1.85
    xu[:, 3][::9] = 0.0                                                # standing rows: V = 0 wherever a = 0 too
    xu[:, 7:7 + T] = -2.5 * rng.integers(0, 2, size=(B, T))
    xu[::9, 7:7 + T] = 0.0
    xu = su._f32(xu)
    gs = su._f32(rng.normal(size=(B, T, 7)))
    V = su.clipped_speeds(xu, DP)
    assert not (V > su.SWITCH).any() and (V[::9] == 0).all()
    ref = su.vjp_st_select(xu, DP, gs)
    got = _vjp(xu, gs, T)
    assert np.isfinite(got[::9]).all()                                 # V = 0: the dynamic quantities there are inf / nan
    _close(got, ref)
    ks = dyn.rollout_vjp(_lib.ROLLOUT_ST_KS, xu.astype(F32), DP, gs.astype(F32), T)
    _close(ks, ref)
    _close(got, np.asarray(ks, np.float64))
    print(f"[st_select_vjp] kinematic-only (B, T) = ({B}, {T}): bit-equal to rollout_vjp(ST_KS): {np.array_equal(got, ks)}")


def test_standing_rows_in_a_mixed_batch_are_finite(gpu):
    B, T = 64, 8
    xu = np.array(_case(B, T)[0])
    gs = _case(B, T)[1]
    xu[::4, 3] = 0.0
    xu[::4, 7:7 + T] = 0.0
    xu = su._f32(xu)
    got = _vjp(xu, gs, T)
    assert np.isfinite(got).all()
    _close(got, su.vjp_st_select(xu, DP, gs))


@pytest.mark.parametrize("tie", [0.0, 0.5, 1.0])
def test_clip_ties_on_exact_bounds_at_step_zero(gpu, tie):
    B, T = 66, 5
    xu = np.array(su.grid_inputs(B, T, seed=17))
    r = np.arange(B) % 6
    sgn = np.where(np.arange(B) % 12 < 6, 1.0, -1.0)
    xu[r == 0, 3] = (sgn * DP[12])[r == 0]                             # V = +-v_max; +v_max is a dynamic step
    xu[r == 0, 7] = (-2.5 * sgn)[r == 0]
    xu[r == 1, 2] = (sgn * DP[11])[r == 1]                             # delta = +-s_max
    xu[r == 2, 7] = (sgn * DP[10])[r == 2]                             # a_0 = +-a_max
    xu[r == 3, 7 + T] = (sgn * DP[9])[r == 3]                          # sv_0 = +-sv_max
    xu = su._f32(xu)
    su.assert_off_switch(xu, DP)
    gs = su._f32(np.random.default_rng(18).normal(size=(B, T, 7)))
    assert (xu[r == 0, 3] == sgn[r == 0] * DP[12]).all() and (xu[r == 1, 2] == sgn[r == 1] * DP[11]).all()
    ref = su.vjp_st_select(xu, DP, gs, tie)
    _close(_vjp(xu, gs, T, tie), ref)
    if tie != 0.5:                                                     # the rule is visible in the reference
        assert np.abs(ref - su.vjp_st_select(xu, DP, gs, 0.5)).max() > 1e-3 * np.abs(ref).max()


@pytest.mark.parametrize("B,T", [(65, 9), (64, 51)], ids=lambda v: str(v))
def test_nan_stays_in_its_row(gpu, B, T):
    xu, gs, _ = _case(B, T)
    clean = _vjp(xu, gs, T)
    bad = np.array(xu)
    bad[5, 4] = np.nan                                                 # heading of row 5
    got = _vjp(bad, gs, T)
    assert np.isnan(got[5]).any()
    keep = np.arange(B) != 5
    np.testing.assert_array_equal(got[keep], clean[keep])


def test_autograd_backward_is_the_vjp_call(gpu):
    import torch
    from irbfn_amd import autograd as ag
    B, T = 65, 9
    xu, gs, _ = _case(B, T)
    xt = torch.tensor(xu, dtype=torch.float32, device="cuda", requires_grad=True)
    gt = torch.tensor(gs, dtype=torch.float32, device="cuda")
    states = ag.integrate_st_mult(xt, DP, clip_tie=1.0)
    assert torch.equal(states, dyn.integrate_st_mult(xt.detach(), DP))
    (states * gt).sum().backward()
    assert torch.equal(xt.grad, dyn.rollout_vjp_select(xt.detach(), DP, gt, T, clip_tie=1.0))


def test_query_to_rollout_end_to_end(gpu):
    """wcrbf_apply -> hstack -> integrate_st_mult -> sum(g * states): the leaf gradients and x.grad are the composition of
    rollout_vjp_select with net.vjp / net.vjp_x, bit for bit."""
    import torch
    from irbfn_amd import autograd as ag
    from irbfn_amd.model import WCRBFNet
    K, D, O, B = 64, 7, 10, 96
    T = O // 2
    rng = np.random.default_rng(23)
    net = WCRBFNet.from_config(dict(configs.model_card(2), num_kernels=K, out_features=O))
    dev = lambda a, rg=False: torch.tensor(np.asarray(a, F32), device="cuda", requires_grad=rg)
    leaves = {"rbf_list": {"centers": dev(rng.uniform(-1, 8, size=(1, K, D)), True), "log_sigs": dev(rng.uniform(0, 2, size=(1, K)), True)},
              "linear": {"kernel": dev(rng.normal(size=(K, O)) * 0.3, True), "bias": dev(np.zeros(O), True)}}
    x = dev(configs.synth_queries(2, B=B), True)
    state0 = dev(su.grid_inputs(B, 0, seed=24))
    g = dev(rng.normal(size=(B, T, 7)))
    u = ag.wcrbf_apply(net, {"params": leaves}, x)
    states = ag.integrate_st_mult(torch.hstack((state0, u)), DP)
    (states * g).sum().backward()
    with torch.no_grad():
        detached = {k: {n: t.detach() for n, t in d.items()} for k, d in leaves.items()}
        u0 = net.apply({"params": detached}, x.detach())
        assert torch.equal(u0, u.detach())
        gu = dyn.rollout_vjp_select(torch.hstack((state0, u0)), DP, g, T)[:, 7:].contiguous()
        want = net.vjp({"params": detached}, x.detach(), gu)["params"]
        want_x = net.vjp_x({"params": detached}, x.detach(), gu)
    assert torch.isfinite(x.grad).all() and float(x.grad.abs().max()) > 0
    assert torch.equal(x.grad, want_x)
    for k, d in leaves.items():
        for n, t in d.items():
            assert torch.equal(t.grad, want[k][n]), (k, n)
