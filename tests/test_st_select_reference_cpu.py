"""CPU checks of the statements in _st_select_util.py: the NumPy statement of the ST_SELECT adjoint (what
vjp_back_step<ST_SELECT> computes) against torch.autograd of the float64 restatement of integrate_st_mult, at the places where a
branch-wise adjoint can go wrong (trajectories that cross V = 3, V = 0, V = 3 exactly, exact clip bounds); the seeds of
irbfn_train_seeds_st_fullint against torch.autograd of their loss; and the two new entry points' signatures."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from irbfn_amd import _lib
from oracle import hand_vjp as hv
from oracle import irbfn_oracle as orc

import _st_select_util as su
import _train_step_util as tu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP = su.DP
TOL = 1e-12


def _check(xu, gs, tie=0.5, dp=DP):
    ref, states, V = su.autograd_vjp(xu, dp, gs)
    got = su.vjp_st_select(xu, dp, gs, tie)
    assert np.isfinite(ref).all() and np.isfinite(got).all()
    assert np.abs(got - ref).max() <= TOL * np.abs(ref).max(), (np.abs(got - ref).max(), np.abs(ref).max())
    return got, states, V


@pytest.mark.parametrize("T", [1, 5, 50])
def test_hand_adjoint_matches_autograd_on_the_grid(T):
    B = 300
    xu = su.grid_inputs(B, T, seed=10 + T)
    gs = np.random.default_rng(T).normal(size=(B, T, 7))
    _, states, V = _check(xu, gs)
    dyn = V > su.SWITCH
    assert 0.3 < dyn.mean() < 0.8                     # both branches carry weight
    with np.errstate(divide="ignore", invalid="ignore"):
        np.testing.assert_allclose(states, orc.integrate_st_mult(xu, DP), rtol=1e-12, atol=1e-12)    # (a) is the oracle's forward


def test_rows_that_cross_the_switch_both_ways():
    T = 8
    rng = np.random.default_rng(3)
    xu = su.grid_inputs(54, T, seed=4)
    xu[:27, 3], xu[:27, 7:7 + T] = 2.6, 2.5           # 2.6, 2.85, 3.1, ...: upwards
    xu[27:, 3], xu[27:, 7:7 + T] = 3.35, -2.5         # 3.35, 3.1, 2.85, ...: downwards
    xu = su._f32(xu)
    V = su.assert_off_switch(xu)
    dyn = V > su.SWITCH
    up = (~dyn[:, :-1] & dyn[:, 1:]).any(axis=1)
    down = (dyn[:, :-1] & ~dyn[:, 1:]).any(axis=1)
    assert up[:27].all() and down[27:].all()
    _check(xu, rng.normal(size=(54, T, 7)))


def test_standing_rows_are_finite_and_kinematic():
    T = 5
    rng = np.random.default_rng(5)
    xu = su.grid_inputs(40, T, seed=6)
    xu[:, 3] = 0.0
    xu[:, 7:7 + T] = 0.0                              # v0 = 0, a = 0: V = 0 at every step
    gs = rng.normal(size=(40, T, 7))
    got, _, V = _check(xu, gs)
    assert (V == 0).all()
    np.testing.assert_array_equal(got, hv.vjp_st_ks(xu, DP, gs))
    got32 = su.vjp_st_select(xu, DP, gs, ft=np.float32)
    assert np.isfinite(got32).all()


def test_speed_exactly_on_the_switch_is_kinematic():
    rng = np.random.default_rng(7)
    xu = su.grid_inputs(27, 1, seed=8)
    xu[:, 3] = 3.0
    gs = rng.normal(size=(27, 1, 7))
    got, states, _ = _check(xu, gs)
    np.testing.assert_array_equal(got, su.vjp_st_select(xu, DP, gs, select=False))
    np.testing.assert_array_equal(got, hv.vjp_st_ks(xu, DP, gs))
    np.testing.assert_allclose(states, orc.integrate_st_ks_mult(xu, DP), rtol=1e-13, atol=1e-13)
    xu[:, 3] = np.nextafter(3.0, 4.0)                 # the next speed up is dynamic
    above = su.vjp_st_select(xu, DP, gs)
    assert (above[:, 5:7] != got[:, 5:7]).any()


@pytest.mark.parametrize("which", ["v", "delta"])
def test_exact_clip_bounds_at_step_zero(which):
    """torch.clip passes gradient 1 on a bound: tie = 1 is autograd's answer; tie = 0 is the answer just outside the bound; the
    result is linear in tie."""
    T = 3
    rng = np.random.default_rng(9)
    col, bound = (3, DP[12]) if which == "v" else (2, DP[11])
    xu = su.grid_inputs(54, T, seed=11)
    sign = np.where(np.arange(54) % 2 == 0, 1.0, -1.0)
    xu[:, col] = sign * bound
    if which == "v":
        xu[:, 7] = -2.5 * sign                        # the speed leaves the bound after step 0
    gs = rng.normal(size=(54, T, 7))
    g = {tie: su.vjp_st_select(xu, DP, gs, tie) for tie in (0.0, 0.5, 1.0)}
    ref, _, V = su.autograd_vjp(xu, DP, gs)
    assert (V[:, 0] == sign * DP[12]).all() if which == "v" else True
    scale = np.abs(ref).max()
    assert np.abs(g[1.0] - ref).max() <= TOL * scale
    outside = xu.copy()
    outside[:, col] = sign * bound * (1 + 1e-12)
    assert np.abs(g[0.0] - su.vjp_st_select(outside, DP, gs, 0.5)).max() <= 1e-9 * scale
    assert np.abs(g[0.5] - 0.5 * (g[0.0] + g[1.0])).max() <= TOL * scale
    assert np.abs(g[1.0] - g[0.0]).max() > 1e-3 * scale          # the tie rule is visible


def test_float32_twin_is_close():
    """the float32 evaluation of the same lines: the error the GPU bound 5e-5 max|ref| + 1e-6 is measured against"""
    for B, T in ((300, 5), (300, 50), (64, 120)):
        xu = su.grid_inputs(B, T, seed=20 + T)
        gs = su._f32(np.random.default_rng(T).normal(size=(B, T, 7)))
        ref = su.vjp_st_select(xu, DP, gs)
        twin = su.vjp_st_select(xu, DP, gs, ft=np.float32)
        assert twin.dtype == np.float32
        assert np.abs(twin - ref).max() <= (5e-5 / 4) * np.abs(ref).max()


def _seed_autograd(x, yp, y, select):
    xt, ypt, yt = (torch.tensor(a) for a in (x, yp, y))
    ypt.requires_grad_(True)
    z = torch.zeros_like(xt[:, 0])
    init = torch.stack([z, z, z, xt[:, 0], z, xt[:, 6], xt[:, 5]], -1)
    dp = [float(c) for c in DP]
    pred, _ = su.st_select_torch(torch.hstack([init, ypt]), dp, select=select)
    act, _ = su.st_select_torch(torch.hstack([init, yt]), dp, select=select)
    loss = (ypt - yt).abs().mean() + (pred[:, :, su.STATE_IDX] - act[:, :, su.STATE_IDX]).abs().mean()
    loss.backward()
    return float(loss.detach()), ypt.grad.numpy()


@pytest.mark.parametrize("select", [True, False])
@pytest.mark.parametrize("T,D", [(1, 7), (5, 7), (16, 9)])
def test_seeds_match_autograd_of_their_loss(select, T, D):
    x, yp, y = su.seed_case(257, T, D, seed=30 + T)
    loss, gy, amb = su.seeds_st_fullint(x, yp, y, DP, 1.0, select)       # torch.clip: gradient 1 on a bound
    assert amb.mean() <= tu.AMBIGUOUS_CAP
    ref_loss, ref = _seed_autograd(x, yp, y, select)
    assert abs(loss - ref_loss) <= 1e-12 * abs(ref_loss)
    assert np.abs(gy - ref).max() <= TOL * np.abs(ref).max()
    # a share of a batch: the means divide by B_total
    part = su.seeds_st_fullint(x[:10], yp[:10], y[:10], DP, 1.0, select, B_total=257)[1]
    np.testing.assert_allclose(part, gy[:10], rtol=1e-13, atol=0)
    loss32, gy32, _ = su.seeds_st_fullint(x, yp, y, DP, 1.0, select, ft=np.float32)
    assert gy32.dtype == np.float32 and np.abs(gy32[~amb] - gy[~amb]).max() <= tu.TWIN_CAP * np.abs(gy).max()


_CTYPE = {"const float*": C.c_void_p, "float*": C.c_void_p, "void*": C.c_void_p, "int": C.c_int, "int64_t": C.c_int64,
          "float": C.c_float}


def _header_signature(name):
    hdr = open(os.path.join(ROOT, "include", "irbfn_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert m, name
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    return [(a.rsplit(" ", 1)[0], a.rsplit(" ", 1)[1]) for a in args]


def test_new_entry_points_header_and_binding_agree():
    want = {
        "irbfn_rollout_vjp_select": ["x0u_dev", "dyn_params_host", "gstates_dev", "g_x0u_dev", "B", "T", "clip_tie", "stream"],
        "irbfn_train_seeds_st_fullint": ["mode", "x_dev", "y_pred_dev", "y_dev", "dyn_params_host", "clip_tie", "gy_dev",
                                         "loss_dev", "partials_dev", "B", "D", "T", "stream"],
    }
    lib = _lib.load()
    for name, names in want.items():
        sig = _header_signature(name)
        assert [n for _, n in sig] == names
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and args == [_CTYPE[t] for t, _ in sig]
        assert hasattr(lib, name)
    assert lib.irbfn_abi_version() == 1
    # argument rules that need no GPU
    BAD, P = -1, C.c_void_p(8)
    d32 = np.asarray(DP, np.float32).ctypes.data_as(C.c_void_p)
    assert lib.irbfn_rollout_vjp_select(None, d32, None, None, 0, 5, 0.5, None) == 0              # B = 0
    assert lib.irbfn_rollout_vjp_select(None, d32, None, None, 4, 5, 0.5, None) == BAD
    assert lib.irbfn_rollout_vjp_select(P, None, P, P, 4, 5, 0.5, None) == BAD
    assert lib.irbfn_rollout_vjp_select(P, d32, P, P, -1, 5, 0.5, None) == BAD
    for mode, D, T in ((_lib.ROLLOUT_FULLINT, 7, 5), (_lib.ROLLOUT_ST_SELECT, 6, 5), (_lib.ROLLOUT_ST_KS, 7, 17),
                       (_lib.ROLLOUT_ST_SELECT, 7, 0)):
        assert lib.irbfn_train_seeds_st_fullint(mode, P, P, P, d32, 0.5, P, P, P, 4, D, T, None) == BAD
    assert lib.irbfn_train_seeds_st_fullint(_lib.ROLLOUT_ST_SELECT, P, P, P, None, 0.5, P, P, P, 4, 7, 5, None) == BAD


def test_vjp_instances_use_no_scratch():
    """The three ST_SELECT VJP instances as the build compiles them: no spilled VGPR, no scratch.  K4<ST_SELECT, 50> stays
    inside its registers only because the seed request computes its piece addresses in place (rollout_vjp.hip: `request`); a
    compiler that undoes that brings scratch traffic into the loop of pass 2, and this test says so."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import time_st_select_vjp as tool
    rows = tool.kernel_resources()
    assert sorted(r[0] for r in rows) == sorted(["rollout_vjp_regs_kernel<ST_SELECT, 8>", "rollout_vjp_regs_kernel<ST_SELECT, 50>",
                                                 "rollout_vjp_park_kernel<ST_SELECT>"])
    for label, vgpr, sgpr, spill, scratch in rows:
        assert spill == 0 and scratch == 0, (label, vgpr, spill, scratch)
