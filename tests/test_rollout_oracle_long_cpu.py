"""CPU checks of the roll-out references at the horizons the GPU tests use beyond the reference's T = 5 / 50: the hand
adjoints (oracle/hand_vjp.py) against torch.autograd of the float64 restatement, the C restatement against the NumPy one,
and the spiral's samples against jnp.linspace(0, s, N), N = 1 included.  No GPU."""
import numpy as np
import pytest
import torch

from _rollout_util import frenet_inputs_long, spiral_inputs, st_inputs
from irbfn_amd import configs
from oracle import c_oracle as co
from oracle import hand_vjp as hv
from oracle import irbfn_oracle as orc

DP = np.array(configs.DYN_PARAMS)


def _autograd(fn, x, g):
    t = torch.tensor(x, requires_grad=True)
    (fn(t) * torch.tensor(g)).sum().backward()
    return t.grad.numpy()


def _close(hand, ref, rtol=1e-9):
    """Row by row, relative to the row's largest cotangent."""
    rowmax = np.abs(ref).max(axis=1, keepdims=True)
    assert (np.abs(hand - ref) <= rtol * rowmax + 1e-12).all(), float((np.abs(hand - ref) / (rowmax + 1e-300)).max())


@pytest.mark.parametrize("mode,T", [("st_ks", 64), ("st_ks", 200), ("fullint", 64), ("fullint", 200), ("frenet", 150)])
def test_hand_rollout_vjps_match_autograd_long(mode, T):
    B = 6
    rng = np.random.default_rng(T)
    if mode == "st_ks":
        xu = st_inputs(B, T, seed=T)
        gs = rng.normal(size=(B, T, 7))
        _close(hv.vjp_st_ks(xu, DP, gs), _autograd(lambda a: orc.integrate_st_ks_mult(a, DP), xu, gs))
    elif mode == "fullint":
        v0, u = rng.uniform(-1, 8, B), np.hstack([rng.normal(size=(B, T)) * 5, rng.normal(size=(B, T)) * 2])
        gs = rng.normal(size=(B, T, 5))
        gv, gu = hv.vjp_fullint(v0, u, gs)
        x = np.hstack([v0[:, None], u])
        ref = _autograd(lambda a: orc.rollout_fullint(a[:, 0], a[:, 1:]), x, gs)
        _close(np.hstack([gv[:, None], gu]), ref)
    else:
        xf = frenet_inputs_long(B, T, seed=T, dp=DP)
        gs = rng.normal(size=(B, T, 8))
        _close(hv.vjp_frenet(xf, DP, gs), _autograd(lambda a: orc.integrate_frenet_mult(a, DP), xf, gs))


@pytest.mark.parametrize("N", [1, 2, 17, 256])
def test_hand_spiral_vjp_matches_autograd(N):
    q = spiral_inputs(8, seed=N)
    gs = np.random.default_rng(N).normal(size=(8, N, 6))
    _close(hv.vjp_spiral(q, gs, N=N), _autograd(lambda a: orc.integrate_path_mult(a, N), q, gs))


@pytest.mark.parametrize("N", [1, 2, 3, 9, 100])
def test_spiral_samples_follow_linspace(N):
    """x_i = sk_i * dx_i with sk = jnp.linspace(0, s, N) (planner_utils.py:55,71): for N = 1 the only sample is at 0."""
    q = spiral_inputs(16, seed=N)
    sk = np.stack([np.linspace(0.0, s, N) for s in q[:, 4]])
    for st in (orc.integrate_path_mult(q, N), co.integrate_path_mult(q, N, np.float64)):
        np.testing.assert_allclose(st[:, :, 0], sk * st[:, :, 4], rtol=1e-14, atol=1e-14)
        np.testing.assert_allclose(st[:, :, 1], sk * st[:, :, 5], rtol=1e-14, atol=1e-14)
    if N == 1:
        # one sample at s = 0: heading 0, curvature k0, (dx, dy) = (1, 0)
        st = orc.integrate_path_mult(q, 1)
        exp = np.stack([0 * q[:, 0], 0 * q[:, 0], 0 * q[:, 0], q[:, 0], 1 + 0 * q[:, 0], 0 * q[:, 0]], -1)
        np.testing.assert_array_equal(st[:, 0], exp)
        g = hv.vjp_spiral(q, np.ones((16, 1, 6)), N=1)
        np.testing.assert_array_equal(g, np.hstack([np.ones((16, 1)), np.zeros((16, 4))]))   # only kappa = k0 depends on q


def test_c_oracle_matches_numpy_at_t100():
    """The GPU horizon tests take the C restatement's float32 run as the float32 yardstick at long T: it must compute what
    the NumPy restatement computes (float64, T = 100, every mode; the spiral at N = 1, 100, 256)."""
    T, B = 100, 40
    rng = np.random.default_rng(100)
    xu = st_inputs(B, T, seed=1)

    def near(a, b):
        scale = np.maximum(np.abs(b).max(axis=1, keepdims=True), 1.0)
        assert (np.abs(a - b) <= 1e-11 * scale).all(), float((np.abs(a - b) / scale).max())

    near(co.integrate_st_mult(xu, DP, T, np.float64), orc.integrate_st_mult(xu, DP))
    near(co.integrate_st_mult(xu, DP, T, np.float64, True), orc.integrate_st_ks_mult(xu, DP))
    xf = frenet_inputs_long(B, T, seed=2, dp=DP)
    near(co.integrate_frenet_mult(xf, DP, T, np.float64), orc.integrate_frenet_mult(xf, DP))
    v0, u = rng.uniform(-1, 8, B), rng.normal(size=(B, 2 * T)) * 3
    near(co.rollout_fullint(v0, u, T, np.float64), orc.rollout_fullint(v0, u))
    q = spiral_inputs(B, seed=3)
    for N in (1, 100, 256):
        near(co.integrate_path_mult(q, N, np.float64), orc.integrate_path_mult(q, N))
