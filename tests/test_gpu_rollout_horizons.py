"""Roll-out kernels at every dispatch boundary and past T = 50 (run on the MI355X box with ``-m gpu``).

launch_mode (irbfn_amd/csrc/rollout.hip) picks the forward kernel by horizon: rollout_fwd_regs_kernel<M, 8> for T <= 8,
rollout_fwd_pair_kernel for 9 <= T <= 50 (the control modes), rollout_fwd_regs_kernel<SPIRAL, 50> for a spiral of
9 <= N <= 50, rollout_fwd_lean_kernel beyond.  launch_rollout_vjp (rollout_vjp.hip) takes rollout_vjp_regs_kernel<M, 8 / 50>
up to T = 50, rollout_vjp_park_kernel up to T = 200 (Frenet: 150) and rollout_vjp_spiral_staged up to N = 256.  Here every
kernel meets the float64 oracle at the horizons around its boundaries (T mod 4 tails, masked register slots, partial
8-sample groups), at batches of one row, of whole 64-row waves and of a ragged last wave, with misaligned buffers and in
the split state / control layout of the planning tick.  A row's result does not depend on the batch it is launched in, its
alignment or the layout: those are compared bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from _rollout_util import assert_states_close, frenet_inputs_long, spiral_inputs, st_inputs
from irbfn_amd import _lib, configs
from irbfn_amd import dynamics as dyn
from irbfn_amd.model import WCRBFNet, _stream_ptr
from irbfn_amd.planner import plan_batch, plan_tick
from oracle import c_oracle as co
from oracle import hand_vjp as hv
from oracle import irbfn_oracle as orc

pytestmark = pytest.mark.gpu
DP = np.array(configs.DYN_PARAMS)
DP32 = DP.astype(np.float32)
SELECT, KS, FULLINT, FRENET, SPIRAL = (_lib.ROLLOUT_ST_SELECT, _lib.ROLLOUT_ST_KS, _lib.ROLLOUT_FULLINT,
                                       _lib.ROLLOUT_FRENET_LS, _lib.ROLLOUT_SPIRAL)
CONTROL_MODES = [SELECT, KS, FULLINT, FRENET]
STATE_DIM = {SELECT: 7, KS: 7, FULLINT: 5, FRENET: 8, SPIRAL: 6}
BATCHES = (1, 64, 65, 128, 129, 1000)      # one row; whole waves; a ragged last wave after full ones
NMAX = max(BATCHES)


def _rows(mode, B, T, seed):
    """Input rows (float32 values, float64 array) of a mode: [state, a_0.., sv_0..], FULLINT [v0, u], spiral [k0..k3, s]."""
    if mode in (SELECT, KS):
        x = st_inputs(B, T, seed)
    elif mode == FULLINT:
        rng = np.random.default_rng(seed)
        x = np.hstack([rng.uniform(-1, 8, (B, 1)), rng.normal(size=(B, T)) * 5, rng.normal(size=(B, T)) * 2])
    elif mode == FRENET:
        x = frenet_inputs_long(B, T, seed, DP)
    else:
        x = spiral_inputs(B, seed)
    return x.astype(np.float32).astype(np.float64)


def _oracle(mode, x, T):
    """(float64 NumPy oracle, float32 C oracle) states [B, T, S] of rows x."""
    x32 = x.astype(np.float32)
    if mode == SELECT:
        return orc.integrate_st_mult(x, DP), co.integrate_st_mult(x32, DP32, T, np.float32)
    if mode == KS:
        return orc.integrate_st_ks_mult(x, DP), co.integrate_st_mult(x32, DP32, T, np.float32, True)
    if mode == FULLINT:
        return orc.rollout_fullint(x[:, 0], x[:, 1:]), co.rollout_fullint(x32[:, 0], x32[:, 1:], T, np.float32)
    if mode == FRENET:
        ref = orc.integrate_frenet_mult(x, DP)
        assert np.abs(ref[:, :, 1] * ref[:, :, 7]).max() < 0.5          # away from the pole of 1/(1 - ey*cur)
        return ref, co.integrate_frenet_mult(x32, DP32, T, np.float32)
    return orc.integrate_path_mult(x, T), co.integrate_path_mult(x32, T, np.float32)


def _params(mode):
    return None if mode in (FULLINT, SPIRAL) else DP


def _forward_raw(mode, xd, T, out_off=0):
    """irbfn_rollout_forward on device rows xd with the states written `out_off` floats into a NaN-filled buffer; the
    floats around the [B, T, S] block must stay NaN."""
    lib = _lib.load()
    B, S = xd.shape[0], STATE_DIM[mode]
    n = B * T * S
    big = torch.full((out_off + n + 8,), float("nan"), dtype=torch.float32, device="cuda")
    keep, pp = dyn._dyn(_params(mode))
    st = lib.irbfn_rollout_forward(mode, C.c_void_p(xd.data_ptr()), pp, C.c_void_p(big.data_ptr() + 4 * out_off), B, T,
                                   _stream_ptr(torch))
    _lib.check(st, "irbfn_rollout_forward")
    guard = torch.cat([big[:out_off], big[out_off + n:]])
    assert torch.isnan(guard).all(), "store outside the states block"
    return big[out_off:out_off + n].view(B, T, S).cpu().numpy()


def _vjp_raw(mode, xd, gd, T, out_off=0, fill=float("nan")):
    """irbfn_rollout_vjp -> (status, cotangent buffer [out_off + B*L + 8] as numpy)."""
    lib = _lib.load()
    B, L = xd.shape[0], xd.shape[1]
    big = torch.full((out_off + B * L + 8,), fill, dtype=torch.float32, device="cuda")
    keep, pp = dyn._dyn(_params(mode))
    st = lib.irbfn_rollout_vjp(mode, C.c_void_p(xd.data_ptr()), pp, C.c_void_p(gd.data_ptr()),
                               C.c_void_p(big.data_ptr() + 4 * out_off), B, T, 0.5, _stream_ptr(torch))
    torch.cuda.synchronize()
    return st, big.cpu().numpy()


def _view(a, off):
    """A contiguous device copy of `a` whose base sits `off` floats past a 256-byte aligned allocation."""
    a = np.ascontiguousarray(a, np.float32)
    big = torch.zeros(off + a.size, dtype=torch.float32, device="cuda")
    v = big[off:off + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == (4 * off) % 16 and v.is_contiguous()
    return v


# ------------------------------------------------------------------ forward: horizons x batches
FWD_T = [8, 9, 49, 51, 52, 53, 54, 64, 100, 300]         # regs<8> | pair | lean, tails T mod 4 = 3, 0, 1, 2
SPIRAL_N = [1, 2, 8, 9, 50, 51, 100, 256, 300]          # regs<8> | regs<50> | lean


def _spiral_floor(q):
    """Per row: the magnitude of the terms the spiral's heading and curvature sum, sum_j |c_j| (s^(j+1) / (j+1) + s^j)
    (planner_utils.py:32-41).  They cancel to results far smaller than themselves (N = 2: the end point is one such sum),
    and float32 gets a sum right to a few ulp of its terms, not of its value: the kernel (reciprocals of j + 1) and the
    float32 restatement (divisions) round differently.  0.02 of it in the scale = 2e-7 of it at rtol 1e-5."""
    c, s = orc.params_to_coefs(q), q[:, 4]
    m = sum(np.abs(c[:, j]) * (s ** (j + 1) / (j + 1) + s ** j) for j in range(4))
    return np.maximum(0.02 * m, 1e-3)[:, None, None]


def _assert_forward_close(mode, got, x, T):
    ref, ref32 = _oracle(mode, x, T)
    if mode == SPIRAL:
        assert_states_close(got, ref, ref32, floor=_spiral_floor(x))
    else:
        # past T = 50 a row's float32 error is a random walk over more steps, and the kernels' polynomial sine / cosine and
        # reciprocal divisions (<= 2 ulp) walk differently from libm's: at T = 52 one of 364000 elements lands 1 % beyond 4x
        assert_states_close(got, ref, ref32, k32=4.0 if T <= 50 else 8.0)


def _check_forward(mode, T, seed):
    x = _rows(mode, NMAX, T, seed)
    xd = torch.from_numpy(x.astype(np.float32)).cuda()
    full = dyn.rollout_forward(mode, xd, _params(mode), T).cpu().numpy()
    _assert_forward_close(mode, full, x, T)
    for B in BATCHES[:-1]:
        got = dyn.rollout_forward(mode, xd[:B].contiguous(), _params(mode), T).cpu().numpy()
        np.testing.assert_array_equal(got, full[:B])          # a row's states do not depend on the launch's batch


@pytest.mark.parametrize("T", FWD_T)
@pytest.mark.parametrize("mode", CONTROL_MODES, ids=["select", "ks", "fullint", "frenet"])
def test_forward_horizons_and_batches(gpu, mode, T):
    _check_forward(mode, T, seed=1000 * mode + T)


@pytest.mark.parametrize("N", SPIRAL_N)
def test_spiral_forward_horizons_and_batches(gpu, N):
    _check_forward(SPIRAL, N, seed=N)


@pytest.mark.parametrize("N", [1, 2, 9, 100])
def test_spiral_samples_follow_linspace(gpu, N):
    """x_i = sk_i * dx_i, sk = jnp.linspace(0, s, N): for N = 1 the only sample sits at 0."""
    q = spiral_inputs(65, seed=N).astype(np.float32)
    st = dyn.rollout_forward(SPIRAL, q, None, N).astype(np.float64)
    sk = np.stack([np.linspace(0.0, s, N) for s in q[:, 4].astype(np.float64)])
    np.testing.assert_allclose(st[:, :, 0], sk * st[:, :, 4], rtol=1e-6, atol=1e-6)
    if N == 1:
        np.testing.assert_array_equal(st[:, 0, [0, 1, 2, 5]], 0.0)
        np.testing.assert_array_equal(st[:, 0, 4], 1.0)
        np.testing.assert_array_equal(st[:, 0, 3], q[:, 0])


@pytest.mark.parametrize("N", [100, 256])
def test_spiral_straight_line(gpu, N):
    s = np.array([0.5, 3.0, 7.5, 10.0])
    q = np.hstack([np.zeros((4, 4)), s[:, None]]).astype(np.float32)
    st = dyn.rollout_forward(SPIRAL, q, None, N)
    np.testing.assert_allclose(st[:, -1, :3], np.stack([s, 0 * s, 0 * s], -1), rtol=0, atol=2e-5 * s.max())
    np.testing.assert_allclose(st[:, :, 0], np.stack([np.linspace(0, v, N) for v in s]), rtol=0, atol=2e-5 * s.max())


# ------------------------------------------------------------------ forward: misaligned inputs and outputs
@pytest.mark.parametrize("T", [9, 33, 50, 53, 64])
@pytest.mark.parametrize("mode", CONTROL_MODES, ids=["select", "ks", "fullint", "frenet"])
def test_forward_misaligned_buffers(gpu, mode, T):
    """Input views 1-3 floats past an aligned base (the lean kernel's aligned-superset control fetch, the DMA
    prologues' fallback) and outputs 1-3 floats past one (every row's carry / line head moves): bit for bit the aligned
    result, and the floats around the states block untouched."""
    B = 129
    x = _rows(mode, B, T, seed=T + 7 * mode)
    aligned = _forward_raw(mode, _view(x, 0), T)
    _assert_forward_close(mode, aligned, x, T)
    for in_off, out_off in ((1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3), (3, 1), (1, 3)):
        got = _forward_raw(mode, _view(x, in_off), T, out_off)
        np.testing.assert_array_equal(got, aligned, err_msg=f"in_off={in_off} out_off={out_off}")


@pytest.mark.parametrize("N", [9, 53, 64])
def test_spiral_forward_misaligned_buffers(gpu, N):
    q = spiral_inputs(129, seed=N).astype(np.float32)
    aligned = _forward_raw(SPIRAL, _view(q, 0), N)
    for in_off, out_off in ((1, 0), (0, 1), (2, 3), (3, 2)):
        np.testing.assert_array_equal(_forward_raw(SPIRAL, _view(q, in_off), N, out_off), aligned)


# ------------------------------------------------------------------ split layout past T = 50
def _tick_net(T, seed):
    cfg = dict(configs.model_card(2), out_features=2 * T, num_kernels=512)
    rng = np.random.default_rng(seed)
    P = {"params": {"rbf_list": {"centers": rng.uniform(-1, 8, size=(1, 512, 7)).astype(np.float32),
                                 "log_sigs": rng.uniform(0, 2, size=(1, 512)).astype(np.float32)},
                    "linear": {"kernel": (rng.normal(size=(512, 2 * T)) * 0.1).astype(np.float32),
                               "bias": np.zeros(2 * T, np.float32)}}}
    return WCRBFNet.from_config(cfg), P


def _np(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


@pytest.mark.parametrize("T", [53, 64])
@pytest.mark.parametrize("mode", [SELECT, KS], ids=["select", "ks"])
def test_split_layout_tick_past_50(gpu, mode, T):
    """plan_tick (mirror flags) and plan_batch roll out [state0] + [controls] from two buffers (LU = 2T): the states are
    those of the combined-layout roll-out of [state0, returned controls], bit for bit, and meet the float64 oracle."""
    net, P = _tick_net(T, seed=T)
    B = 777
    x = configs.synth_queries(2, B=B)
    st0 = configs.initial_state_from_query(x)
    mirror = (np.arange(B) % 3 == 1).astype(np.int32)
    fn = dyn.integrate_st_mult if mode == SELECT else dyn.integrate_st_ks_mult
    ref_fn = orc.integrate_st_mult if mode == SELECT else orc.integrate_st_ks_mult
    for ctrl, states in (plan_tick(net, P, x, mirror, st0, DP, mode=mode), plan_batch(net, P, x, st0, DP, mode=mode)):
        ctrl, states = _np(ctrl), _np(states)
        xu = np.hstack([st0, ctrl]).astype(np.float32)
        np.testing.assert_array_equal(states, fn(xu, DP))
        sub = np.arange(0, B, 7)
        assert_states_close(states[sub], ref_fn(xu[sub].astype(np.float64), DP),
                            co.integrate_st_mult(xu[sub], DP32, T, np.float32, mode == KS))
    u_m, _ = plan_tick(net, P, x, mirror, st0, DP, mode=mode)
    u_0, _ = plan_tick(net, P, x, None, st0, DP, mode=mode)
    u_m, u_0 = _np(u_m), _np(u_0)
    m = mirror == 1
    np.testing.assert_array_equal(u_m[~m], u_0[~m])
    np.testing.assert_array_equal(u_m[m][:, :T], u_0[m][:, :T])
    np.testing.assert_array_equal(u_m[m][:, T:], -u_0[m][:, T:])           # mirrored rows: steering velocity flipped


# ------------------------------------------------------------------ VJPs
def _autograd32(mode, x, gs, T):
    """Cotangent of the rows from float32 torch.autograd of the oracle restatement."""
    t = torch.tensor(x, dtype=torch.float32, requires_grad=True)
    d = torch.tensor(DP32)
    if mode == KS:
        st = orc.integrate_st_ks_mult(t, d)
    elif mode == FULLINT:
        st = orc.rollout_fullint(t[:, 0], t[:, 1:])
    elif mode == FRENET:
        st = orc.integrate_frenet_mult(t, d)
    else:
        st = orc.integrate_path_mult(t, T)
    (st * torch.tensor(gs, dtype=torch.float32)).sum().backward()
    return t.grad.numpy().astype(np.float64)


def _hand(mode, x, gs, T):
    if mode == KS:
        return hv.vjp_st_ks(x, DP, gs)
    if mode == FULLINT:
        gv, gu = hv.vjp_fullint(x[:, 0], x[:, 1:], gs)
        return np.hstack([gv[:, None], gu])
    if mode == FRENET:
        return hv.vjp_frenet(x, DP, gs)
    return hv.vjp_spiral(x, gs, N=T)


def assert_grads_close(got, ref, ref32=None):
    """Input-row cotangents against the float64 hand adjoint.  Per row: pass if |err| <= 5e-5 * rowmax + 1e-6 (rowmax = the
    row's largest |ref|) -- or, where float32 itself is worse conditioned over a long horizon, if the error is within 4x
    the error float32 torch.autograd of the oracle restatement makes on that row (mirrors assert_states_close)."""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape
    rowmax = np.abs(ref).max(axis=1, keepdims=True)
    err = np.abs(got - ref)
    bound = 5e-5 * rowmax + 1e-6
    if ref32 is not None:
        bound = np.maximum(bound, 4.0 * np.abs(ref32 - ref).max(axis=1, keepdims=True))
    bad = err > bound
    assert not bad.any(), (int(bad.sum()), float(err.max()), float((err / (rowmax + 1e-30)).max()))


VJP_B = (1, 65, 257)


def _check_vjp(mode, T, seed):
    S = STATE_DIM[mode]
    x = _rows(mode, VJP_B[-1], T, seed)
    gs = np.random.default_rng(seed + 1).normal(size=(x.shape[0], T, S)).astype(np.float32).astype(np.float64)
    ref = _hand(mode, x, gs, T)
    xd, gd = torch.from_numpy(x.astype(np.float32)).cuda(), torch.from_numpy(gs.astype(np.float32)).cuda()
    full = dyn.rollout_vjp(mode, xd, _params(mode), gd, T).cpu().numpy()
    np.testing.assert_array_equal(dyn.rollout_vjp(mode, xd, _params(mode), gd, T).cpu().numpy(), full)   # deterministic
    assert_grads_close(full, ref, _autograd32(mode, x, gs, T))
    for B in VJP_B[:-1]:
        got = dyn.rollout_vjp(mode, xd[:B].contiguous(), _params(mode), gd[:B].contiguous(), T).cpu().numpy()
        np.testing.assert_array_equal(got, full[:B])


VJP_T = [8, 9, 33, 49, 51, 64, 100]


@pytest.mark.parametrize("T", VJP_T + [200])
@pytest.mark.parametrize("mode", [KS, FULLINT], ids=["ks", "fullint"])
def test_vjp_horizons(gpu, mode, T):
    _check_vjp(mode, T, seed=100 * mode + T)


@pytest.mark.parametrize("T", VJP_T + [150])
def test_frenet_vjp_horizons(gpu, T):
    _check_vjp(FRENET, T, seed=T)


@pytest.mark.parametrize("N", [1, 2, 8, 9, 16, 17, 255, 256])
def test_spiral_vjp_horizons(gpu, N):
    _check_vjp(SPIRAL, N, seed=N)


@pytest.mark.parametrize("T", [9, 33, 50, 53, 64])
@pytest.mark.parametrize("mode", [KS, FULLINT, FRENET], ids=["ks", "fullint", "frenet"])
def test_vjp_misaligned_buffers(gpu, mode, T):
    """Rows, seeds and the cotangent output 1-3 floats off 16-byte alignment: K4 leaves its LDS-DMA paths (dma_ok = 0)
    for per-lane loads and stores, the park kernel reads the same rows through other addresses.  Bit for bit the
    aligned result; nothing written outside the cotangent block."""
    B, S = 129, STATE_DIM[mode]
    x = _rows(mode, B, T, seed=T + mode)
    gs = np.random.default_rng(T).normal(size=(B, T, S)).astype(np.float32).astype(np.float64)
    L = x.shape[1]
    st, buf = _vjp_raw(mode, _view(x, 0), _view(gs, 0), T)
    assert st == 0
    aligned = buf[:B * L].reshape(B, L)
    assert np.isnan(buf[B * L:]).all()
    assert_grads_close(aligned, _hand(mode, x, gs, T), _autograd32(mode, x, gs, T))
    for xo, go, oo in ((1, 0, 0), (0, 2, 0), (0, 0, 3), (3, 1, 2), (2, 3, 1)):
        st, buf = _vjp_raw(mode, _view(x, xo), _view(gs, go), T, out_off=oo)
        assert st == 0
        assert np.isnan(buf[:oo]).all() and np.isnan(buf[oo + B * L:]).all()
        np.testing.assert_array_equal(buf[oo:oo + B * L].reshape(B, L), aligned, err_msg=f"offsets {xo} {go} {oo}")


# ------------------------------------------------------------------ limits
@pytest.mark.parametrize("mode,T", [(KS, 201), (FULLINT, 201), (FRENET, 151), (SPIRAL, 257)],
                         ids=["ks", "fullint", "frenet", "spiral"])
def test_vjp_beyond_limits_is_refused(gpu, mode, T):
    """One past the largest horizon (T = 200 / 150, N = 256 run in the tests above): UNSUPPORTED -> ValueError, and no
    kernel touches the output."""
    B, S = 65, STATE_DIM[mode]
    x = spiral_inputs(B, seed=1) if mode == SPIRAL else np.zeros((B, (1 if mode == FULLINT else S) + 2 * T))
    xd = torch.from_numpy(x.astype(np.float32)).cuda()
    gd = torch.ones((B, T, S), dtype=torch.float32, device="cuda")
    st, buf = _vjp_raw(mode, xd, gd, T, fill=-7.0)
    assert st == -2 and (buf == -7.0).all()      # IRBFN_ERR_UNSUPPORTED, output untouched
    with pytest.raises(ValueError):
        dyn.rollout_vjp(mode, xd, _params(mode), gd, T)


def test_st_select_vjp_stays_refused(gpu):
    for T in (5, 64):
        with pytest.raises(ValueError):
            dyn.rollout_vjp(SELECT, np.zeros((4, 7 + 2 * T), np.float32), DP, np.zeros((4, T, 7), np.float32), T)
