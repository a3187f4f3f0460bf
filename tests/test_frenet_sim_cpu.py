"""The Frenet frame of the closed-loop simulation without a GPU: Track's curvature and pose_at against the float64 statement
(tests/_frenet_sim_util.py), the statement against the oracle's two vehicle models (a sign or convention error that the
statement and the kernel would share shows here), the argument checks of the two entry points (decided before any HIP call)
and the error paths of irbfn_amd.simulate."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import _frenet_sim_util as fu
import _simulate_util as su
from irbfn_amd import _lib, configs, simulate
from irbfn_amd.model import WCRBFNet
from oracle import irbfn_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ------------------------------------------------------------------ curvature
@pytest.mark.parametrize("N,R", [(12, 5.0), (1000, 5.0), (257, 2.5)])
def test_curvature_of_a_regular_polygon(N, R):
    want = (np.pi / N) / (R * np.sin(np.pi / N))
    assert abs(want - 1.0 / R) <= (np.pi / N) ** 2 / 6.0 / R * 1.01
    for ccw, sign in ((True, 1.0), (False, -1.0)):
        wp = fu.ngon(N, R, ccw=ccw)
        k = simulate.Track(wp, wrap=True).curvature
        assert k.shape == (N,) and k.dtype == np.float64
        # float64 rounding of the inputs: a corner is rounded by R 2^-53 per coordinate, so a heading taken over a side of length
        # 2 pi R / N is off by up to 4 (R 2^-53) / (2 pi R / N) rad, and a difference of two of them, 4 pi / N rad, by the
        # relative 2^-52 N^2 / pi^2 (2.3e-11 at N = 1000); the lengths add N / pi times 2^-52
        rel = 2.0 ** -52 * N * N / np.pi ** 2 + 2.0 ** -52 * N
        assert np.max(np.abs(k - sign * want)) <= rel * want
        assert np.array_equal(k, fu.curvature(wp, True))
        # an open line through the same corners: the ends are one-sided, the interior is unchanged
        ko = simulate.Track(wp, wrap=False).curvature
        assert np.array_equal(ko[1:-1], k[1:-1]) and np.array_equal(ko, fu.curvature(wp, False))
        ln = np.hypot(*(wp[1, :2] - wp[0, :2]))
        assert abs(ko[0] - sign * (2 * np.pi / N) / ln) <= 2 * rel * abs(ko[0])
        assert abs(ko[-1] - sign * (2 * np.pi / N) / ln) <= 2 * rel * abs(ko[-1])


def test_curvature_of_a_straight_line_and_across_pi():
    for wrap in (False, True):
        assert np.array_equal(simulate.Track(su.straight_track(20), wrap=wrap).curvature[1:-1], np.zeros(18))
    assert np.array_equal(simulate.Track(su.straight_track(20), wrap=False).curvature, np.zeros(20))
    # a polygon started so that the heading column crosses +-pi in the middle of the line: no spike
    N, R = 64, 3.0
    wp = fu.ngon(N, R)
    th = wp[:, 2]
    assert np.any(np.abs(np.diff(th)) > 6.0)
    k = simulate.Track(wp, wrap=True).curvature
    assert np.max(np.abs(k - k[0])) <= 1e-12
    # the same headings written without the jump (theta + 2 pi behind it): the same curvature to rounding
    wp2 = wp.copy()
    wp2[:, 2] = np.unwrap(th)
    assert np.max(np.abs(simulate.Track(wp2, wrap=True).curvature - k)) <= 1e-12
    # two way-points: both ends one-sided
    two = simulate.Track(np.array([[0, 0, 0.25, 1.0], [2.0, 0, 0.75, 1.0]]), wrap=False).curvature
    assert np.array_equal(two, [0.25, 0.25])


def test_track_takes_a_curvature_of_its_own():
    wp = su.straight_track(10)
    k = np.linspace(-1, 1, 10)
    assert np.array_equal(simulate.Track(wp, curvature=k).curvature, k)
    assert np.array_equal(simulate.Track(wp, curvature=list(k.astype(np.float32))).curvature, k.astype(np.float32).astype(np.float64))
    for bad in (k[:9], k[None], 0.5, np.zeros((10, 1))):
        with pytest.raises(ValueError):
            simulate.Track(wp, curvature=bad)
    # a repeated way-point divides by zero at its neighbours: inf / NaN there, no warning turned error, no other entry touched
    wp2 = fu.ngon(12, 5.0)
    wp2[5] = wp2[4]
    k2 = simulate.Track(wp2, wrap=True).curvature
    assert np.isfinite(k2[[0, 1, 2, 8, 9, 10, 11]]).all() and k2.shape == (12,)


# ------------------------------------------------------------------ pose_at <-> the statement
def test_pose_at_is_the_inverse_of_the_statement():
    rng = np.random.default_rng(3)
    B = 50
    # a straight line along +x: (s, ey, epsi) come back up to float64 rounding and the float32 projection parameter in s
    wp = su.straight_track(60)
    tr = simulate.Track(wp, wrap=False)
    track, curv = fu.track_dict(wp, False), fu.curvature(wp, False)
    s, ey, epsi = rng.uniform(1.0, 28.0, B), rng.uniform(-0.6, 0.6, B), rng.uniform(-1.0, 1.0, B)
    ey[:3] = [0.0, 0.25, -0.25]
    s[0], epsi[0] = 3.25, 0.0                                    # a lattice point on the line: t = 0.5 and d = 0 exactly
    x, y, psi = tr.pose_at(s, ey, epsi)
    st = fu.ks_state(x, y, psi, 0.1, 3.0)
    # t is a float32 quotient, so the foot of the perpendicular is off by up to a = len 2^-22 along the line: s by a, and the
    # distance sqrt(ey^2 + a^2) by a^2 / (2 |ey|), or by a for a car on the line
    a = 0.5 * 2.0 ** -22
    for b in range(B):
        fr, i, d, t = fu.to_frenet(track, curv, st[b])
        assert abs(fr[0] - s[b]) <= a + 30.0 * 2.0 ** -52
        assert abs(fr[1] - ey[b]) <= min(a, a * a / (2 * abs(ey[b]) + 1e-300)) + 1e-15
        assert abs(fr[6] - epsi[b]) <= 1e-15 and fr[7] == 0.0
        assert fr[2] == 0.1 and fr[3] == 3.0 and fr[4] == 0.0 and fr[5] == 0.0
    assert fu.to_frenet(track, curv, st[0])[0][1] == 0.0 and not np.signbit(fu.to_frenet(track, curv, st[0])[0][1])
    # the N-gon, points whose projection falls into the interior of their segment (pose_at is not the inverse at a vertex)
    N, R = 200, 5.0
    wp = fu.ngon(N, R)
    tr = simulate.Track(wp, wrap=True)
    track, curv = fu.track_dict(wp, True), fu.curvature(wp, True)
    seg_len = tr.len[0]
    j = rng.integers(0, N - 1, B)
    s = tr.cum[j] + rng.uniform(0.3, 0.7, B) * seg_len
    ey, epsi = rng.uniform(-0.4, 0.4, B), rng.uniform(-0.4, 0.4, B)
    x, y, psi = tr.pose_at(s, ey, epsi)
    st = fu.ks_state(x, y, psi, 0.0, 3.0)
    a = seg_len * 2.0 ** -22
    for b in range(B):
        fr, i, d, t = fu.to_frenet(track, curv, st[b])
        assert i == j[b] and 0.0 < t < 1.0
        assert abs(fr[0] - s[b]) <= a + 35.0 * 2.0 ** -50
        # nearest_point rounds the segment vector to float32 (2^-24 of each component) before it places the foot along it
        assert abs(fr[1] - ey[b]) <= a * a / (2 * abs(ey[b])) + seg_len * 2.0 ** -23
        # the line's heading turns 2 pi / N over a segment, so an error a / seg_len in t turns it by 2^-22 * 2 pi / N
        assert abs(fr[6] - epsi[b]) <= 2.0 ** -22 * 2 * np.pi / N + 1e-14
        assert abs(fr[7] - curv[0]) <= 1e-12
    # pose_at clips s to the polyline and takes scalars
    x0, y0, p0 = tr.pose_at(-1.0)
    assert (float(x0), float(y0)) == (wp[0, 0], wp[0, 1]) and float(p0) == wp[0, 2]


# ------------------------------------------------------------------ frame <-> model
def _frame_model(kind, flip=1.0):
    """-> (frenet rows of the world-frame ST_KS Euler step, the oracle's Frenet step from the converted start, kappa v dt)"""
    wp, wrap, (s, ey, epsi), delta, u, p = fu.frame_model_case(kind)
    tr = simulate.Track(wp, wrap=wrap)
    track, curv = fu.track_dict(wp, wrap, window=(-1, -1)), fu.curvature(wp, wrap)
    x, y, psi = tr.pose_at(s, ey, epsi)
    st = fu.ks_state(x, y, psi, delta, 3.0)
    B = st.shape[0]
    fr0 = np.array([fu.to_frenet(track, curv, st[b])[0] for b in range(B)])
    # (a car seeded next to a vertex may be nearer to the neighbouring segment: ey differs by up to |ey| (1 - cos(2 pi / N)))
    assert np.max(np.abs(fr0[:, 1] - ey)) <= 1e-5 and np.max(np.abs(fr0[:, 6] - epsi)) <= 2 * np.pi / wp.shape[0] + 1e-12
    st1 = orc.dynamic_st_onestep_aux(np.concatenate([st, np.tile(u, (B, 1))], axis=1), p)
    fr1 = np.array([fu.to_frenet(track, curv, st1[b])[0] for b in range(B)])
    start = fr0.copy()
    start[:, 7] *= flip
    model = orc.dynamic_frenet_onestep(start, np.tile(u, (B, 1)), p)
    return fr1, model, float(np.max(np.abs(curv))) * 3.0 * p[8]


def test_statement_agrees_with_the_frenet_model_on_a_straight_line():
    fr1, model, _ = _frame_model("straight")
    # s carries the float32 projection parameter t (0.5 m segments: 0.5 * 2^-24 per conversion); the other seven are float64
    assert np.max(np.abs(fr1[:, 0] - model[:, 0])) <= 4 * 0.5 * 2.0 ** -24
    assert np.max(np.abs(fr1[:, 1:] - model[:, 1:])) <= 1e-13


def test_statement_agrees_with_the_frenet_model_on_the_1000_gon():
    """Figures of the statement alone (this test's inputs, no GPU): max |d epsi| 3.6e-4, max |d ey| 1.8e-5, inside half of each
    bound, so the device test keeps the same inputs."""
    fr1, model, kvdt = _frame_model("ngon")
    assert abs(kvdt - 6e-3) <= 1e-6
    d_epsi, d_ey = np.max(np.abs(fr1[:, 6] - model[:, 6])), np.max(np.abs(fr1[:, 1] - model[:, 1]))
    print(f"frame <-> model on the 1000-gon: max |d epsi| = {d_epsi:.3e}, max |d ey| = {d_ey:.3e}")
    assert d_epsi <= 0.25 * kvdt and d_ey <= 5e-4
    assert d_epsi <= 0.125 * kvdt and d_ey <= 2.5e-4            # half of each: room for the device's float32 plant
    assert np.max(np.abs(fr1[:, 2] - model[:, 2])) <= 1e-15 and np.max(np.abs(fr1[:, 3] - model[:, 3])) <= 1e-14
    # what the bound is for: the other sign of the curvature moves epsi by 2 kappa v dt
    _, flipped, _ = _frame_model("ngon", flip=-1.0)
    assert np.min(np.abs(fr1[:, 6] - flipped[:, 6])) > 4 * 0.25 * kvdt


# ------------------------------------------------------------------ argument checks
def _track_struct(**kw):
    d = dict(waypoints_dev=8, cum_dev=8, len_dev=8, length=10.0, lookahead=1.0, max_reacquire=2.0, half_width=0.0, N=5, wrap=1,
             win_back=8, win_fwd=55)
    d.update(kw)
    return _lib.SimTrack(**d)


BAD_TRACKS = [dict(N=1), dict(win_back=-1, win_fwd=5), dict(win_back=5, win_fwd=-1), dict(win_back=-2, win_fwd=-2),
              dict(lookahead=float("nan")), dict(max_reacquire=-1.0), dict(half_width=float("nan"))]


def test_sim_advance_frenet_rejects_bad_arguments_without_gpu():
    lib = _lib.load()
    sel = _lib.ROLLOUT_ST_SELECT
    p = (C.c_float * 13)()

    def call(tr, curv=8, mode=sel, controls=None, T=0, host=None, dev=None, n_sub=1, B=4, ptrs=(8,) * 6):
        st, sg, ss, rc, x, m = ptrs
        return lib.irbfn_sim_advance_frenet(C.byref(tr) if tr is not None else None, curv, mode, 0, controls, T, host, dev, n_sub,
                                            st, sg, ss, rc, x, m, None, None, None, None, B, None)
    ok = _track_struct()
    assert call(None) == -1
    assert call(ok, B=-1) == -1
    assert call(ok, n_sub=0) == -1
    for kw in BAD_TRACKS:
        assert call(_track_struct(**kw)) == -1, kw
        assert call(_track_struct(**kw), B=0) == -1, kw                  # the scalars are checked whatever B
    assert call(ok, controls=8, T=0, host=p) == -1                       # controls with T < 1
    for mode in (_lib.ROLLOUT_FULLINT, _lib.ROLLOUT_FRENET_LS, _lib.ROLLOUT_SPIRAL, 99, -1):
        assert call(ok, mode=mode) == -1
    assert call(ok, controls=8, T=5) == -1                               # a plant step without parameters
    assert call(ok, curv=None) == -1                                     # no curvature
    for k in range(6):                                                   # each required per-car pointer
        assert call(ok, ptrs=tuple(None if j == k else 8 for j in range(6))) == -1
    for name in ("waypoints_dev", "cum_dev", "len_dev"):
        assert call(_track_struct(**{name: None})) == -1
    assert call(ok, B=0, curv=None, ptrs=(None,) * 6) == 0               # B = 0 is a no-op whatever the pointers
    assert call(_track_struct(win_back=-1, win_fwd=-1), mode=_lib.ROLLOUT_ST_KS, B=0) == 0


def test_cartesian_to_frenet_rejects_bad_arguments_without_gpu():
    lib = _lib.load()

    def call(tr, curv=8, state=8, seg=None, frenet=8, B=4):
        return lib.irbfn_cartesian_to_frenet(C.byref(tr) if tr is not None else None, curv, state, seg, frenet, None, None, None,
                                             B, None)
    ok = _track_struct()
    assert call(None) == -1
    assert call(ok, B=-1) == -1
    for kw in BAD_TRACKS:
        assert call(_track_struct(**kw)) == -1, kw
        assert call(_track_struct(**kw), B=0) == -1, kw
    assert call(ok, curv=None) == -1 and call(ok, state=None) == -1 and call(ok, frenet=None) == -1
    for name in ("waypoints_dev", "cum_dev", "len_dev"):
        assert call(_track_struct(**{name: None})) == -1
    assert call(ok, B=0, curv=None, state=None, frenet=None) == 0


def test_simulate_frenet_shape_and_type_errors():
    wp = su.straight_track(10)
    tr = simulate.Track(wp, wrap=False, lookahead=1.0, max_reacquire=3.0)
    net7 = WCRBFNet.from_config(dict(configs.model_card(2), num_kernels=16, out_features=10))
    card8 = json.load(open(os.path.join(GOLDEN, "ckpt_dnmpc_12regions_frenet_l1_bigdata.json")))
    net8 = WCRBFNet.from_config(card8)
    odd8 = WCRBFNet.from_config(dict(card8, out_features=5))
    assert net8.in_features == 8 and net8.out_features == 2 and odd8.out_features == 5
    s0 = np.zeros((3, 7), np.float32)
    with pytest.raises(TypeError):
        simulate.closed_loop_frenet(object(), {}, tr, s0, 2, dyn_params=su.DYN)
    with pytest.raises(TypeError):
        simulate.closed_loop_frenet(net8, {}, wp, s0, 2, dyn_params=su.DYN)
    with pytest.raises(ValueError, match="8 inputs"):
        simulate.closed_loop_frenet(net7, {}, tr, s0, 2, dyn_params=su.DYN)
    with pytest.raises(ValueError, match="8 inputs and 2T outputs"):
        simulate.closed_loop_frenet(odd8, {}, tr, s0, 2, dyn_params=su.DYN)
    with pytest.raises(ValueError, match="7 inputs"):                     # and the Cartesian loop still refuses the Frenet net
        simulate.closed_loop(net8, {}, tr, s0, 2, dyn_params=su.DYN)
    with pytest.raises(ValueError, match="state0"):
        simulate.closed_loop_frenet(net8, {}, tr, np.zeros((3, 8), np.float32), 2, dyn_params=su.DYN)
    with pytest.raises(ValueError, match="plant_params"):
        simulate.closed_loop_frenet(net8, {}, tr, s0, 2, dyn_params=su.DYN, plant_params=np.zeros((2, 13)))
    with pytest.raises(ValueError):
        simulate.closed_loop_frenet(net8, {}, tr, s0, 2)
    with pytest.raises(ValueError):
        simulate.closed_loop_frenet(net8, {}, tr, s0, 2, dyn_params=su.DYN, n_sub=0)
    with pytest.raises(ValueError):
        simulate.closed_loop_frenet(net8, {}, tr, s0, 2, dyn_params=su.DYN, mode=_lib.ROLLOUT_FRENET_LS)
    with pytest.raises(TypeError):
        simulate.advance_frenet(wp, None, None, None, None, None, None)
    with pytest.raises(TypeError):
        simulate.to_frenet(wp, s0)
    with pytest.raises(ValueError):
        simulate.to_frenet(tr, np.zeros((3, 8), np.float32))
    with pytest.raises(ValueError):
        simulate.to_frenet(tr, s0, seg=np.zeros(4, np.int32))
