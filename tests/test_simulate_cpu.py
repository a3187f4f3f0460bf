"""Closed-loop simulation without a GPU: the float64 statement of a tick on lattice data, the window enumeration, the argument
checks of irbfn_sim_advance (decided before any HIP call) and the error paths of irbfn_amd.simulate."""
import ctypes as C

import numpy as np
import pytest

import _simulate_util as su
from irbfn_amd import _lib, configs, simulate
from irbfn_amd.model import WCRBFNet


def test_statement_on_a_straight_lattice_track():
    """A car on a straight lattice line at lattice speed and dt (kinematic branch: v < 3, no steering): the goal is the way-point
    behind the first crossing of the look-ahead circle, and progress after n ticks is exactly n v dt."""
    wp = su.straight_track(40, step=0.5, v=2.0)
    track = dict(wp=wp, wrap=False, lookahead=1.25, max_reacquire=5.0, half_width=0.0, window=(8, 55))
    p = su.DYN.copy()
    p[8] = 0.125                                   # dt
    state = np.array([1.25, 2.0, 0.0, 2.0, 0.0, 0.0, 0.0])
    rec = su.new_record()
    r = su.tick(track, state, 0, rec)
    assert r["status"] == su.OK and r["seg"] == 0 and r["d"] == 0.0 and r["t"] == 0.5
    # the circle of radius 1.25 about x = 1.25 crosses the line at x = 2.5 = way-point 3, i.e. at the end of segment 2
    assert np.array_equal(r["goal"], wp[2]) and not r["mirror"]
    assert rec["ticks"] == 1.0 and rec["progress"] == 0.0 and rec["s_last"] == 0.25
    n = 6
    for k in range(n):
        r = su.tick(track, r["state"], r["seg"], rec, controls=(0.0, 0.0), params=p, n_sub=1, tick_no=k + 1)
        assert r["status"] == su.OK
    assert rec["progress"] == n * 2.0 * 0.125 and rec["ticks"] == n + 1.0
    assert r["state"][0] == 1.25 + n * 0.25 and rec["sum_d2"] == 0.0 and rec["sum_dv"] == 0.0 and rec["fail_tick"] == -1.0
    # two half steps cover the same ground
    rec2 = su.new_record()
    r2 = su.tick(track, state, 0, rec2)
    r2 = su.tick(track, r2["state"], r2["seg"], rec2, controls=(0.0, 0.0), params=p, n_sub=2, tick_no=1)
    assert rec2["progress"] == 0.25 and r2["state"][0] == 1.5


def test_statement_stops_a_car():
    wp = su.straight_track(10)
    track = dict(wp=wp, wrap=False, lookahead=1.0, max_reacquire=3.0, half_width=0.0, window=(-1, -1))
    far = su.tick(track, np.array([3.0, 8.0, 0, 1.0, 0, 0, 0]), 0, su.new_record(), tick_no=4)
    assert far["status"] == su.LOST and far["rec"]["fail_tick"] == 4.0 and "x" not in far
    end = su.tick(track, np.array([5.5, 2.0, 0, 1.0, 0, 0, 0]), 0, su.new_record())     # the last way-point: nothing ahead
    assert end["status"] == su.LOST
    near = su.tick(track, np.array([3.0, 4.0, 0, 1.0, 0, 0, 0]), 0, su.new_record())    # beyond lookahead, within reacquire
    assert near["status"] == su.OK and np.array_equal(near["goal"], wp[near["seg"]])
    off = su.tick(dict(track, half_width=0.5), np.array([3.0, 2.75, 0, 1.0, 0, 0, 0]), 0, su.new_record())
    assert off["status"] == su.OFF_TRACK and off["rec"]["ticks"] == 1.0
    nan = su.tick(track, np.array([3.0, 2.0, 0, 1.0, 0, 0, 0]), 0, su.new_record(), controls=(np.nan, 0.0), params=su.DYN, tick_no=2)
    assert nan["status"] == su.NONFINITE and nan["rec"]["ticks"] == 0.0 and nan["rec"]["fail_tick"] == 2.0


@pytest.mark.parametrize("N", [2, 3, 65])
@pytest.mark.parametrize("wrap", [False, True])
def test_window_visits_each_segment_once(N, wrap):
    M = N - 1
    windows = [(-1, -1), (0, 0), (8, 55), (M, M), (3 * M + 1, 5), (1, M - 1 if M > 1 else 0)]
    for back, fwd in windows:
        for seg in sorted({0, M // 2, M - 1}):
            segs = su.window_segments(N, wrap, seg, back, fwd)
            assert len(segs) == len(set(segs)) and all(0 <= s < M for s in segs), (back, fwd, seg, segs)
            assert seg in segs
            if back < 0 or back + fwd + 1 >= M and wrap:
                assert sorted(segs) == list(range(M))
            elif wrap:
                assert len(segs) == back + fwd + 1 and segs[0] == (seg - back) % M
            else:
                assert segs == list(range(max(seg - back, 0), min(seg + fwd, M - 1) + 1))
    if N == 65:
        seam = su.window_segments(N, True, 2, 8, 20)               # across the seam: 58 .. 63, 0 .. 22
        assert seam == list(range(58, 64)) + list(range(0, 23)) and su.runs(seam) == [list(range(58, 64)), list(range(0, 23))]
        assert su.window_segments(N, False, 2, 8, 20) == list(range(0, 23))      # clipped at the start
        assert su.window_segments(N, False, 60, 8, 20) == list(range(52, 64))    # and at the end
        assert su.window_segments(N, False, 30, 100, 100) == list(range(64))     # both
        assert su.window_segments(N, False, 999, 1, 1) == [62, 63]               # a segment index outside the line is clipped first


def _track_struct(**kw):
    d = dict(waypoints_dev=8, cum_dev=8, len_dev=8, length=10.0, lookahead=1.0, max_reacquire=2.0, half_width=0.0, N=5, wrap=1,
             win_back=8, win_fwd=55)
    d.update(kw)
    return _lib.SimTrack(**d)


def test_sim_advance_rejects_bad_arguments_without_gpu():
    lib = _lib.load()
    assert lib.irbfn_sim_record_doubles() == len(simulate.RECORD) == len(su.RECORD) == 7
    sel = _lib.ROLLOUT_ST_SELECT
    p = (C.c_float * 13)()

    def call(tr, mode=sel, controls=None, T=0, host=None, dev=None, n_sub=1, B=4, ptrs=(8,) * 6):
        st, sg, ss, rc, x, m = ptrs
        return lib.irbfn_sim_advance(C.byref(tr) if tr is not None else None, mode, 0, controls, T, host, dev, n_sub, st, sg, ss,
                                     rc, x, m, None, None, None, B, None)
    ok = _track_struct()
    assert call(None) == -1                                              # no track
    assert call(ok, B=-1) == -1
    assert call(_track_struct(N=1)) == -1
    assert call(ok, n_sub=0) == -1
    assert call(_track_struct(win_back=-1, win_fwd=5)) == -1
    assert call(_track_struct(win_back=5, win_fwd=-1)) == -1
    assert call(_track_struct(win_back=-2, win_fwd=-2)) == -1
    assert call(ok, controls=8, T=0, host=p) == -1                       # controls with T < 1
    for mode in (_lib.ROLLOUT_FULLINT, _lib.ROLLOUT_FRENET_LS, _lib.ROLLOUT_SPIRAL, 99, -1):
        assert call(ok, mode=mode) == -1
    assert call(_track_struct(lookahead=float("nan"))) == -1
    assert call(_track_struct(max_reacquire=-1.0)) == -1
    assert call(ok, controls=8, T=5) == -1                               # a plant step without parameters
    for k in range(6):                                                   # each required per-car pointer
        assert call(ok, ptrs=tuple(None if j == k else 8 for j in range(6))) == -1
    for name in ("waypoints_dev", "cum_dev", "len_dev"):
        assert call(_track_struct(**{name: None})) == -1
    # B = 0 is a no-op whatever the pointers; the window of the whole line and KS are accepted
    assert call(ok, B=0, ptrs=(None,) * 6) == 0
    assert call(_track_struct(win_back=-1, win_fwd=-1), mode=_lib.ROLLOUT_ST_KS, B=0) == 0
    assert call(_track_struct(N=1), B=0) == -1                           # but the scalars are still checked


def test_simulate_shape_and_type_errors():
    wp = su.straight_track(10)
    with pytest.raises(ValueError):
        simulate.Track(wp[:, :3])
    with pytest.raises(ValueError):
        simulate.Track(wp[:1])
    with pytest.raises(ValueError):
        simulate.Track(wp, window=(-1, 4))
    with pytest.raises(ValueError):
        simulate.Track(wp, window=(1, 2, 3))
    with pytest.raises(ValueError):
        simulate.Track(wp, lookahead=float("nan"))
    tr = simulate.Track(wp, wrap=False, lookahead=1.0, max_reacquire=3.0)
    cum, ln, length = su.arc_tables(wp, False)
    assert np.array_equal(tr.cum, cum) and np.array_equal(tr.len, ln) and tr.length == length == 4.5
    assert simulate.Track(wp, wrap=True).length == 9.0 and simulate.Track(wp, window=None).window == (-1, -1)
    net = WCRBFNet.from_config(dict(configs.model_card(2), num_kernels=16, out_features=10))
    s0 = np.zeros((3, 7), np.float32)
    with pytest.raises(TypeError):
        simulate.closed_loop(object(), {}, tr, s0, 2, dyn_params=su.DYN)
    with pytest.raises(TypeError):
        simulate.closed_loop(net, {}, wp, s0, 2, dyn_params=su.DYN)
    with pytest.raises(ValueError):
        simulate.closed_loop(net, {}, tr, np.zeros((3, 6), np.float32), 2, dyn_params=su.DYN)
    with pytest.raises(ValueError):
        simulate.closed_loop(net, {}, tr, s0, 2, dyn_params=su.DYN, plant_params=np.zeros((2, 13)))
    with pytest.raises(ValueError):
        simulate.closed_loop(net, {}, tr, s0, 2, dyn_params=su.DYN[:12])
    with pytest.raises(ValueError):
        simulate.closed_loop(net, {}, tr, s0, 2)
    with pytest.raises(ValueError):
        simulate.closed_loop(net, {}, tr, s0, 2, dyn_params=su.DYN, n_sub=0)
    with pytest.raises(ValueError):
        simulate.closed_loop(net, {}, tr, s0, -1, dyn_params=su.DYN)
    with pytest.raises(ValueError):
        simulate.closed_loop(net, {}, tr, s0, 2, dyn_params=su.DYN, mode=_lib.ROLLOUT_FULLINT)
