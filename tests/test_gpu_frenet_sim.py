"""The Frenet frame of the closed-loop simulation on the GPU (K14): ``irbfn_cartesian_to_frenet`` against the float64 statement
of tests/_frenet_sim_util.py, and ``irbfn_sim_advance_frenet`` / ``simulate.closed_loop_frenet`` against their parts --
``irbfn_sim_advance``, ``irbfn_cartesian_to_frenet``, ``irbfn_plan_queries_frenet`` -- bit for bit (no tolerance)."""
import numpy as np
import pytest
import torch

import _frenet_sim_util as fu
import _simulate_util as su
import test_frenet_sim_cpu as cpu_checks
from _cluster_util import cluster_case
from conftest import load_ckpt_fixture, load_deeper_fixture
from irbfn_amd import _lib, configs, dynamics as dyn, planner, simulate
from irbfn_amd.model import ClusterWCRBFNet, DeeperWCRBFNet, WCRBFNet

pytestmark = pytest.mark.gpu
SELECT, KS = _lib.ROLLOUT_ST_SELECT, _lib.ROLLOUT_ST_KS
COL = {n: k for k, n in enumerate(simulate.RECORD)}
T = 5
FR = dict(s=0, ey=1, delta=2, vx=3, vy=4, wz=5, epsi=6, curv=7)


def same(a, b):
    """bit for bit, NaN == NaN"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    raw = lambda v: v.reshape(-1).contiguous().view(torch.uint8)
    return bool(torch.equal(raw(a), raw(b)))


class Cars:
    """the per-car arrays of B cars and one tick on them, Cartesian (x [B,7]) or Frenet (x [B,8] and the pose)"""

    def __init__(self, track, state, frenet, seg=None):
        self.track, self.frenet_form = track, frenet
        self.state = state.clone() if torch.is_tensor(state) else torch.as_tensor(np.asarray(state, np.float32)).cuda().contiguous()
        B = self.B = self.state.shape[0]
        if seg is None:
            self.seg = track.seed(self.state[:, :2].double()).contiguous()
        else:
            self.seg = torch.as_tensor(np.asarray(seg), dtype=torch.int32).cuda()
        self.status = torch.zeros(B, dtype=torch.int32, device="cuda")
        self.record = simulate.new_record(B, torch)
        self.x = torch.full((B, 8 if frenet else 7), -7.0, dtype=torch.float32, device="cuda")
        self.mirror = torch.full((B,), -7, dtype=torch.int32, device="cuda")
        self.frenet = torch.full((B, 8), -7.0, dtype=torch.float64, device="cuda")
        self.goal = torch.full((B, 4), -7.0, dtype=torch.float64, device="cuda")
        self.dist = torch.full((B,), -7.0, dtype=torch.float64, device="cuda")
        self.t = torch.full((B,), -7.0, dtype=torch.float64, device="cuda")

    SHARED = ("state", "seg", "status", "record", "goal", "dist", "t")          # what both forms of the tick produce

    def arrays(self):
        return dict(state=self.state, seg=self.seg, status=self.status, record=self.record, x=self.x, mirror=self.mirror,
                    frenet=self.frenet, goal=self.goal, dist=self.dist, t=self.t)

    def advance(self, controls=None, params=None, n_sub=1, mode=SELECT, tick=0, rows=slice(None)):
        a = {k: v[rows] for k, v in self.arrays().items()}
        if torch.is_tensor(params) and params.dim() == 2:
            params = params[rows]
        kw = dict(controls=None if controls is None else controls[rows], plant_params=params, n_sub=n_sub, mode=mode, tick=tick,
                  goal_out=a["goal"], dist_out=a["dist"], t_out=a["t"])
        if self.frenet_form:
            simulate.advance_frenet(self.track, a["state"], a["seg"], a["status"], a["record"], a["x"], a["mirror"],
                                    frenet_out=a["frenet"], **kw)
        else:
            simulate.advance(self.track, a["state"], a["seg"], a["status"], a["record"], a["x"], a["mirror"], **kw)
        return self

    def snapshot(self):
        return {k: v.clone() for k, v in self.arrays().items()}


def controls_for(B, seed=0, T=T):
    rng = np.random.default_rng(seed + B)
    u = np.concatenate([rng.uniform(-4, 4, (B, T)), rng.uniform(-2, 2, (B, T))], axis=1).astype(np.float32)
    return torch.from_numpy(u).cuda()


# ------------------------------------------------------------------ 1. the conversion against the statement
BMAX = 257
TRACKS = {
    "straight": lambda: (su.straight_track(40), False),
    "oval_open": lambda: (su.oval(130), False),
    "oval_closed": lambda: (su.oval(131, closed=True), True),
    "hairpin": lambda: (su.hairpin(301), True),
    "ngon": lambda: (fu.ngon(1000, 5.0), True),
}
_reference = {}


def conversion_reference(name, windowed):
    """the statement for the BMAX cars of a track, computed once: (track, states f32, seg in or None, frenet, seg, d, t)"""
    key = (name, windowed)
    if key not in _reference:
        wp, wrap = TRACKS[name]()
        st = su.cars_on(wp, BMAX, seed=len(name), spread=0.25 if name != "ngon" else 0.1)
        st[:, 6] = np.random.default_rng(5).uniform(-0.3, 0.3, BMAX)             # beta
        track = fu.track_dict(wp, wrap)
        curv = fu.curvature(wp, wrap)
        seg_in = None
        if windowed:      # most windows (8 back, 55 forward) hold the car's segment, some miss it; some indices lie outside the line
            near = conversion_reference(name, False)[4]
            seg_in = (near + np.random.default_rng(7).integers(-70, 20, BMAX)).astype(np.int32)
        rows = [fu.to_frenet(track, curv, st[b].astype(np.float64), None if seg_in is None else int(seg_in[b])) for b in range(BMAX)]
        _reference[key] = (simulate.Track(wp, wrap=wrap), st, seg_in, np.array([r[0] for r in rows]),
                           np.array([r[1] for r in rows], np.int32), np.array([r[2] for r in rows]), np.array([r[3] for r in rows]),
                           curv)
    return _reference[key]


@pytest.mark.parametrize("windowed", [False, True])
@pytest.mark.parametrize("name", list(TRACKS))
def test_conversion_against_the_statement(gpu, name, windowed):
    track, st, seg_in, want, wseg, wd, wt, curv = conversion_reference(name, windowed)
    assert np.array_equal(track.curvature, curv)
    for B in (1, 16, 257):
        fr, seg, dist = simulate.to_frenet(track, st[:B], None if seg_in is None else seg_in[:B])
        fr, seg, dist = fr.cpu().numpy(), seg.cpu().numpy(), dist.cpu().numpy()
        assert fr.shape == (B, 8) and seg.dtype == np.int32 and dist.dtype == np.float64
        assert np.array_equal(seg, wseg[:B])
        assert np.array_equal(dist, wd[:B])                                   # the arithmetic of irbfn_nearest_point: exact
        assert np.array_equal(fr[:, FR["s"]], want[:B, FR["s"]])
        assert np.array_equal(np.signbit(fr[:, FR["ey"]]), np.signbit(want[:B, FR["ey"]]))         # the side
        assert np.array_equal(np.abs(fr[:, FR["ey"]]), dist) and np.array_equal(fr[:, FR["ey"]], want[:B, FR["ey"]])
        assert np.array_equal(fr[:, FR["delta"]], want[:B, FR["delta"]]) and np.array_equal(fr[:, FR["wz"]], want[:B, FR["wz"]])
        for col in ("vx", "vy", "epsi", "curv"):
            err = np.max(np.abs(fr[:, FR[col]] - want[:B, FR[col]]))
            assert err <= 1e-12, (col, err)
    if name != "straight":
        assert 0.2 < np.mean(want[:, FR["ey"]] > 0) < 0.8 and np.abs(want[:, FR["epsi"]]).max() <= np.pi
    if windowed and name in ("hairpin", "oval_closed"):
        full = conversion_reference(name, False)
        assert (full[4] != wseg).sum() >= 3                                    # some windows missed the nearest segment
    # t comes out of the stand-alone entry point only through the C ABI
    lib = _lib.load()
    sd = torch.as_tensor(st).cuda()
    t = torch.empty(BMAX, dtype=torch.float64, device="cuda")
    frd = torch.empty((BMAX, 8), dtype=torch.float64, device="cuda")
    sg = None if seg_in is None else torch.as_tensor(seg_in).cuda()
    import ctypes as C
    tr = track.struct(torch)
    rc = lib.irbfn_cartesian_to_frenet(C.byref(tr), track.curvature_device(torch).data_ptr(), sd.data_ptr(),
                                       sg.data_ptr() if sg is not None else None, frd.data_ptr(), None, None, t.data_ptr(), BMAX,
                                       torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and np.array_equal(t.cpu().numpy(), wt) and np.array_equal(frd.cpu().numpy()[:, 0], want[:, 0])


# ------------------------------------------------------------------ 2. signs and the mirror threshold
def test_signs_and_the_mirror_threshold_on_a_straight_line(gpu):
    wp = su.straight_track(40)
    wp[:, 1] = 0.0                                           # along +x at y = 0, x = 1 .. 20.5
    track = simulate.Track(wp, wrap=False, lookahead=1.25, max_reacquire=5.0, window=None)
    edge = np.float32(-0.05)
    assert float(edge) < -0.05 < float(np.nextafter(edge, np.float32(0)))
    ys = np.array([0.0, 0.5, -0.5, edge, np.nextafter(edge, np.float32(0)), 0.05, -0.25, 0.25], np.float32)
    psis = np.array([0.0, 0.3, -0.3, 0.2, 0.2, -0.2, 0.1, -0.1], np.float32)
    B = len(ys)
    st = np.zeros((B, 7), np.float32)
    st[:, 0] = 2.25 + 0.5 * np.arange(B)                     # lattice points: t = 0.5 exactly, d = |y|
    st[:, 1], st[:, 4] = ys, psis
    st[:, 2], st[:, 3], st[:, 5], st[:, 6] = 0.125, 2.0, 0.75, 0.25
    cars = Cars(track, st, True).advance()
    assert bool((cars.status == 0).all())
    fr, x, m = cars.frenet.cpu().numpy(), cars.x.cpu().numpy(), cars.mirror.cpu().numpy()
    assert np.array_equal(fr[:, FR["ey"]], ys.astype(np.float64))                # ey = y: the sign of y, left is positive
    assert not np.signbit(fr[0, FR["ey"]]) and fr[0, FR["ey"]] == 0.0            # d = 0: +0
    assert np.array_equal(np.sign(fr[:, FR["epsi"]]), np.sign(psis)) and np.abs(fr[:, FR["epsi"]] - psis.astype(np.float64)).max() <= 1e-15
    assert m.tolist() == [0, 0, 1, 1, 0, 0, 1, 0]
    assert np.all(fr[:, FR["vy"]] > 0) and np.all(fr[:, FR["wz"]] == 0.75) and np.all(fr[:, FR["curv"]] == 0.0)
    sgn = np.where(m == 1, -1.0, 1.0)
    goal_v = cars.goal.cpu().numpy()[:, 3]
    want = np.stack([sgn * fr[:, 1], fr[:, 2], fr[:, 3], sgn * fr[:, 4], goal_v, sgn * fr[:, 5], sgn * fr[:, 6], fr[:, 7]],
                    axis=1).astype(np.float32)
    assert np.array_equal(x, want)
    assert np.all(x[m == 1, 0] >= np.float32(0.05)) and x[2, 6] == np.float32(0.3) and x[3, 6] < 0     # mirrored rows: ey, epsi negated


# ------------------------------------------------------------------ 3. the fused tick equals its parts
def check_parts(fren, cart, before):
    """the Frenet tick `fren` against the Cartesian tick `cart` from the same inputs, the conversion of its new state with the
    segments it started from, and the query builder; `before`: fren's snapshot in front of the call"""
    old_seg = before["seg"]
    for n in Cars.SHARED:
        assert same(fren.arrays()[n], cart.arrays()[n]), n
    ok = fren.status == 0
    fr, seg, dist = simulate.to_frenet(fren.track, fren.state, old_seg)
    assert same(fren.frenet[ok], fr[ok]) and same(fren.seg[ok], seg[ok]) and same(fren.dist[ok], dist[ok])
    x, _, mirror = planner.build_queries_frenet(fren.frenet, fren.goal[:, 3].contiguous())
    assert same(fren.x[ok], x[ok]) and same(fren.mirror[ok], mirror[ok])
    for n in ("x", "frenet", "mirror"):                      # stopped in this call or before it: nothing of step 6
        assert same(fren.arrays()[n][~ok], before[n][~ok]), n
    return ok


def tick_cases():
    oval = su.oval(130)
    yield "oval_wrap", simulate.Track(oval, wrap=True, lookahead=1.5, max_reacquire=3.0, half_width=1.2), su.cars_on(oval, 257, spread=0.8), None
    yield "oval_open", simulate.Track(oval, wrap=False, lookahead=1.5, max_reacquire=3.0, half_width=1.2), su.cars_on(oval, 65, spread=0.8), None
    hp = su.hairpin(301)
    segs = np.array([20, 40, 77, 3, 0, 7, 100, 130, 299, 295, 292, 150])
    st = np.zeros((len(segs), 7), np.float32)
    st[:, :2] = hp[segs, :2] + 0.5 * (hp[segs + 1, :2] - hp[segs, :2])
    st[:8, 1] += 0.3
    st[:, 3] = 2.0
    yield "hairpin", simulate.Track(hp, wrap=True, lookahead=1.0, max_reacquire=50.0, window=(8, 55)), st, segs
    xy = np.array([[0, 0], [1, 0], [2, 0], [2, 1], [1, 1], [0, 1], [0, 0]], np.float64)       # K12's tie across the seam
    nxt = np.roll(xy, -1, axis=0) - xy
    rect = np.concatenate([xy, np.arctan2(nxt[:, 1], nxt[:, 0])[:, None], np.full((7, 1), 2.0)], axis=1)
    st = np.zeros((2, 7), np.float32)
    st[0, :2], st[1, :2] = [-0.25, -0.25], [2.25, -0.25]
    st[:, 3] = 1.0
    yield "seam_tie", simulate.Track(rect, wrap=True, lookahead=0.75, max_reacquire=3.0, window=(2, 2)), st, np.array([0, 0])


TICK_CASES = {name: (track, st, seg) for name, track, st, seg in tick_cases()}


@pytest.mark.parametrize("per_car", [False, True])
@pytest.mark.parametrize("n_sub,mode", [(1, SELECT), (3, KS), (3, SELECT), (1, KS)])
@pytest.mark.parametrize("name", list(TICK_CASES))
def test_fused_tick_equals_its_parts(gpu, name, n_sub, mode, per_car):
    track, st, seg = TICK_CASES[name]
    B = st.shape[0]
    u = controls_for(B)
    if name in ("hairpin", "seam_tie"):
        u = u * 0.1
    p = np.asarray(configs.DYN_PARAMS, np.float32)
    if per_car:
        p = torch.from_numpy(np.tile(p, (B, 1))).cuda()
        p[:, 0] = torch.linspace(0.5, 1.1, B)
    fren, cart = Cars(track, st, True, seg), Cars(track, st, False, seg)
    before = fren.snapshot()
    ok0 = check_parts(fren.advance(), cart.advance(), before)
    if name == "seam_tie":
        assert fren.seg.tolist() == [0, 1] and fren.frenet[:, FR["ey"]].tolist() == [-np.sqrt(0.125)] * 2
    before = fren.snapshot()
    ok1 = check_parts(fren.advance(u, p, n_sub, mode, tick=1), cart.advance(u, p, n_sub, mode, tick=1), before)
    assert int(ok1.sum()) >= max(1, B // 3) and int((ok0 & ~ok1).sum()) == int((~ok1).sum()) - int((~ok0).sum())
    if name == "oval_wrap":
        assert int((~ok1).sum()) > 0 and int(fren.mirror[ok1].sum()) > 0 and int((fren.mirror[ok1] == 0).sum()) > 0


# ------------------------------------------------------------------ 4. freezing, cutting, repeating, arguments
def test_each_status_freezes_its_car_and_no_other(gpu):
    wp = su.straight_track(10)                               # x = 1 .. 5.5 at y = 2, open
    track = simulate.Track(wp, wrap=False, lookahead=1.0, max_reacquire=2.0, half_width=2.5, window=None)
    B = 16
    st = np.zeros((B, 7), np.float32)
    st[:, 0] = 1.25 + 0.25 * (np.arange(B) % 8)
    st[:, 1] = 2.0 + 0.125 * (np.arange(B) % 3)
    st[:, 3] = 1.0
    FAR, END, OFF, NAN = 1, 6, 9, 14
    st[FAR, 1] = 2.0 + 2.25                                  # between max_reacquire and half_width
    st[END, :2] = [5.5, 2.0]                                 # the last way-point: no intersection ahead
    st[OFF, 1] = 2.0 - 2.75                                  # beyond half_width
    u = controls_for(B)
    u[:, 0], u[:, T] = 0.5, 0.0
    u[NAN, 0] = float("nan")
    p = configs.DYN_PARAMS
    cars = Cars(track, st, True).advance(tick=0)
    first = cars.snapshot()
    assert [int(cars.status[k]) for k in (FAR, END, OFF)] == [_lib.SIM_LOST, _lib.SIM_LOST, _lib.SIM_OFF_TRACK]
    assert int((cars.status != 0).sum()) == 3
    for k in (FAR, END, OFF):                                # counted, no pose and no query
        assert float(cars.record[k, COL["ticks"]]) == 1.0 and float(cars.x[k, 0]) == -7.0 and float(cars.frenet[k, 0]) == -7.0
    cars.advance(u, p, tick=1)
    second = cars.snapshot()
    assert int(cars.status[NAN]) == _lib.SIM_NONFINITE and float(cars.record[NAN, COL["fail_tick"]]) == 1.0
    assert same(second["x"][NAN], first["x"][NAN]) and same(second["frenet"][NAN], first["frenet"][NAN])
    assert int((cars.status != 0).sum()) == 4
    for k in (FAR, END, OFF):
        assert all(same(second[n][k], first[n][k]) for n in first), k
    u2 = u.clone()
    u2[NAN, 0] = 0.5
    cars.advance(u2, p, tick=2)
    for k in (FAR, END, OFF, NAN):
        assert all(same(cars.arrays()[n][k], second[n][k]) for n in second), k
    keep = torch.tensor([k for k in range(B) if k not in (FAR, END, OFF, NAN)]).cuda()
    alone = Cars(track, st[keep.cpu().numpy()], True).advance(tick=0).advance(u[keep], p, tick=1).advance(u2[keep], p, tick=2)
    assert bool((alone.status == 0).all())
    assert all(same(cars.arrays()[n][keep], alone.arrays()[n]) for n in second)


def test_a_nan_curvature_stops_the_car_one_tick_later(gpu):
    wp = su.straight_track(20)
    k = np.zeros(20)
    k[4:7] = np.nan
    track = simulate.Track(wp, wrap=False, lookahead=1.0, max_reacquire=2.0, window=None, curvature=k)
    st = np.zeros((3, 7), np.float32)
    st[:, 0], st[:, 1], st[:, 3] = [1.75, 3.25, 6.25], 2.0, 1.0          # the second car sits on segment 4
    cars = Cars(track, st, True).advance()
    assert cars.status.tolist() == [0, 0, 0] and torch.isnan(cars.x[:, 7]).tolist() == [False, True, False]
    net, params = frenet_net("12regions")
    ctrl, _ = planner.plan_tick(net, params, cars.x, cars.mirror, rollout=False)
    assert bool(torch.isnan(ctrl[1]).any())
    cars.advance(ctrl, configs.DYN_PARAMS, tick=1)
    assert cars.status.tolist() == [0, _lib.SIM_NONFINITE, 0]


def test_cars_cut_into_two_calls_and_repeats(gpu):
    B, cut = 257, 37
    wp = su.oval(130)
    track = simulate.Track(wp, wrap=True, lookahead=1.5, max_reacquire=3.0, half_width=1.2)
    st = su.cars_on(wp, B, spread=0.8)
    u = controls_for(B)
    rows = torch.from_numpy(np.tile(np.asarray(configs.DYN_PARAMS, np.float32), (B, 1))).cuda()
    rows[:, 0] = torch.linspace(0.5, 1.1, B)
    one = Cars(track, st, True).advance().advance(u, rows, 2, SELECT, tick=1)
    two = Cars(track, st, True)
    for rs in (slice(0, cut), slice(cut, B)):
        two.advance(rows=rs)
    for rs in (slice(cut, B), slice(0, cut)):
        two.advance(u, rows, 2, SELECT, tick=1, rows=rs)
    assert 0 < int((one.status != 0).sum()) < B
    assert all(same(a, b) for a, b in zip(one.arrays().values(), two.arrays().values()))
    again = Cars(track, st, True).advance().advance(u, rows, 2, SELECT, tick=1)
    assert all(same(a, b) for a, b in zip(one.arrays().values(), again.arrays().values()))
    a, b = simulate.to_frenet(track, st), simulate.to_frenet(track, st)
    halves = [simulate.to_frenet(track, st[:cut]), simulate.to_frenet(track, st[cut:])]
    for k in range(3):
        assert same(a[k], b[k]) and same(a[k], torch.cat([halves[0][k], halves[1][k]]))


def test_no_cars_and_bad_arguments_with_a_live_device(gpu):
    wp = su.oval(130)
    track = simulate.Track(wp, wrap=True)
    empty = Cars(track, np.zeros((0, 7), np.float32), True, seg=np.zeros(0, np.int32))
    empty.advance()                                          # B = 0: IRBFN_OK, raises nothing
    fr, seg, dist = simulate.to_frenet(track, np.zeros((0, 7), np.float32))
    assert fr.shape == (0, 8) and seg.shape == (0,) and dist.shape == (0,)
    cpu_checks.test_sim_advance_frenet_rejects_bad_arguments_without_gpu()
    cpu_checks.test_cartesian_to_frenet_rejects_bad_arguments_without_gpu()
    cars = Cars(track, su.cars_on(wp, 4), True)
    with pytest.raises(ValueError, match="x must be"):       # the Cartesian query's width
        simulate.advance_frenet(track, cars.state, cars.seg, cars.status, cars.record, cars.x[:, :7].contiguous(), cars.mirror)
    with pytest.raises(ValueError, match="frenet_out"):
        simulate.advance_frenet(track, cars.state, cars.seg, cars.status, cars.record, cars.x, cars.mirror,
                                frenet_out=cars.frenet.float())


# ------------------------------------------------------------------ 5. frame <-> model on the device
def frame_model_on_device(kind):
    """-> (pose after one ST_KS plant tick, irbfn_rollout_forward(FRENET_LS, T = 1) from the pose before it), [B,8] float64"""
    wp, wrap, (s, ey, epsi), delta, u, p = fu.frame_model_case(kind)
    track = simulate.Track(wp, wrap=wrap, lookahead=1.0, max_reacquire=5.0)
    x, y, psi = track.pose_at(s, ey, epsi)
    st = fu.ks_state(x, y, psi, delta, 3.0).astype(np.float32)
    B = st.shape[0]
    cars = Cars(track, st, True).advance(mode=KS)
    assert bool((cars.status == 0).all())
    fr0 = cars.frenet.clone()
    ctrl = torch.from_numpy(np.tile(u, (B, 1)).astype(np.float32)).cuda()
    cars.advance(ctrl, p.astype(np.float32), 1, KS, tick=1)
    assert bool((cars.status == 0).all())
    model = dyn.rollout_forward(_lib.ROLLOUT_FRENET_LS, torch.cat([fr0.float(), ctrl], dim=1).contiguous(), p.astype(np.float32), 1)
    return cars.frenet.cpu().numpy(), model[:, -1, :].double().cpu().numpy(), float(np.abs(track.curvature).max()) * 3.0 * p[8]


def test_plant_tick_agrees_with_the_frenet_model_on_a_straight_line(gpu):
    fr1, model, _ = frame_model_on_device("straight")
    for col in ("ey", "delta", "vx", "epsi"):
        err = np.max(np.abs(fr1[:, FR[col]] - model[:, FR[col]]))
        print(f"straight line, {col}: max |d| = {err:.3e}")
        assert err <= 1e-5, (col, err)


def test_plant_tick_agrees_with_the_frenet_model_on_the_1000_gon(gpu):
    fr1, model, kvdt = frame_model_on_device("ngon")
    d_epsi, d_ey = np.max(np.abs(fr1[:, FR["epsi"]] - model[:, FR["epsi"]])), np.max(np.abs(fr1[:, FR["ey"]] - model[:, FR["ey"]]))
    print(f"1000-gon: max |d epsi| = {d_epsi:.3e}, max |d ey| = {d_ey:.3e}")
    assert d_epsi <= 0.25 * kvdt and d_ey <= 5e-4
    assert np.max(np.abs(fr1[:, FR["delta"]] - model[:, FR["delta"]])) <= 1e-5
    assert np.max(np.abs(fr1[:, FR["vx"]] - model[:, FR["vx"]])) <= 1e-5


# ------------------------------------------------------------------ 6. closed_loop_frenet against the composed loop
def frenet_net(kind):
    if kind == "12regions":
        cfg, params = load_ckpt_fixture("dnmpc_12regions_frenet_l1_bigdata")[:2]
        return WCRBFNet.from_config(cfg), params
    if kind == "deeper":
        cfg, params = load_deeper_fixture()[:2]
        return DeeperWCRBFNet.from_config(cfg), params
    _, cfg, params, _ = cluster_case(5, R=3, K=16, O=10, B=1, D=8)
    return ClusterWCRBFNet(**cfg), params


def composed_loop(net, params, track, state0, ticks, p, mode):
    """plan_tick -> irbfn_sim_advance -> irbfn_cartesian_to_frenet -> irbfn_plan_queries_frenet, per tick"""
    cars = Cars(track, state0, False)
    B = cars.B
    x = torch.zeros((B, 8), dtype=torch.float32, device="cuda")
    mirror = torch.zeros(B, dtype=torch.int32, device="cuda")
    for k in range(ticks + 1):
        old = cars.seg.clone()
        if k == 0:
            cars.advance(mode=mode, tick=0)
        else:
            ctrl, _ = planner.plan_tick(net, params, x, mirror, rollout=False, mode=mode)
            cars.advance(ctrl, p, 1, mode, tick=k)
        live = cars.status == 0
        fr, _, _ = simulate.to_frenet(track, cars.state, old)
        qx, _, qm = planner.build_queries_frenet(fr, cars.goal[:, 3].contiguous())
        x = torch.where(live[:, None], qx, x)
        mirror = torch.where(live, qm, mirror)
    return cars


@pytest.mark.parametrize("kind", ["12regions", "deeper", "cluster"])
def test_closed_loop_frenet_equals_the_composed_loop(gpu, kind):
    net, params = frenet_net(kind)
    assert net.in_features == 8 and net.out_features == {"12regions": 2, "deeper": 10, "cluster": 10}[kind]
    wp = fu.ellipse(200)                                     # radius of curvature >= 16 / 6 m, line speed 4 m/s
    track = simulate.Track(wp, wrap=True, lookahead=1.0, max_reacquire=4.0, half_width=3.0)
    assert np.abs(track.curvature).max() <= 0.4
    B, ticks = 33, 20
    rng = np.random.default_rng(11)
    x, y, psi = track.pose_at(rng.uniform(0.0, track.length - 1.0, B), rng.uniform(-0.3, 0.3, B), rng.uniform(-0.2, 0.2, B))
    st = fu.ks_state(x, y, psi, 0.0, rng.uniform(3.0, 4.5, B)).astype(np.float32)
    st[B - 1, :2] += 40.0                                    # one car far beyond half_width
    p = configs.DYN_PARAMS
    want = composed_loop(net, params, track, st, ticks, p, SELECT)
    res = simulate.closed_loop_frenet(net, params, track, st, ticks, dyn_params=p, record_every=5)
    assert same(res.state, want.state) and same(res.status, want.status)
    col = lambda name: want.record[:, COL[name]]
    assert same(res.fail_tick, col("fail_tick").to(torch.int64)) and same(res.ticks, col("ticks").to(torch.int64))
    assert same(res.max_dev, col("max_d")) and same(res.progress, col("progress"))
    assert same(res.rms_dev, torch.sqrt(col("sum_d2") / col("ticks"))) and same(res.mean_abs_dv, col("sum_dv") / col("ticks"))
    assert res.states.shape == (4, B, 7) and same(res.states[-1], res.state)
    assert int(res.status[B - 1]) == _lib.SIM_OFF_TRACK and int(res.fail_tick[B - 1]) == 0
    assert not same(res.state[:B - 1], torch.as_tensor(st[:B - 1]).cuda())       # the cars moved
