"""A float64 / NumPy statement of the Frenet frame of the closed-loop simulation (include/irbfn_hip.h:
irbfn_cartesian_to_frenet, irbfn_sim_advance_frenet), composed from tests/_simulate_util.py and the oracle's restatements, and
the inputs the Frenet simulation tests share.  A plain module (no fixtures, no hooks).

  wrap        : e - 2 pi rint(e / 2 pi).
  curvature   : the way-point curvatures of a race line.
  pose        : the Frenet row of one car from its nearest segment.
  to_frenet   : search (whole line or window) and pose of one car.
  tick        : _simulate_util.tick with step 6 replaced by the pose and oracle.plan_query_frenet.
Every operation is a rounded float64 one (Python floats: no product is fused into a sum)."""
import math

import numpy as np

import _simulate_util as su
from oracle import irbfn_oracle as orc

TWO_PI = 2.0 * math.pi


def wrap(e):
    return e - TWO_PI * np.rint(e / TWO_PI)


def curvature(wp, wrap_track):
    """kappa [N]: wrap(theta_{i+1} - theta_{i-1}) / (len_{i-1} + len_i); the ends across the seam with the closing segment's
    length on a wrap track, one-sided on an open one"""
    wp = np.asarray(wp, np.float64)
    N = wp.shape[0]
    th = wp[:, 2]
    _, ln, _ = su.arc_tables(wp, wrap_track)
    c = wp[0, :2] - wp[-1, :2]
    closing = math.sqrt(c[0] * c[0] + c[1] * c[1])
    k = np.empty(N)
    for i in range(1, N - 1):
        k[i] = wrap(th[i + 1] - th[i - 1]) / (ln[i - 1] + ln[i])
    if wrap_track:
        k[0] = wrap(th[1] - th[N - 1]) / (closing + ln[0])
        k[N - 1] = wrap(th[0] - th[N - 2]) / (ln[N - 2] + closing)
    else:
        k[0] = wrap(th[1] - th[0]) / ln[0]
        k[N - 1] = wrap(th[N - 1] - th[N - 2]) / ln[N - 2]
    return k


def pose(wp, curv, cum, ln, state, d, t, i):
    """[s, ey, delta, vx, vy, wz, epsi, curv] of the single-track state [x, y, delta, v, psi, psi_dot, beta] whose nearest
    segment is i at parameter t and distance d"""
    x, y, delta, v, psi, wz, beta = [float(a) for a in state]
    d, t = float(d), float(t)
    dx, dy = float(wp[i + 1, 0] - wp[i, 0]), float(wp[i + 1, 1] - wp[i, 1])
    c = dx * (y - float(wp[i, 1])) - dy * (x - float(wp[i, 0]))
    ey = d if c >= 0.0 else -d
    s = float(cum[i]) + t * float(ln[i])
    th = float(wp[i, 2]) + t * float(wrap(float(wp[i + 1, 2]) - float(wp[i, 2])))
    epsi = float(wrap(psi - th))
    k = float(curv[i]) + t * (float(curv[i + 1]) - float(curv[i]))
    return np.array([s, ey, delta, v * math.cos(beta), v * math.sin(beta), wz, epsi, k])


def to_frenet(track, curv, state, seg=None):
    """track: the dict of _simulate_util.tick.  seg None: every segment; else the track's window around it.
    -> (frenet [8], i, d, t)"""
    wp, wrap_track = np.asarray(track["wp"], np.float64), bool(track["wrap"])
    N = wp.shape[0]
    cum, ln, _ = su.arc_tables(wp, wrap_track)
    back, fwd = (-1, -1) if seg is None else track["window"]
    state = np.asarray(state, np.float64)
    d, t, i = su.nearest_in(state[:2], wp[:, :2], su.window_segments(N, wrap_track, 0 if seg is None else seg, back, fwd))
    return pose(wp, curv, cum, ln, state, d, t, i), i, d, t


def tick(track, curv, state, seg, rec, controls=None, params=None, n_sub=1, tick_no=0):
    """One Frenet tick of one car: steps 1-5 are _simulate_util.tick's; a car that drives on gets frenet [8], and x [8] float32
    and mirror from oracle.plan_query_frenet(frenet, goal speed)"""
    out = su.tick(track, state, seg, rec, controls=controls, params=params, n_sub=n_sub, tick_no=tick_no)
    if out["status"] != su.OK:
        return out
    wp = np.asarray(track["wp"], np.float64)
    cum, ln, _ = su.arc_tables(wp, bool(track["wrap"]))
    fr = pose(wp, curv, cum, ln, out["state"], out["d"], out["t"], out["seg"])
    x, mirror, _ = orc.plan_query_frenet(fr, out["goal"][3])
    out.update(frenet=fr, x=x, mirror=int(mirror))
    return out


def ngon(N, R, ccw=True, v=3.0):
    """the N corners of a regular N-gon of radius R as way-points [N,4]: heading of the segment that leaves each corner (the
    last one closes the polygon), speed v"""
    a = TWO_PI * np.arange(N) / N
    if not ccw:
        a = -a
    xy = np.stack([R * np.cos(a), R * np.sin(a)], axis=1)
    nxt = np.roll(xy, -1, axis=0) - xy
    return np.concatenate([xy, np.arctan2(nxt[:, 1], nxt[:, 0])[:, None], np.full((N, 1), v)], axis=1)


def track_dict(wp, wrap_track, lookahead=1.0, max_reacquire=20.0, half_width=0.0, window=(8, 55)):
    return dict(wp=np.asarray(wp, np.float64), wrap=wrap_track, lookahead=lookahead, max_reacquire=max_reacquire,
                half_width=half_width, window=window)


def ks_state(x, y, psi, delta, v):
    """single-track rows [x, y, delta, v, psi, 0, 0] of the kinematic model"""
    x, y, psi, delta, v = np.broadcast_arrays(x, y, psi, delta, v)
    z = np.zeros_like(x, dtype=np.float64)
    return np.stack([x, y, delta, v, psi, z, z], axis=-1).astype(np.float64)


def frame_model_case(kind, B=40, seed=0):
    """The inputs of the frame <-> model check, shared by the CPU and the GPU test: B kinematic cars at v = 3 on a straight line
    along +x or on the 1000-gon of radius 5 m (counter-clockwise), |ey|, |epsi| <= 0.4, |delta| <= 0.2, controls a = 1,
    sv = 0.5, dt = 0.01.  -> (way-points, wrap, Frenet seeds (s, ey, epsi), delta, controls [2], parameters [13])"""
    rng = np.random.default_rng(seed)
    if kind == "straight":
        wp, wrap_track = su.straight_track(60, step=0.5, v=3.0), False
        s = rng.uniform(2.0, 25.0, B)
    else:
        wp, wrap_track = ngon(1000, 5.0), True
        s = rng.uniform(0.5, 30.0, B)
    ey, epsi, delta = rng.uniform(-0.4, 0.4, B), rng.uniform(-0.4, 0.4, B), rng.uniform(-0.2, 0.2, B)
    p = su.DYN.copy()
    p[8] = 0.01
    return wp, wrap_track, (s, ey, epsi), delta, np.array([1.0, 0.5]), p


def ellipse(N, a=6.0, b=4.0, v=4.0):
    """a closed line of N way-points on the ellipse with semi-axes a, b (smallest radius of curvature b^2 / a), counter-clockwise,
    headings along the segments, line speed v"""
    th = TWO_PI * np.arange(N) / N
    xy = np.stack([a * np.cos(th), b * np.sin(th)], axis=1)
    nxt = np.roll(xy, -1, axis=0) - xy
    return np.concatenate([xy, np.arctan2(nxt[:, 1], nxt[:, 0])[:, None], np.full((N, 1), v)], axis=1)
