"""A float64 / NumPy statement of one tick of the closed-loop simulation (include/irbfn_hip.h: irbfn_sim_advance), composed
from the oracle's restatements of the stages, and the inputs the simulation tests share.  A plain module (no fixtures, no
hooks).

  window_segments : the segments a window visits, in visiting order.
  nearest_in      : oracle.nearest_point(skip_nan=True) on each contiguous run of those segments; smallest (distance, index).
  fold_stats      : the statistics of one tick folded into a record.
  tick            : the whole tick of one car.
Way-points sit on the quarter-integer lattice of _planner_front_util, so that arc lengths and their sums are exact."""
import math

import numpy as np

from oracle import irbfn_oracle as orc

OK, NONFINITE, OFF_TRACK, LOST = 0, 1, 2, 3
RECORD = ("ticks", "sum_d2", "max_d", "sum_dv", "progress", "s_last", "fail_tick")


def window_segments(N, wrap, seg, back, fwd):
    """segments visited from the last nearest segment `seg`: seg - back .. seg + fwd, modulo N - 1 on a wrap track, else
    clipped to [0, N - 2]; back = fwd = -1 (or a window at least as long as a wrap track): all of them, from 0"""
    M = N - 1
    s = min(max(int(seg), 0), M - 1)
    if back < 0 or (wrap and back + fwd + 1 >= M):
        return list(range(M))
    if wrap:
        return [(s - back + k) % M for k in range(back + fwd + 1)]
    return list(range(max(s - back, 0), min(s + fwd, M - 1) + 1))


def runs(segs):
    """contiguous ascending runs of a visiting order"""
    out = []
    for s in segs:
        if out and out[-1][-1] + 1 == s:
            out[-1].append(s)
        else:
            out.append([s])
    return out


def nearest_in(point, xy, segs):
    """-> (d, t, i) over the segments `segs` of the polyline xy [N,2]: the smallest distance, ties to the lowest index"""
    best = (np.inf, 0.0, None)
    for run in runs(segs):
        _, d, t, k = orc.nearest_point(np.asarray(point, np.float64), xy[run[0]:run[-1] + 2], skip_nan=True)
        if not np.isfinite(d):
            continue
        i = run[0] + k
        if d < best[0] or (d == best[0] and i < best[2]):
            best = (float(d), float(t), i)
    return best if best[2] is not None else (np.inf, 0.0, 0)


def arc_tables(wp, wrap):
    """cum / len [N-1] and the line's length, float64"""
    d = wp[1:, :2] - wp[:-1, :2]
    ln = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    cum = np.concatenate([[0.0], np.cumsum(ln)[:-1]])
    c = wp[0, :2] - wp[-1, :2]
    return cum, ln, float(ln.sum() + (math.sqrt(c[0] * c[0] + c[1] * c[1]) if wrap else 0.0))


def new_record():
    return dict(ticks=0.0, sum_d2=0.0, max_d=0.0, sum_dv=0.0, progress=0.0, s_last=0.0, fail_tick=-1.0)


def fold_stats(rec, d, t, i, v, wp, cum, ln, length, wrap):
    """step 3, in its order; every operation a rounded float64 one"""
    first = rec["ticks"] == 0.0
    rec["ticks"] += 1.0
    rec["sum_d2"] += d * d
    rec["max_d"] = max(rec["max_d"], d)
    rec["sum_dv"] += abs(float(v) - wp[i, 3])
    s = cum[i] + t * ln[i]
    if not first:
        e = s - rec["s_last"]
        if wrap:
            if e > length / 2.0:
                e -= length
            elif e <= -length / 2.0:
                e += length
        rec["progress"] += e
    rec["s_last"] = s
    return rec


def tick(track, state, seg, rec, controls=None, params=None, n_sub=1, tick_no=0):
    """One tick of one car in float64.  track: dict(wp [N,4], wrap, lookahead, max_reacquire, half_width, window (back, fwd));
    state [7]; controls (a, sv) or None; the plant is the select model (oracle.dynamic_st_onestep).
    -> dict(state, seg, status, rec, and, for a car that drives on, goal [4], d, t, x [7] float32, mirror)."""
    wp, wrap = np.asarray(track["wp"], np.float64), bool(track["wrap"])
    N = wp.shape[0]
    cum, ln, length = arc_tables(wp, wrap)
    state = np.asarray(state, np.float64).copy()
    out = dict(state=state, seg=seg, status=OK, rec=rec)
    if controls is not None:
        p = np.asarray(params, np.float64).copy()
        p[8] = p[8] / n_sub
        for _ in range(n_sub):
            state = orc.dynamic_st_onestep(state[None], np.asarray(controls, np.float64)[None], p)[0]
        out["state"] = state
        if not np.isfinite(state).all():
            rec["fail_tick"] = float(tick_no)
            out["status"] = NONFINITE
            return out
    back, fwd = track["window"]
    d, t, i = nearest_in(state[:2], wp[:, :2], window_segments(N, wrap, seg, back, fwd))
    fold_stats(rec, d, t, i, state[3], wp, cum, ln, length, wrap)
    status, goal = OK, None
    if track["half_width"] > 0 and d > track["half_width"]:
        status = OFF_TRACK
    elif d < track["lookahead"]:
        _, fi, _ = orc.intersect_point(state[:2], track["lookahead"], wp[:, :2], i + t, wrap)
        if fi is None:
            status = LOST
        else:
            goal = wp[(fi + N) % N]
    elif d < track["max_reacquire"]:
        goal = wp[i]
    else:
        status = LOST
    out["status"] = status
    if status != OK:
        rec["fail_tick"] = float(tick_no)
        return out
    x, mirror, _ = orc.plan_query_cartesian(state, goal, unfused=True)
    out.update(seg=i, goal=goal, d=d, t=t, x=x, mirror=int(mirror))
    return out


def straight_track(N, step=0.5, v=2.0):
    """N way-points `step` apart along +x from (1, 2), heading 0, speed v: all on the quarter-integer lattice"""
    x = 1.0 + step * np.arange(N)
    return np.stack([x, np.full(N, 2.0), np.zeros(N), np.full(N, v)], axis=1)


def oval(N, closed=False):
    """a closed line of N way-points about 0.6 m apart; `closed`: the last way-point repeats the first"""
    n = N - 1 if closed else N
    th = np.linspace(0, 2 * np.pi, n, endpoint=False)
    r = 0.1 * n
    xy = np.stack([r * np.cos(th), 0.6 * r * np.sin(th)], axis=1)
    head = np.arctan2(np.roll(xy[:, 1], -1) - xy[:, 1], np.roll(xy[:, 0], -1) - xy[:, 0])
    wp = np.concatenate([xy, head[:, None], (2.0 + np.cos(2 * th))[:, None]], axis=1)
    return np.vstack([wp, wp[:1]]) if closed else wp


def hairpin(N):
    """out along +x and back 0.4 m above, the last way-point repeating the first: a car on the way out that drifts upwards
    is globally nearest to a segment of the way back, half a lap from its window"""
    h = (N - 1) // 2
    out = np.stack([0.5 * np.arange(h), np.zeros(h)], axis=1)
    back = np.stack([0.5 * np.arange(N - 1 - h)[::-1] + 0.25, np.full(N - 1 - h, 0.4)], axis=1)
    xy = np.vstack([out, back])
    xy = np.vstack([xy, xy[:1]])
    head = np.arctan2(np.roll(xy[:, 1], -1) - xy[:, 1], np.roll(xy[:, 0], -1) - xy[:, 0])
    return np.concatenate([xy, head[:, None], np.full((N, 1), 2.0)], axis=1)


DYN = np.array([1.0489, 3.74, 0.04712, 0.15875, 0.17145, 4.718, 5.4562, 0.074, 0.1, 3.2, 9.51, 0.4189, 7.0])


def cars_on(wp, B, seed=0, spread=0.3, vlo=0.0, vhi=6.0):
    """B single-track states near the line wp [N,4]: on random segments, `spread` metres off, heading within 0.3 rad"""
    rng = np.random.default_rng(seed + 13 * B)
    N = wp.shape[0]
    j = rng.integers(0, N - 1, B)
    u = rng.uniform(0, 1, B)
    p = wp[j, :2] + u[:, None] * (wp[j + 1, :2] - wp[j, :2]) + rng.normal(size=(B, 2)) * spread
    st = np.zeros((B, 7))
    st[:, :2] = p
    st[:, 2] = rng.uniform(-0.3, 0.3, B)
    st[:, 3] = rng.uniform(vlo, vhi, B)
    st[:, 4] = wp[j, 2] + rng.uniform(-0.3, 0.3, B)
    st[:, 5] = rng.uniform(-0.5, 0.5, B)
    st[:, 6] = rng.uniform(-0.1, 0.1, B)
    return st.astype(np.float32)
