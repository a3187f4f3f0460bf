"""Closed-loop simulation of a net on a race line: plan, apply the first control, move, plan again from where the car went
(the loop of the reference's ``scripts/eval_dnmpc.py`` and gym notebooks, without the gym), for B cars at once and one plant
parameter row per car.  One planning tick is two launches: ``planner.plan_tick(..., rollout=False)`` and
``irbfn_sim_advance`` or ``irbfn_sim_advance_frenet`` (include/irbfn_hip.h states the tick; csrc/sim_advance.hip).  Everything
stays on the device; nothing synchronises with the host until a result is read.

Covered: the Cartesian planner (``IRBFNPlanner.plan``, 7-input nets, ``closed_loop``) and the Frenet planner
(``IRBFNFrenetPlanner.plan``, 8-input nets, ``closed_loop_frenet``: the tick converts the plant state to the Frenet pose on the
polyline, ``to_frenet`` alone).  The plant is the single-track state ``[x, y, delta, v, psi, psi_dot, beta]`` under
``ROLLOUT_ST_SELECT`` or ``ROLLOUT_ST_KS`` in both.  Not covered: a spline frame, laser scans, collisions, an RK4 plant
(DESIGN.md)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from .dynamics import _dyn
from .model import _ptr, _stream_ptr, to_device_f32
from .planner import _check_net, plan_tick

RECORD = ("ticks", "sum_d2", "max_d", "sum_dv", "progress", "s_last", "fail_tick")   # the per-car float64 record


class Track:
    """A race line ``waypoints [N,4]`` = (x, y, heading, speed), float64.  ``wrap``: the line is closed (way-point N - 1 is
    followed by way-point 0).  ``lookahead``: pure-pursuit radius; a car farther than it from the line but within
    ``max_reacquire`` steers for its nearest way-point; ``half_width > 0``: a car farther than it from the line is off the
    track.  ``window = (back, forward)``: segments searched around a car's last nearest segment; ``None``: all of them.
    The arc lengths ``cum`` / ``len`` [N-1] and the line's ``length`` (closing segment included on a wrap track) are computed
    once, in float64, on the host; so is ``curvature`` [N], one value per way-point, by the rule of include/irbfn_hip.h
    (irbfn_cartesian_to_frenet) unless the caller passes its own array."""

    def __init__(self, waypoints, wrap: bool = True, lookahead: float = 1.0, max_reacquire: float = 20.0,
                 half_width: float = 0.0, window=(8, 55), curvature=None):
        wp = np.ascontiguousarray(np.asarray(waypoints.detach().cpu() if hasattr(waypoints, "detach") else waypoints,
                                             dtype=np.float64))
        if wp.ndim != 2 or wp.shape[1] != 4 or wp.shape[0] < 2:
            raise ValueError("waypoints must be [N,4] = (x, y, heading, speed) with N >= 2")
        if window is None:
            window = (-1, -1)
        if len(window) != 2 or any(int(w) != w for w in window):
            raise ValueError("window must be (segments back, segments forward) or None")
        back, fwd = int(window[0]), int(window[1])
        if back < -1 or fwd < -1 or (back == -1) != (fwd == -1):
            raise ValueError("window sides must be >= 0, or both -1 for the whole line")
        if not lookahead >= 0 or not max_reacquire >= 0 or half_width != half_width:
            raise ValueError("lookahead and max_reacquire must be >= 0 and half_width a number")
        self.waypoints = wp
        self.N = wp.shape[0]
        self.wrap = bool(wrap)
        self.lookahead, self.max_reacquire, self.half_width = float(lookahead), float(max_reacquire), float(half_width)
        self.window = (back, fwd)
        d = wp[1:, :2] - wp[:-1, :2]
        self.len = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
        self.cum = np.concatenate([[0.0], np.cumsum(self.len)[:-1]])
        c = wp[0, :2] - wp[-1, :2]
        self.length = float(self.len.sum() + (np.sqrt(c[0] * c[0] + c[1] * c[1]) if self.wrap else 0.0))
        self._dev = None
        if curvature is None:
            curvature = self._curvature(float(np.sqrt(c[0] * c[0] + c[1] * c[1])))
        else:
            curvature = np.ascontiguousarray(np.asarray(curvature.detach().cpu() if hasattr(curvature, "detach") else curvature,
                                                        dtype=np.float64))
            if curvature.shape != (self.N,):
                raise ValueError(f"curvature must be [N] = [{self.N}], one value per way-point")
        self.curvature = curvature
        self._curv_dev = None

    def _curvature(self, closing: float):
        """kappa_i = wrap(theta_{i+1} - theta_{i-1}) / (len_{i-1} + len_i); the ends across the seam on a wrap track, else
        one-sided.  A repeated way-point divides by zero: inf or NaN there, as the rule says."""
        th, ln, N = self.waypoints[:, 2], self.len, self.N
        k = np.empty(N)
        with np.errstate(divide="ignore", invalid="ignore"):
            k[1:-1] = wrap_angle(th[2:] - th[:-2]) / (ln[:-1] + ln[1:])
            if self.wrap:
                k[0] = wrap_angle(th[1] - th[N - 1]) / (closing + ln[0])
                k[N - 1] = wrap_angle(th[0] - th[N - 2]) / (ln[N - 2] + closing)
            else:
                k[0] = wrap_angle(th[1] - th[0]) / ln[0]
                k[N - 1] = wrap_angle(th[N - 1] - th[N - 2]) / ln[N - 2]
        return k

    def curvature_device(self, torch):
        """-> curvature [N] float64 on the current device, made once per device"""
        dev = torch.device("cuda", torch.cuda.current_device())
        if self._curv_dev is None or self._curv_dev.device != dev:
            self._curv_dev = torch.from_numpy(self.curvature).to(dev)
        return self._curv_dev

    def pose_at(self, s, ey=0.0, epsi=0.0):
        """-> (x, y, psi), host float64: the point at arc length ``s`` of the polyline (clipped to its N - 1 segments), ``ey`` to
        the left of its segment, heading ``epsi`` off the line's interpolated heading.  The inverse of the Frenet pose away from
        the vertices; seeds cars at lateral and heading offsets."""
        s, ey, epsi = np.broadcast_arrays(np.asarray(s, np.float64), np.asarray(ey, np.float64), np.asarray(epsi, np.float64))
        wp, ln, cum = self.waypoints, self.len, self.cum
        i = np.clip(np.searchsorted(cum, s, side="right") - 1, 0, self.N - 2)
        t = np.clip((s - cum[i]) / ln[i], 0.0, 1.0)
        dx, dy = wp[i + 1, 0] - wp[i, 0], wp[i + 1, 1] - wp[i, 1]
        x = wp[i, 0] + t * dx - ey * dy / ln[i]
        y = wp[i, 1] + t * dy + ey * dx / ln[i]
        psi = wp[i, 2] + t * wrap_angle(wp[i + 1, 2] - wp[i, 2]) + epsi
        return x, y, psi

    def device(self, torch):
        """-> (waypoints [N,4], xy [N,2], cum, len) float64 tensors on the current device, made once per device"""
        dev = torch.device("cuda", torch.cuda.current_device())
        if self._dev is None or self._dev[0].device != dev:
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            self._dev = (up(self.waypoints), up(self.waypoints[:, :2]), up(self.cum), up(self.len))
        return self._dev

    def struct(self, torch) -> _lib.SimTrack:
        wp, _, cum, ln = self.device(torch)
        return _lib.SimTrack(wp.data_ptr(), cum.data_ptr(), ln.data_ptr(), self.length, self.lookahead, self.max_reacquire,
                             self.half_width, self.N, int(self.wrap), self.window[0], self.window[1])

    def seed(self, xy):
        """nearest segment [B] int32 of the points xy [B,2] over the whole line: one ``nearest_point`` call"""
        from .planner_utils import nearest_point
        torch = _lib.require_gpu()
        return nearest_point(xy, self.device(torch)[1])[3]


def wrap_angle(e):
    """e - 2 pi rint(e / 2 pi), float64"""
    return e - 2.0 * np.pi * np.rint(e / (2.0 * np.pi))


def new_record(B: int, torch, device=None):
    """the record [B, len(RECORD)] of cars that have not moved: zeros, fail_tick = -1"""
    rec = torch.zeros((B, len(RECORD)), dtype=torch.float64, device=device or torch.device("cuda", torch.cuda.current_device()))
    rec[:, RECORD.index("fail_tick")] = -1.0
    return rec


def _advance(frenet: bool, track, state, seg, status, record, x, mirror, controls, plant_params, n_sub, mode, tick, frenet_out,
             goal_out, dist_out, t_out):
    """``advance`` (frenet false: x [B,7], no frenet_out) and ``advance_frenet`` (x [B,8])"""
    torch = _lib.require_gpu()
    lib = _lib.load()
    B = state.shape[0]
    want = {"state": (state, (B, 7), torch.float32), "seg": (seg, (B,), torch.int32), "status": (status, (B,), torch.int32),
            "record": (record, (B, len(RECORD)), torch.float64), "x": (x, (B, 8 if frenet else 7), torch.float32),
            "mirror": (mirror, (B,), torch.int32), "frenet_out": (frenet_out, (B, 8), torch.float64),
            "goal_out": (goal_out, (B, 4), torch.float64), "dist_out": (dist_out, (B,), torch.float64),
            "t_out": (t_out, (B,), torch.float64)}
    for name, (t, shape, dtype) in want.items():
        if t is None and name.endswith("_out"):
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda or tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous device tensor {list(shape)} of {dtype}")
    null = C.c_void_p(None)
    opt = lambda t: _ptr(t) if t is not None else null
    T, keep, host, dev = 0, None, null, None
    if controls is not None:
        if (not isinstance(controls, torch.Tensor) or not controls.is_cuda or controls.dim() != 2 or controls.shape[0] != B
                or controls.shape[1] % 2 or controls.shape[1] < 2 or controls.dtype != torch.float32 or not controls.is_contiguous()):
            raise ValueError("controls must be a contiguous float32 device tensor [B, 2T]")
        T = controls.shape[1] // 2
        if isinstance(plant_params, torch.Tensor) and plant_params.dim() == 2:
            dev = to_device_f32(plant_params, torch)
            if tuple(dev.shape) != (B, 13):
                raise ValueError("per-car plant_params must be [B, 13]")
        else:
            keep, host = _dyn(plant_params)
            if keep is None:
                raise ValueError("a plant step needs plant_params")
    tr = track.struct(torch)
    if frenet:
        st = lib.irbfn_sim_advance_frenet(C.byref(tr), _ptr(track.curvature_device(torch)), int(mode), int(tick), opt(controls),
                                          T, host, opt(dev), int(n_sub), _ptr(state), _ptr(seg), _ptr(status), _ptr(record),
                                          _ptr(x), _ptr(mirror), opt(frenet_out), opt(goal_out), opt(dist_out), opt(t_out), B,
                                          _stream_ptr(torch))
        _lib.check(st, "irbfn_sim_advance_frenet")
        return
    st = lib.irbfn_sim_advance(C.byref(tr), int(mode), int(tick), opt(controls), T, host, opt(dev), int(n_sub), _ptr(state),
                               _ptr(seg), _ptr(status), _ptr(record), _ptr(x), _ptr(mirror), opt(goal_out), opt(dist_out),
                               opt(t_out), B, _stream_ptr(torch))
    _lib.check(st, "irbfn_sim_advance")


def advance(track: Track, state, seg, status, record, x, mirror, controls=None, plant_params=None, n_sub: int = 1,
            mode: int = _lib.ROLLOUT_ST_SELECT, tick: int = 0, goal_out=None, dist_out=None, t_out=None):
    """One ``irbfn_sim_advance`` on device tensors, all updated in place: state [B,7] f32, seg / status [B] i32, record
    [B,7] f64, x [B,7] f32, mirror [B] i32.  ``controls`` [B,2T] f32 (None: no plant step, the call that prepares tick 0);
    ``plant_params``: 13 numbers on the host, or a float32 device tensor [B,13] with one row per car.  Optional outputs
    goal_out [B,4], dist_out [B], t_out [B] (float64)."""
    _advance(False, track, state, seg, status, record, x, mirror, controls, plant_params, n_sub, mode, tick, None, goal_out,
             dist_out, t_out)


def advance_frenet(track: Track, state, seg, status, record, x, mirror, controls=None, plant_params=None, n_sub: int = 1,
                   mode: int = _lib.ROLLOUT_ST_SELECT, tick: int = 0, frenet_out=None, goal_out=None, dist_out=None, t_out=None):
    """One ``irbfn_sim_advance_frenet``: ``advance`` with the Frenet planner's query, x [B,8] f32, and the optional output
    frenet_out [B,8] f64 = [s, ey, delta, vx, vy, wz, epsi, curv] of the cars that drive on."""
    if not isinstance(track, Track):
        raise TypeError(f"track must be a simulate.Track, not {type(track).__name__}")
    _advance(True, track, state, seg, status, record, x, mirror, controls, plant_params, n_sub, mode, tick, frenet_out, goal_out,
             dist_out, t_out)


def to_frenet(track: Track, state, seg=None):
    """Frenet poses of single-track states [B,7] on ``track`` (``irbfn_cartesian_to_frenet``) -> (frenet [B,8] f64 = [s, ey,
    delta, vx, vy, wz, epsi, curv], seg [B] i32, dist [B] f64).  ``seg`` [B] int32: search the track's window around it, as a
    tick does; None: every segment."""
    if not isinstance(track, Track):
        raise TypeError(f"track must be a simulate.Track, not {type(track).__name__}")
    shape = tuple(state.shape) if hasattr(state, "shape") else np.asarray(state).shape
    if len(shape) != 2 or shape[1] != 7:
        raise ValueError("state must be [B,7] = [x, y, delta, v, psi, psi_dot, beta]")
    B = shape[0]
    if seg is not None and tuple(seg.shape) != (B,):
        raise ValueError("seg must be [B]")
    torch = _lib.require_gpu()
    lib = _lib.load()
    sd = to_device_f32(state, torch)
    null = C.c_void_p(None)
    if seg is not None:
        seg = (seg if isinstance(seg, torch.Tensor) else torch.as_tensor(np.asarray(seg))).to(device=sd.device, dtype=torch.int32).contiguous()
    frenet = torch.empty((B, 8), dtype=torch.float64, device=sd.device)
    seg_out = torch.empty((B,), dtype=torch.int32, device=sd.device)
    dist = torch.empty((B,), dtype=torch.float64, device=sd.device)
    tr = track.struct(torch)
    st = lib.irbfn_cartesian_to_frenet(C.byref(tr), _ptr(track.curvature_device(torch)), _ptr(sd),
                                       _ptr(seg) if seg is not None else null, _ptr(frenet), _ptr(seg_out), _ptr(dist), null, B,
                                       _stream_ptr(torch))
    _lib.check(st, "irbfn_cartesian_to_frenet")
    return frenet, seg_out, dist


@dataclass
class SimResult:
    """Per-car results of ``closed_loop`` (device tensors [B]).  ``ticks``: calls that reached the way-point search (the one
    that prepared tick 0 included); ``fail_tick``: plant steps taken when the car stopped, -1 for a car still driving;
    ``rms_dev`` / ``max_dev``: distance from the line; ``mean_abs_dv``: |speed - the line's speed at the nearest segment|;
    ``progress``: arc length covered along the line; ``laps`` = progress / the line's length.  ``states``
    [ticks // record_every, B, 7] where asked for."""
    status: object
    fail_tick: object
    ticks: object
    rms_dev: object
    max_dev: object
    mean_abs_dv: object
    progress: object
    laps: object
    state: object
    states: object = None

    def summary(self, quantiles=(0.0, 0.5, 0.9, 1.0)) -> dict:
        """counts per status and quantiles over the cars of each figure: plain torch ops, read back here"""
        import torch
        out = {"cars": int(self.status.numel()),
               "status": {name: int((self.status == code).sum()) for code, name in _lib.SIM_STATUS_NAMES.items()}}
        q = torch.tensor(list(quantiles), dtype=torch.float64, device=self.status.device)
        for name in ("rms_dev", "max_dev", "mean_abs_dv", "progress", "laps"):
            v = getattr(self, name)
            v = v[torch.isfinite(v)]
            out[name] = [float(t) for t in torch.quantile(v, q)] if v.numel() else []
        return out


def _plant(plant_params, dyn_params, B):
    """-> ("host", 13 floats) or ("dev", [B,13] array-like), shapes checked without a GPU"""
    p = dyn_params if plant_params is None else plant_params
    if p is None:
        raise ValueError("closed_loop needs dyn_params or plant_params: 13 entries (dynamics.py:24-36)")
    shape = tuple(p.shape) if hasattr(p, "shape") else np.asarray(p).shape
    if shape == (13,):
        return "host", p
    if shape == (B, 13):
        return "dev", p
    raise ValueError(f"plant_params must be [13] or [B, 13] = [{B}, 13], not {list(shape)}")


def _closed_loop(frenet: bool, net, params, track, state0, ticks, dyn_params, plant_params, n_sub, mode, record_every):
    """``closed_loop`` (frenet false) and ``closed_loop_frenet``: the checks, the arrays and the loop"""
    _check_net(net)
    if not isinstance(track, Track):
        raise TypeError(f"track must be a simulate.Track, not {type(track).__name__}")
    if mode not in (_lib.ROLLOUT_ST_SELECT, _lib.ROLLOUT_ST_KS):
        raise ValueError("the plant is ROLLOUT_ST_SELECT or ROLLOUT_ST_KS")
    if int(ticks) != ticks or ticks < 0 or int(n_sub) != n_sub or n_sub < 1 or int(record_every) != record_every or record_every < 0:
        raise ValueError("ticks >= 0, n_sub >= 1 and record_every >= 0 must be integers")
    shape = tuple(state0.shape) if hasattr(state0, "shape") else np.asarray(state0).shape
    if len(shape) != 2 or shape[1] != 7:
        raise ValueError("state0 must be [B,7] = [x, y, delta, v, psi, psi_dot, beta]")
    D = 8 if frenet else 7
    if net.in_features != D or net.out_features % 2 or net.out_features < 2:
        raise ValueError(f"the {'Frenet' if frenet else 'Cartesian'} planner's net has {D} inputs and 2T outputs")
    B = shape[0]
    kind, plant = _plant(plant_params, dyn_params, B)
    torch = _lib.require_gpu()
    state = to_device_f32(state0, torch).clone()
    dev = state.device
    if kind == "dev":
        plant = to_device_f32(plant, torch)
    seg = track.seed(state[:, :2].to(torch.float64)).contiguous()
    status = torch.zeros((B,), dtype=torch.int32, device=dev)
    record = new_record(B, torch, dev)
    x = torch.zeros((B, D), dtype=torch.float32, device=dev)
    mirror = torch.zeros((B,), dtype=torch.int32, device=dev)
    states = torch.empty((ticks // record_every, B, 7), dtype=torch.float32, device=dev) if record_every else None
    step = advance_frenet if frenet else advance
    step(track, state, seg, status, record, x, mirror, mode=mode, tick=0)
    for k in range(int(ticks)):
        ctrl, _ = plan_tick(net, params, x, mirror, rollout=False, mode=mode)
        step(track, state, seg, status, record, x, mirror, controls=ctrl, plant_params=plant, n_sub=n_sub, mode=mode, tick=k + 1)
        if record_every and (k + 1) % record_every == 0:
            states[(k + 1) // record_every - 1].copy_(state)
    col = lambda name: record[:, RECORD.index(name)]
    n = col("ticks")
    return SimResult(status=status, fail_tick=col("fail_tick").to(torch.int64), ticks=n.to(torch.int64),
                     rms_dev=torch.sqrt(col("sum_d2") / n), max_dev=col("max_d").clone(), mean_abs_dv=col("sum_dv") / n,
                     progress=col("progress").clone(), laps=col("progress") / track.length, state=state, states=states)


def closed_loop(net, params: dict, track: Track, state0, ticks: int, dyn_params=None, plant_params=None, n_sub: int = 1,
                mode: int = _lib.ROLLOUT_ST_SELECT, record_every: int = 0) -> SimResult:
    """Drives B cars from ``state0 [B,7]`` along ``track`` for ``ticks`` planning ticks: query -> ``plan_tick`` -> first control
    -> ``n_sub`` plant steps of ``dt / n_sub`` -> way-point search -> next query.  ``dyn_params``: the 13 parameters of the
    model; ``plant_params`` ([13] or [B,13], default ``dyn_params``): those of the plant each car drives on.  net: a WCRBFNet, a
    DeeperWCRBFNet or a ClusterWCRBFNet with 7 inputs (any other type raises TypeError).  ``record_every = k > 0``: keep the
    states after ticks k, 2k, ..."""
    return _closed_loop(False, net, params, track, state0, ticks, dyn_params, plant_params, n_sub, mode, record_every)


def closed_loop_frenet(net, params: dict, track: Track, state0, ticks: int, dyn_params=None, plant_params=None, n_sub: int = 1,
                       mode: int = _lib.ROLLOUT_ST_SELECT, record_every: int = 0) -> SimResult:
    """``closed_loop`` for the Frenet planner's nets: 8 inputs ``[ey, delta, vx, vy, vx_goal, wz, epsi, curv]`` and 2T outputs
    (the 12-region golden net has T = 1).  ``state0`` is still the single-track ``[B,7]`` and the plant Cartesian; each tick
    takes the car's Frenet pose on the polyline (``track.curvature``; include/irbfn_hip.h: irbfn_sim_advance_frenet) and the
    goal way-point's speed as ``vx_goal``.  ``Track.pose_at`` seeds cars at lateral and heading offsets."""
    return _closed_loop(True, net, params, track, state0, ticks, dyn_params, plant_params, n_sub, mode, record_every)
