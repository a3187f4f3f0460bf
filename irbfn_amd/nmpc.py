"""Batched NMPC solver on the device (``irbfn_nmpc_solve``, csrc/nmpc_solve.hip, K13): for B independent (state, goal) pairs
the control sequence that minimises a tracking cost through the project's own roll-out model under the control bounds -- a
projected Levenberg-Marquardt, one problem per GPU lane (include/irbfn_hip.h states the rule; DESIGN.md "K13").

It closes the two open ends of the pipeline: ``make_table`` writes a label table in the reference's ``.npz`` layout (the
reference's labels come from CasADi / IPOPT solvers, which this project cannot run), and ``closed_loop`` drives the cars of
``simulate.closed_loop`` with the solver instead of a net -- the controller a net imitates, on the same line and plant.

``solve_frenet`` (``irbfn_nmpc_solve_frenet``, K15) is the same solver through the Frenet low-speed model: the controller the
Frenet planner's 8-input nets imitate.  ``make_table_frenet`` writes their label tables, ``closed_loop_frenet`` drives the cars
of ``simulate.closed_loop_frenet`` with it.

Weights, tolerances and damping constants are this project's own; the reference's are not readable here.
Everything stays on the device; nothing synchronises with the host until a result is read."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _lib, tables
from .dynamics import _dyn
from .model import _ptr, _stream_ptr, to_device_f32
from . import simulate

T_MAX = 8


@dataclass(frozen=True)
class Weights:
    """cost = 1/2 [sum_{t<T} q . e_t^2 + qf . e_T^2 + sum r . u_t^2 + sum rd . (u_{t+1} - u_t)^2]; e = (x, y, heading, speed)
    errors, u = (a, sv).  The defaults are this project's own."""
    q: Sequence[float] = (1.0, 1.0, 0.5, 0.1)
    qf: Sequence[float] = (10.0, 10.0, 5.0, 1.0)
    r: Sequence[float] = (0.01, 0.1)
    rd: Sequence[float] = (0.01, 0.1)


@dataclass(frozen=True)
class FrenetWeights(Weights):
    """``Weights`` for ``solve_frenet``: e = (s, ey, heading error, vx) errors.  The defaults are this project's own: the lateral,
    heading and speed weights of ``Weights``, and none on s -- progress along the line is free."""
    q: Sequence[float] = (0.0, 1.0, 0.5, 0.1)
    qf: Sequence[float] = (0.0, 10.0, 5.0, 1.0)


@dataclass
class NMPCResult:
    """Device tensors: controls [B,2T] f32 = [a_0..a_{T-1}, sv_0..sv_{T-1}]; cost0 / cost [B] f32 (clipped start / result);
    status [B] i32 (``_lib.NMPC_STATUS_NAMES``); iterations [B] i32; grad [B,2T] f32 = J^T r at ``controls`` where asked for."""
    controls: object
    cost0: object
    cost: object
    status: object
    iterations: object
    grad: object = None


def _shape(a):
    return tuple(a.shape) if hasattr(a, "shape") else np.asarray(a).shape


def _options(weights, max_iter, lambda0, lambda_min, lambda_max, tol, eps) -> _lib.NmpcOptions:
    """the options struct, every range checked here (no GPU needed)"""
    if not isinstance(weights, Weights):
        raise TypeError(f"weights must be nmpc.Weights, not {type(weights).__name__}")
    o = _lib.NmpcOptions()
    for name, n in (("q", 4), ("qf", 4), ("r", 2), ("rd", 2)):
        v = [float(c) for c in getattr(weights, name)]
        if len(v) != n or any(not (c >= 0.0 and math.isfinite(c)) for c in v):
            raise ValueError(f"weights.{name} must be {n} finite numbers >= 0")
        setattr(o, name, (C.c_float * n)(*v))
    if int(max_iter) != max_iter or max_iter < 0:
        raise ValueError("max_iter must be an integer >= 0")
    for name, v in (("lambda0", lambda0), ("lambda_min", lambda_min), ("lambda_max", lambda_max), ("tol", tol), ("eps", eps)):
        if not (v >= 0.0 and math.isfinite(v)):
            raise ValueError(f"{name} must be a finite number >= 0")
        setattr(o, name, float(v))
    if lambda_min > lambda_max:
        raise ValueError("lambda_min must not exceed lambda_max")
    o.max_iter = int(max_iter)
    return o


_STATE = {False: (7, "[x, y, delta, v, psi, psi_dot, beta]", "(x, y, heading, speed)"),
          True: (8, "[s, ey, delta, vx, vy, wz, epsi, curv]", "(s, ey, heading error, vx)")}


def _check_problem(state0, goal, u0, dyn_params, T, mode, frenet=False):
    """shapes and ranges of one solve, checked without a GPU -> (B, "host" | "dev").  ``frenet``: the Frenet model's state row
    (there is no mode to choose)."""
    if int(T) != T or not 1 <= T <= T_MAX:
        raise ValueError(f"the horizon T must be an integer in 1..{T_MAX}")
    if not frenet and mode not in (_lib.ROLLOUT_ST_SELECT, _lib.ROLLOUT_ST_KS):
        raise ValueError("the model is ROLLOUT_ST_SELECT or ROLLOUT_ST_KS")
    width, names, errors = _STATE[bool(frenet)]
    s = _shape(state0)
    if len(s) != 2 or s[1] != width:
        raise ValueError(f"state0 must be [B,{width}] = {names}")
    B = s[0]
    if _shape(goal) != (B, 4):
        raise ValueError(f"goal must be [B,4] = [{B}, 4] = {errors}")
    if u0 is not None and _shape(u0) != (B, 2 * T):
        raise ValueError(f"u0 must be [B,2T] = [{B}, {2 * T}]")
    if dyn_params is None:
        raise ValueError("solve needs dyn_params: 13 entries (dynamics.py:24-36)")
    d = _shape(dyn_params)
    if d == (13,):
        return B, "host"
    if d == (B, 13):
        return B, "dev"
    raise ValueError(f"dyn_params must be [13] or [B, 13] = [{B}, 13], not {list(d)}")


def solve(state0, goal, dyn_params, T: int = 5, weights: Weights = Weights(), u0=None, mode: int = _lib.ROLLOUT_ST_KS,
          max_iter: int = 30, lambda0: float = 1e-3, lambda_min: float = 1e-9, lambda_max: float = 1e6, tol: float = 1e-6,
          eps: float = 1e-6, want_grad: bool = False) -> NMPCResult:
    """One ``irbfn_nmpc_solve``: state0 [B,7], goal [B,4], ``dyn_params`` 13 numbers or a [B,13] tensor (one row per problem),
    start ``u0`` [B,2T] (None: zeros).  ``max_iter = 0`` evaluates cost and gradient at the clipped start."""
    return _solve(False, state0, goal, dyn_params, T, weights, u0, mode, max_iter, lambda0, lambda_min, lambda_max, tol, eps,
                  want_grad)


def solve_frenet(state0, goal, dyn_params, T: int = 5, weights: Weights = FrenetWeights(), u0=None, max_iter: int = 30,
                 lambda0: float = 1e-3, lambda_min: float = 1e-9, lambda_max: float = 1e6, tol: float = 1e-6, eps: float = 1e-6,
                 want_grad: bool = False) -> NMPCResult:
    """One ``irbfn_nmpc_solve_frenet``: ``solve`` through the Frenet low-speed model.  state0 [B,8] = [s, ey, delta, vx, vy, wz,
    epsi, curv], goal [B,4] = (s, ey, heading error, vx).  A row that starts outside the frame (1 - ey curv <= 0) comes back
    ``NMPC_NONFINITE``."""
    return _solve(True, state0, goal, dyn_params, T, weights, u0, None, max_iter, lambda0, lambda_min, lambda_max, tol, eps,
                  want_grad)


def _solve(frenet, state0, goal, dyn_params, T, weights, u0, mode, max_iter, lambda0, lambda_min, lambda_max, tol, eps, want_grad):
    """``solve`` (frenet false) and ``solve_frenet``: the checks, the buffers and the call"""
    B, kind = _check_problem(state0, goal, u0, dyn_params, T, mode, frenet)
    opt = _options(weights, max_iter, lambda0, lambda_min, lambda_max, tol, eps)
    torch = _lib.require_gpu()
    lib = _lib.load()
    sd, gd = to_device_f32(state0, torch), to_device_f32(goal, torch)
    ud = to_device_f32(u0, torch) if u0 is not None else None
    null = C.c_void_p(None)
    keep, host, dev = None, null, None
    if kind == "dev":
        dev = to_device_f32(dyn_params, torch)
    else:
        keep, host = _dyn(dyn_params)
    u = torch.empty((B, 2 * T), dtype=torch.float32, device=sd.device)
    cost = torch.empty((B, 2), dtype=torch.float32, device=sd.device)
    info = torch.empty((B, 2), dtype=torch.int32, device=sd.device)
    grad = torch.empty((B, 2 * T), dtype=torch.float32, device=sd.device) if want_grad else None
    opt_p = lambda t: _ptr(t) if t is not None else null
    rest = (int(T), _ptr(sd), _ptr(gd), opt_p(ud), host, opt_p(dev), C.byref(opt), _ptr(u), _ptr(cost), _ptr(info), opt_p(grad), B,
            _stream_ptr(torch))
    if frenet:
        _lib.check(lib.irbfn_nmpc_solve_frenet(*rest), "irbfn_nmpc_solve_frenet")
    else:
        _lib.check(lib.irbfn_nmpc_solve(int(mode), *rest), "irbfn_nmpc_solve")
    return NMPCResult(controls=u, cost0=cost[:, 0], cost=cost[:, 1], status=info[:, 0], iterations=info[:, 1], grad=grad)


def query_problem(x):
    """The planner's query ``[v, x_g, y_g, theta_g, v_g, beta, psi_dot]`` [B,7] (planner_geom.h) -> (state0 [B,7], goal [B,4]):
    state0 = [0, 0, 0, v, 0, psi_dot, beta] (the training convention, train_nmpc.py:260-266), goal = (x_g, y_g, theta_g, v_g).
    NumPy in, NumPy out; tensor in, tensor out."""
    if len(_shape(x)) != 2 or _shape(x)[1] != 7:
        raise ValueError("queries must be [B,7] = [v, x_g, y_g, theta_g, v_g, beta, psi_dot]")
    if hasattr(x, "new_zeros"):
        state0 = x.new_zeros(x.shape)
        goal = x[:, 1:5].contiguous()
    else:
        x = np.asarray(x)
        state0 = np.zeros_like(x)
        goal = np.ascontiguousarray(x[:, 1:5])
    state0[:, 3] = x[:, 0]
    state0[:, 5] = x[:, 6]
    state0[:, 6] = x[:, 5]
    return state0, goal


def solve_queries(x, dyn_params, T: int = 5, **kw) -> NMPCResult:
    """``solve`` on planner queries x [B,7] (``query_problem``)."""
    state0, goal = query_problem(x)
    return solve(state0, goal, dyn_params, T=T, **kw)


def frenet_query_problem(x):
    """The Frenet planner's query ``[ey, delta, vx, vy, vx_goal, wz, epsi, curv]`` [B,8] (planner_geom.h) -> (state0 [B,8], goal
    [B,4]): state0 = [0, ey, delta, vx, vy, wz, epsi, curv], goal = (0, 0, 0, vx_goal).  The query is taken literally: mirroring it
    is the planner's business, not the table's.  NumPy in, NumPy out; tensor in, tensor out."""
    if len(_shape(x)) != 2 or _shape(x)[1] != 8:
        raise ValueError("queries must be [B,8] = [ey, delta, vx, vy, vx_goal, wz, epsi, curv]")
    if hasattr(x, "new_zeros"):
        state0 = x.new_zeros(x.shape)
        goal = x.new_zeros((x.shape[0], 4))
    else:
        x = np.asarray(x)
        state0 = np.zeros_like(x)
        goal = np.zeros((x.shape[0], 4), x.dtype)
    state0[:, 1:4] = x[:, 0:3]
    state0[:, 4] = x[:, 3]
    state0[:, 5:8] = x[:, 5:8]
    goal[:, 3] = x[:, 4]
    return state0, goal


def solve_queries_frenet(x, dyn_params, T: int = 5, **kw) -> NMPCResult:
    """``solve_frenet`` on Frenet planner queries x [B,8] (``frenet_query_problem``)."""
    state0, goal = frenet_query_problem(x)
    return solve_frenet(state0, goal, dyn_params, T=T, **kw)


def make_table(x, dyn_params, T: int = 5, save: Optional[str] = None, **kw):
    """Label table of the queries x [N,7]: -> (inputs [N,7], outputs [N,T,2]) NumPy float32, the reference's ``.npz`` layout
    (tables.py).  A row whose solve did not converge holds ``tables.INFEASIBLE`` in every output, so
    ``tables.remove_infeasible`` drops it; ``tables.flatten_outputs`` / ``tables.mirror`` apply unchanged.  ``save``: also
    written there with ``np.savez`` (keys ``inputs``, ``outputs``)."""
    return _table(solve_queries(x, dyn_params, T=T, **kw), x, save)


def make_table_frenet(x, dyn_params, T: int = 5, save: Optional[str] = None, **kw):
    """``make_table`` for the Frenet planner's nets: queries x [N,8] -> (inputs [N,8], outputs [N,T,2]), the same layout and the
    same ``tables.INFEASIBLE`` fill of the rows that did not converge, labels from ``solve_queries_frenet``."""
    return _table(solve_queries_frenet(x, dyn_params, T=T, **kw), x, save)


def _table(res, x, save):
    u = res.controls.cpu().numpy()
    ok = res.status.cpu().numpy() == _lib.NMPC_CONVERGED
    inputs = np.ascontiguousarray(np.asarray(x.detach().cpu() if hasattr(x, "detach") else x, dtype=np.float32))
    outputs = fill_infeasible(u, ok)
    if save is not None:
        np.savez(save, inputs=inputs, outputs=outputs)
    return inputs, outputs


def fill_infeasible(u, ok):
    """controls [N,2T] and a row mask -> outputs [N,T,2] = (a, sv) per step, rows outside the mask all ``tables.INFEASIBLE``"""
    u = np.asarray(u, dtype=np.float32)
    T = u.shape[1] // 2
    outputs = np.stack([u[:, :T], u[:, T:]], axis=-1)
    outputs[~np.asarray(ok, dtype=bool)] = tables.INFEASIBLE
    return outputs


def shift_controls(u, T: int):
    """warm start of the next tick: every control moves one step forward, the last one repeats (plain torch ops)"""
    import torch
    return torch.cat([u[:, 1:T], u[:, T - 1:T], u[:, T + 1:], u[:, 2 * T - 1:]], dim=1).contiguous()


_LOOP_SOLVE_KW = ("weights", "max_iter", "lambda0", "lambda_min", "lambda_max", "tol", "eps")


def closed_loop(track, state0, ticks: int, dyn_params, plant_params=None, T: int = 5, n_sub: int = 1,
                mode: int = _lib.ROLLOUT_ST_SELECT, record_every: int = 0, **kw) -> simulate.SimResult:
    """``simulate.closed_loop`` with the solver in the net's place: per tick one ``simulate.advance`` (plant, way-point search,
    goal) and one ``solve`` on the car's world-frame state and goal, warm-started from the previous solution shifted by one
    step.  ``dyn_params`` ([13]): the solver's model; ``plant_params`` ([13] or [B,13], default ``dyn_params``): the plant each
    car drives on.  Same statistics and status words as ``simulate.closed_loop``.  A frozen car is solved like any other row
    and ignored by ``advance``.  Further keywords go to ``solve``: its weights and iteration constants (the start and the
    gradient are the loop's own business)."""
    return _closed_loop(False, track, state0, ticks, dyn_params, plant_params, T, n_sub, mode, record_every, kw)


def closed_loop_frenet(track, state0, ticks: int, dyn_params, plant_params=None, T: int = 5, n_sub: int = 1,
                       mode: int = _lib.ROLLOUT_ST_SELECT, record_every: int = 0, **kw) -> simulate.SimResult:
    """``closed_loop`` with ``solve_frenet``: per tick one ``simulate.advance_frenet`` (plant, way-point search, Frenet pose on
    the polyline, goal) and one ``solve_frenet`` on the float32 pose with s = 0 and the goal (0, 0, 0, the goal way-point's
    speed) -- back onto the line at the line's speed -- warm-started in the same way.  ``state0`` is still the single-track
    [B,7]; ``mode`` and ``plant_params`` describe the Cartesian plant, ``dyn_params`` the solver's Frenet model.  Further keywords
    go to ``solve_frenet`` (default weights: ``FrenetWeights``)."""
    return _closed_loop(True, track, state0, ticks, dyn_params, plant_params, T, n_sub, mode, record_every, kw)


def _frenet_tick_problem(pose, goal):
    """what ``closed_loop_frenet`` solves each tick, from the outputs of ``simulate.advance_frenet`` (float64 device tensors pose
    [B,8], goal [B,4]) -> (state0 [B,8], goal [B,4]) float32: the pose with s = 0, and (0, 0, 0, the goal way-point's speed)"""
    import torch
    state0 = pose.to(torch.float32)
    state0[:, 0] = 0.0
    g = torch.zeros((pose.shape[0], 4), dtype=torch.float32, device=pose.device)
    g[:, 3] = goal[:, 3].to(torch.float32)
    return state0, g


def _closed_loop(frenet, track, state0, ticks, dyn_params, plant_params, T, n_sub, mode, record_every, kw):
    """``closed_loop`` (frenet false) and ``closed_loop_frenet``: the checks, the arrays, the loop and the result"""
    name = "closed_loop_frenet" if frenet else "closed_loop"
    if not isinstance(track, simulate.Track):
        raise TypeError(f"track must be a simulate.Track, not {type(track).__name__}")
    extra = sorted(set(kw) - set(_LOOP_SOLVE_KW))
    if extra:
        raise TypeError(f"{name} passes only {', '.join(_LOOP_SOLVE_KW)} on to solve, not {', '.join(extra)}")
    if int(ticks) != ticks or ticks < 0 or int(n_sub) != n_sub or n_sub < 1 or int(record_every) != record_every or record_every < 0:
        raise ValueError("ticks >= 0, n_sub >= 1 and record_every >= 0 must be integers")
    shape = _shape(state0)
    if len(shape) != 2 or shape[1] != 7:
        raise ValueError("state0 must be [B,7] = [x, y, delta, v, psi, psi_dot, beta]")
    B = shape[0]
    if frenet and mode not in (_lib.ROLLOUT_ST_SELECT, _lib.ROLLOUT_ST_KS):
        raise ValueError("the plant's model is ROLLOUT_ST_SELECT or ROLLOUT_ST_KS")
    _check_problem(np.empty((B, 8 if frenet else 7)), np.empty((B, 4)), None, dyn_params, T, mode, frenet)
    _options(kw.get("weights", FrenetWeights() if frenet else Weights()), kw.get("max_iter", 30), kw.get("lambda0", 1e-3),
             kw.get("lambda_min", 1e-9), kw.get("lambda_max", 1e6), kw.get("tol", 1e-6), kw.get("eps", 1e-6))
    kind, plant = simulate._plant(plant_params, dyn_params, B)
    torch = _lib.require_gpu()
    state = to_device_f32(state0, torch).clone()
    dev = state.device
    if kind == "dev":
        plant = to_device_f32(plant, torch)
    seg = track.seed(state[:, :2].to(torch.float64)).contiguous()
    status = torch.zeros((B,), dtype=torch.int32, device=dev)
    record = simulate.new_record(B, torch, dev)
    x = torch.zeros((B, 8 if frenet else 7), dtype=torch.float32, device=dev)
    mirror = torch.zeros((B,), dtype=torch.int32, device=dev)
    goal = torch.zeros((B, 4), dtype=torch.float64, device=dev)
    states = torch.empty((ticks // record_every, B, 7), dtype=torch.float32, device=dev) if record_every else None
    if frenet:
        pose = torch.zeros((B, 8), dtype=torch.float64, device=dev)
        advance = lambda **a: simulate.advance_frenet(track, state, seg, status, record, x, mirror, mode=mode, frenet_out=pose,
                                                      goal_out=goal, **a)
        control = lambda warm: solve_frenet(*_frenet_tick_problem(pose, goal), dyn_params, T=T, u0=warm, **kw).controls
    else:
        advance = lambda **a: simulate.advance(track, state, seg, status, record, x, mirror, mode=mode, goal_out=goal, **a)
        control = lambda warm: solve(state, goal.to(torch.float32), dyn_params, T=T, u0=warm, mode=mode, **kw).controls
    advance(tick=0)
    warm = None
    for k in range(int(ticks)):
        ctrl = control(warm)
        advance(controls=ctrl, plant_params=plant, n_sub=n_sub, tick=k + 1)
        warm = shift_controls(ctrl, T)
        if record_every and (k + 1) % record_every == 0:
            states[(k + 1) // record_every - 1].copy_(state)
    col = lambda name: record[:, simulate.RECORD.index(name)]
    n = col("ticks")
    return simulate.SimResult(status=status, fail_tick=col("fail_tick").to(torch.int64), ticks=n.to(torch.int64),
                              rms_dev=torch.sqrt(col("sum_d2") / n), max_dev=col("max_d").clone(),
                              mean_abs_dv=col("sum_dv") / n, progress=col("progress").clone(),
                              laps=col("progress") / track.length, state=state, states=states)
