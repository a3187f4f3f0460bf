"""The statements behind the Frenet NMPC solver (irbfn_amd/csrc/nmpc_solve.hip, K15; include/irbfn_hip.h: irbfn_nmpc_solve_frenet),
shared by test_nmpc_frenet_cpu.py (which holds them to central differences and to the oracle's hand adjoint) and
test_gpu_nmpc_frenet.py (which holds the kernel to them).  The rule is that of _nmpc_util.py; lm_step, cost_from_states, wrap and
the status constants are its own, imported.  What is stated here is what differs: the Frenet low-speed step and its Jacobian, the
residuals (s, ey, epsi, vx), and the frame guard.  NumPy, vectorised over the rows, every function in the dtype of its arrays.

  step            : one step of the model (the oracle's restatement of dynamics.py:190-281, low-speed right-hand side)
  step_jacobian   : F_x = d s' / d s, d s' / d a, d s' / d sv -- rollout_adjoint.h: jvp_coeffs<FRENET_LS>, entry for entry
  rollout         : the states, and which rows started every step inside the frame (1 - ey curv > 0)
  cost / linearize: the cost (+inf outside the frame), and g = J^T r, H = J^T J from the sensitivities
  solve           : the projected Levenberg-Marquardt with the guard
  family          : the problem families of the tests (reach / reg / stage / sat)
"""
import numpy as np

from oracle import irbfn_oracle as orc

from _nmpc_util import CONVERGED, DEFAULTS, DP, MAX_ITER, NONFINITE, STALLED, cost_from_states, lm_step, weights_as, wrap  # noqa: F401

COMP = (0, 1, 6, 3)                                     # the state component behind the residuals s, ey, heading error, speed
AS_ST = (0, 1, 2, 3, 6)                                 # the components that move; in this order _nmpc_util reads them as its own

WEIGHTS = {
    "reach": dict(q=(0, 0, 0, 0), qf=(10, 10, 5, 1), r=(0, 0), rd=(0, 0)),
    "reg": dict(q=(0, 0, 0, 0), qf=(0, 10, 5, 1), r=(0.01, 0.1), rd=(0.01, 0.1)),
    "stage": dict(q=(0, 1, 0.5, 0.1), qf=(0, 10, 5, 1), r=(0.01, 0.1), rd=(0.01, 0.1)),
}
WEIGHTS["sat"] = WEIGHTS["reg"]


def step(s, a, sv, dp):
    """s [B,8] = [s, ey, delta, vx, vy, wz, epsi, curv], a / sv [B] -> s' [B,8], in the dtype of s"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return orc.dynamic_frenet_onestep(s, np.stack([a, sv], -1), dp)


def _clipgrad(v, lo, hi, tie, ft):
    return np.where((v > lo) & (v < hi), ft(1), np.where((v == lo) | (v == hi), ft(tie), ft(0))).astype(ft)


def step_jacobian(s, dp, tie=0.5):
    """-> (Fx [B,8,8], Fa [B,8], Fsv [B,8]).  The controls are taken inside their box (slope 1); the clip of delta has slope 1
    inside, 0 outside, `tie` on a bound; vx has no clip."""
    ft = s.dtype.type
    dp = np.asarray(dp, ft)
    B = s.shape[0]
    LF, LR, dt, sm = dp[3], dp[4], dp[8], dp[11]
    one = ft(1)
    Lw = LR + LF
    ey, d_raw, vx, epsi, cur = (s[:, i] for i in (1, 2, 3, 6, 7))
    dc = np.clip(d_raw, -sm, sm)
    md = _clipgrad(d_raw, -sm, sm, tie, ft)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ce, se, td = np.cos(epsi), np.sin(epsi), np.tan(dc)
        den = one - ey * cur
        s1 = dt * (vx * ce * cur / (den * den))
        s3 = dt * (ce / den)
        s4 = dt * (-vx * se / den)
        Fx = np.zeros((B, 8, 8), ft)
        for i in range(8):
            Fx[:, i, i] = one
        Fx[:, 0, 1] = s1
        Fx[:, 0, 3] = s3
        Fx[:, 0, 6] = s4
        Fx[:, 1, 3] = dt * se
        Fx[:, 1, 6] = dt * vx * ce
        Fx[:, 6, 1] = -(cur * s1)
        Fx[:, 6, 2] = md * dt * vx * (one + td * td) / Lw
        Fx[:, 6, 3] = dt * td / Lw - cur * s3
        Fx[:, 6, 6] += -(cur * s4)
    Fa = np.zeros((B, 8), ft)
    Fa[:, 3] = dt
    Fsv = np.zeros((B, 8), ft)
    Fsv[:, 2] = dt
    return Fx, Fa, Fsv


def residual(s, goal):
    """[B,4]: (s - g_0, ey - g_1, wrap(epsi - g_2), vx - g_3)"""
    return np.stack([s[:, 0] - goal[:, 0], s[:, 1] - goal[:, 1], wrap(s[:, 6] - goal[:, 2]), s[:, 3] - goal[:, 3]], axis=1)


def inside_frame(s):
    """1 - ey curv > 0: the step that starts from s is inside the frame"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (s.dtype.type(1) - s[:, 1] * s[:, 7]) > 0


def rollout(u, s0, dp):
    """-> (states: T arrays [B,8], inside [B]: every step of the row started inside the frame)"""
    T = u.shape[1] // 2
    s, states, inside = s0, [], np.ones(s0.shape[0], bool)
    for t in range(T):
        inside &= inside_frame(s)
        s = step(s, u[:, t], u[:, T + t], dp)
        states.append(s)
    return states, inside


def cost_of(states, inside, u, goal, W):
    """the cost of _nmpc_util.cost_from_states on the residual components, +inf for a row that left the frame"""
    with np.errstate(invalid="ignore", over="ignore"):
        c = cost_from_states([s[:, AS_ST] for s in states], u, goal, W)[0]
    return np.where(inside, c, c.dtype.type(np.inf))


def cost(u, s0, goal, dp, W):
    states, inside = rollout(u, s0, dp)
    return cost_of(states, inside, u, goal, W)


def linearize(u, s0, goal, dp, W, tie=0.5):
    """-> (cost [B], g = J^T r [B,N], H = J^T J [B,N,N]) at u"""
    ft = u.dtype.type
    B, N = u.shape
    T = N // 2
    S = np.zeros((B, 8, N), ft)
    g, H = np.zeros((B, N), ft), np.zeros((B, N, N), ft)
    s, states, inside = s0, [], np.ones(B, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T):
            inside &= inside_frame(s)
            Fx, Fa, Fsv = step_jacobian(s, dp, tie)
            S = np.matmul(Fx, S)
            S[:, :, t], S[:, :, T + t] = Fa, Fsv
            s = step(s, u[:, t], u[:, T + t], dp)
            states.append(s)
            e = residual(s, goal)
            w = W["qf"] if t == T - 1 else W["q"]
            for k in range(4):
                row = S[:, COMP[k], :]
                g += (w[k] * e[:, k])[:, None] * row
                H += w[k] * row[:, :, None] * row[:, None, :]
    for t in range(T):
        for o, wr in ((0, W["r"][0]), (T, W["r"][1])):
            g[:, o + t] += wr * u[:, o + t]
            H[:, o + t, o + t] += wr
    for t in range(T - 1):
        for o, wd in ((0, W["rd"][0]), (T, W["rd"][1])):
            i, j = o + t, o + t + 1
            d = wd * (u[:, j] - u[:, i])
            g[:, i] -= d
            g[:, j] += d
            H[:, i, i] += wd
            H[:, j, j] += wd
            H[:, i, j] -= wd
            H[:, j, i] -= wd
    return cost_of(states, inside, u, goal, W), g, H


def solve(s0, goal, dp, W, T, u0=None, ft=np.float64, max_iter=30, lambda0=1e-3, lambda_min=1e-9, lambda_max=1e6, tol=1e-6,
          eps=1e-6, history=False):
    """The projected Levenberg-Marquardt of irbfn_nmpc_solve_frenet, every operand of dtype ft: _nmpc_util.solve (two-sided
    convergence test) with the Frenet linearisation and the guard -- a clipped start outside the frame has cost +inf and is
    NONFINITE like any other non-finite first cost; a trial step outside it has cost +inf, is rejected, and lambda grows.
    -> dict(u, cost0, cost, status, iters, grad[, costs])."""
    s0, goal, dp = np.asarray(s0, ft), np.asarray(goal, ft), np.asarray(dp, ft)
    W = weights_as(W, ft)
    B, N = s0.shape[0], 2 * T
    hi = np.concatenate([np.full(T, dp[10], ft), np.full(T, dp[9], ft)])
    raw = np.zeros((B, N), ft) if u0 is None else np.asarray(u0, ft)
    u = np.clip(raw, -hi, hi)
    finite = np.isfinite(s0).all(1) & np.isfinite(goal).all(1) & np.isfinite(raw).all(1) & np.isfinite(dp).all()
    lam = np.full(B, lambda0, ft)
    lmin, lmax, tol_ = ft(lambda_min), ft(lambda_max), ft(tol)
    status = np.full(B, MAX_ITER, np.int32)
    iters = np.zeros(B, np.int32)
    c, g, H = linearize(u, s0, goal, dp, W)
    bad = ~finite | ~np.isfinite(c)
    c0 = np.where(bad, ft(np.nan), c)
    c = c0.copy()
    status[bad] = NONFINITE
    status[~bad & (c == 0)] = CONVERGED
    done = bad | (c == 0)
    costs = [c.copy()]
    for it in range(max_iter):
        if done.all():
            break
        fixed = ((u <= -hi) & (g > 0)) | ((u >= hi) & (g < 0))
        d = lm_step(H, g, fixed, lam, eps)
        up = np.clip(u + d, -hi, hi)
        with np.errstate(invalid="ignore"):
            cp = cost(up, s0, goal, dp, W)
            act = ~done
            acc = act & (cp < c)
            near = np.abs(c - cp) <= tol_ * c
            conv = act & (near | (acc & (cp == 0)))
            rej = act & ~acc & ~conv
        iters[act] += 1
        u = np.where(acc[:, None], up, u)
        c = np.where(acc, cp, c)
        lam = np.where(acc, np.maximum(lam / ft(10), lmin), np.where(rej, np.minimum(ft(10) * lam, lmax), lam))
        stall = rej & (lam >= lmax)
        status[conv] = CONVERGED
        status[stall] = STALLED
        done = done | conv | stall
        costs.append(c.copy())
        _, g, H = linearize(u, s0, goal, dp, W)
    out = dict(u=u, cost0=c0, cost=c, status=status, iters=iters, grad=g)
    if history:
        out["costs"] = np.stack(costs, axis=0)
    return out


def draw(B, seed):
    """-> (rng after the draw, state0 [B,8] float32-representable float64): [0, ey, delta, vx, 0, 0, epsi, curv], ey ~ U(-0.5, 0.5),
    delta ~ U(-0.2, 0.2), vx ~ U(0.5, 6), epsi ~ U(-0.3, 0.3), curv ~ U(-0.3, 0.3), drawn in this order: 1 - ey curv >= 0.85"""
    rng = np.random.default_rng(seed)
    s0 = np.zeros((B, 8))
    for col, (lo, hi) in ((1, (-0.5, 0.5)), (2, (-0.2, 0.2)), (3, (0.5, 6.0)), (6, (-0.3, 0.3)), (7, (-0.3, 0.3))):
        s0[:, col] = rng.uniform(lo, hi, B)
    return rng, s0.astype(np.float32).astype(np.float64)


def edge_family(B, seed=17):
    """-> (state0 [B,8], goal [B,4], weights): rows next to the centre of curvature of a 2 m bend (curv = 0.5, ey ~ U(1.7, 1.98),
    so 1 - ey curv in 0.01 .. 0.15) whose goal lies beyond it (ey = 3).  With seed 17 and 256 rows about a quarter leave the frame
    with the controls at rest (NONFINITE), and of the others 36 at T = 5 meet a trial step that does."""
    rng = np.random.default_rng(seed)
    s0 = np.zeros((B, 8))
    for col, (lo, hi) in ((1, (1.7, 1.98)), (2, (-0.4, 0.4)), (3, (0.5, 6.0)), (6, (-0.5, 0.5))):
        s0[:, col] = rng.uniform(lo, hi, B)
    s0[:, 7] = 0.5
    goal = np.zeros((B, 4))
    goal[:, 1], goal[:, 3] = 3.0, 6.0
    return s0.astype(np.float32).astype(np.float64), goal, dict(q=(0, 0, 0, 0), qf=(0, 10, 5, 1), r=(0, 0), rd=(0, 0))


def family(name, B, T=5, seed=123):
    """-> (state0 [B,8], goal [B,4], weights), float32-representable float64, state0 from `draw`.
    reg / stage: goal = (0, 0, 0, U(1, 6)): back onto the line at another speed; progress is free.
    reach: the goal is (s, ey, epsi, vx) after rolling out u* with a* ~ U(-4, 4), sv* ~ U(-1.5, 1.5) (float64 model), so the
    minimum is 0.
    sat: reg with the goal 2 m to the other side of the line and speed 9: most rows end on a bound."""
    rng, s0 = draw(B, seed)
    if name == "reach":
        ustar = np.hstack([rng.uniform(-4, 4, (B, T)), rng.uniform(-1.5, 1.5, (B, T))])
        sT = rollout(ustar, s0, DP)[0][-1]
        goal = np.stack([sT[:, k] for k in COMP], axis=1)
    else:
        goal = np.zeros((B, 4))
        goal[:, 3] = rng.uniform(1.0, 6.0, B)
        if name == "sat":
            goal[:, 1] = -2.0 * np.sign(s0[:, 1])
            goal[:, 3] = 9.0
    return s0, goal.astype(np.float32).astype(np.float64), WEIGHTS[name]
