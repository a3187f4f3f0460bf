"""The statements behind the ST_SELECT adjoint (irbfn_amd/csrc/rollout_adjoint.h: vjp_back_step<ST_SELECT>) and the single-track
full-integration seeds (train_step.hip: seeds_multistep_kernel), shared by test_st_select_reference_cpu.py (which holds them to
torch.autograd) and test_gpu_st_select_vjp.py / test_gpu_train_st.py (which hold the kernels to them).  A plain module.

The convention.  One step is x' = x + select(V > 3, f, f_ks) dt, V the clipped speed (oracle.dynamic_st_onestep).  The adjoint
holds the mask constant: a step taken on the dynamic branch back-propagates through f, one taken on the kinematic branch through
f_ks, V = 3 exactly is kinematic.  The reference has no counterpart (jax.grad through its lax.select is NaN at V = 0).

  st_select_torch     : (a) the float64 restatement in torch.  f is evaluated on a copy of the state whose speed column is
                        where(mask, v, 5.0) -- finite on every lane, the true state on every lane that selects it -- and f_ks on
                        the true state; the values are oracle.integrate_st_mult's, the gradient is branch-wise and free of NaN.
  vjp_st_select       : (b) the NumPy statement of the kernel's formulas, every operand of dtype ft (np.float64: the reference
                        the kernels are held to; np.float32: "what a plain float32 evaluation makes of the same inputs").
  seeds_st_fullint    : (c) loss, gy = d loss / d y_pred and the ambiguous rows of irbfn_train_seeds_st_fullint, dtype ft.
  grid_inputs         : (d) rows whose speeds stay == 0.1 (mod 0.25): never within 0.1 of the switch at 3, never on v_max = 7.
"""
import numpy as np

from irbfn_amd import configs
from oracle import irbfn_oracle as orc

import _train_step_util as tu

DP = np.array(configs.DYN_PARAMS, np.float64)          # KAT-1
SWITCH = 3.0
STATE_IDX = [0, 1, 3, 4]                               # the state components of the reference's one-step loss


# ------------------------------------------------------------------ (a) float64 restatement, torch
def st_select_step_torch(x, a, sv, dp):
    import torch
    V = torch.clip(x[:, 3], min=-dp[12], max=dp[12])
    mask = V > SWITCH
    safe = torch.cat([x[:, :3], torch.where(mask, x[:, 3], torch.full_like(V, 5.0))[:, None], x[:, 4:]], dim=1)
    f, _, _ = orc.st_rhs(safe, a, sv, dp)
    _, f_ks, _ = orc.st_rhs(x, a, sv, dp)
    return x + torch.where(mask[:, None], f, f_ks) * dp[8], V


def st_select_torch(xu, dp, T=None, select=True):
    """xu [B, 7 + 2T] (torch, float64) -> (all_states [B, T, 7], V [B, T] = the clipped speed each step saw).
    select=False: the kinematic model alone (oracle.integrate_st_ks_mult)."""
    import torch
    T = (xu.shape[1] - 7) // 2 if T is None else T
    x = xu[:, :7]
    states, Vs = [], []
    for t in range(T):
        if select:
            x, V = st_select_step_torch(x, xu[:, 7 + t], xu[:, 7 + T + t], dp)
        else:
            V = torch.clip(x[:, 3], min=-dp[12], max=dp[12])
            x = orc.dynamic_st_onestep_aux(torch.cat([x, xu[:, 7 + t:8 + t], xu[:, 7 + T + t:8 + T + t]], dim=1), dp)
        states.append(x)
        Vs.append(V)
    if T == 0:
        return xu.new_zeros((xu.shape[0], 0, 7)), xu.new_zeros((xu.shape[0], 0))
    return torch.stack(states, 1), torch.stack(Vs, 1)


def autograd_vjp(xu, dp, gs, select=True):
    """torch.autograd of (a): (g [B, 7 + 2T], states, V) as float64 NumPy"""
    import torch
    xt = torch.tensor(np.asarray(xu, np.float64), requires_grad=True)
    states, V = st_select_torch(xt, [float(c) for c in dp], select=select)
    (states * torch.tensor(np.asarray(gs, np.float64))).sum().backward()
    return xt.grad.numpy(), states.detach().numpy(), V.detach().numpy()


# ------------------------------------------------------------------ (b) the kernel's formulas, NumPy, one dtype
def _clipgrad(v, lo, hi, tie, ft):
    return np.where((v > lo) & (v < hi), ft(1), np.where((v == lo) | (v == hi), ft(tie), ft(0))).astype(ft)


def _forward_states(xu, dp, T, select):
    """the pre-step states [T] of the roll-out, in the dtype of xu (oracle steps)"""
    s = xu[:, :7]
    pre = []
    for t in range(T):
        pre.append(s)
        if select:
            s = orc.dynamic_st_onestep(s, np.stack([xu[:, 7 + t], xu[:, 7 + T + t]], -1), dp)
        else:
            s = orc.dynamic_st_onestep_aux(np.hstack([s, xu[:, 7 + t:8 + t], xu[:, 7 + T + t:8 + T + t]]), dp)
    return pre


def vjp_st_select(xu, dp, gs, tie=0.5, ft=np.float64, select=True):
    """gs [B, T, 7] -> g [B, 7 + 2T]: rollout_adjoint.h, vjp_back_step<ST_SELECT>, line by line.  select=False holds every step
    to the kinematic branch (= oracle/hand_vjp.py: vjp_st_ks)."""
    xu, gs = np.asarray(xu, ft), np.asarray(gs, ft)
    dp = np.asarray(dp, ft)
    B, T = xu.shape[0], (xu.shape[1] - 7) // 2
    mu, m, I, lf, lr, C_Sf, C_Sr, h, dt, svm, am, sm, vm = (dp[i] for i in range(13))
    g9, one = ft(orc.G_ACC), ft(1)
    Lw = lr + lf
    pre = _forward_states(xu, dp, T, select)
    g = np.zeros_like(xu)
    lam = [np.zeros(B, ft) for _ in range(7)]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for t in range(T - 1, -1, -1):
            lam = [lam[i] + gs[:, t, i] for i in range(7)]
            d_raw, v_raw, psi, pd, beta = (pre[t][:, i] for i in (2, 3, 4, 5, 6))
            a_in, sv_in = xu[:, 7 + t], xu[:, 7 + T + t]
            DELTA, V, A = np.clip(d_raw, -sm, sm), np.clip(v_raw, -vm, vm), np.clip(a_in, -am, am)
            md, mv = _clipgrad(d_raw, -sm, sm, tie, ft), _clipgrad(v_raw, -vm, vm, tie, ft)
            ma, ms = _clipgrad(a_in, -am, am, tie, ft), _clipgrad(sv_in, -svm, svm, tie, ft)
            dyn = (V > ft(SWITCH)) if select else np.zeros(B, bool)
            ang = np.where(dyn, psi + beta, psi)
            cp, sp, td = np.cos(ang), np.sin(ang), np.tan(DELTA)
            # kinematic lanes: ST_KS
            gak = ma * dt * lam[3]
            l2k = lam[2] + md * lam[4] * (V / Lw) * (one + td * td) * dt
            l3k = lam[3] + mv * dt * (lam[0] * cp + lam[1] * sp + lam[4] * td / Lw)
            head = dt * V * (-lam[0] * sp + lam[1] * cp)
            # dynamic lanes
            glr, glf = g9 * lr - A * h, g9 * lf + A * h
            E, F = C_Sf * glr, C_Sr * glf
            P, Q, R, M = lf * E, lr * F, lf * lf * E + lr * lr * F, F * lr - E * lf
            rV = one / V
            pv = pd * rV
            c5, c6 = (mu * m) / (I * Lw), (mu * rV) / Lw
            U = E * DELTA - (F + E) * beta + M * pv
            Ea, Fa = -C_Sf * h, C_Sr * h
            f5A = c5 * (lf * Ea * DELTA + (lr * Fa - lf * Ea) * beta - (lf * lf * Ea + lr * lr * Fa) * pv)
            f6A = c6 * (Ea * DELTA - (Fa + Ea) * beta + (Fa * lr - Ea * lf) * pv)
            f5V, f6V = c5 * R * pv * rV, -c6 * (U + M * pv) * rV
            f5W, f6W = -c5 * R * rV, c6 * M * rV - one
            gad = ma * dt * (lam[3] + lam[5] * f5A + lam[6] * f6A)
            l2d = lam[2] + md * dt * (lam[5] * (c5 * P) + lam[6] * (c6 * E))
            l3d = lam[3] + mv * dt * (lam[0] * cp + lam[1] * sp + lam[5] * f5V + lam[6] * f6V)
            l5d = lam[5] + dt * (lam[4] + lam[5] * f5W + lam[6] * f6W)
            l6d = lam[6] + head + dt * (lam[5] * (c5 * (Q - P)) - lam[6] * (c6 * (F + E)))
            g[:, 7 + t] = np.where(dyn, gad, gak)
            g[:, 7 + T + t] = ms * dt * lam[2]
            lam = [lam[0], lam[1], np.where(dyn, l2d, l2k), np.where(dyn, l3d, l3k), lam[4] + head,
                   np.where(dyn, l5d, lam[5]), np.where(dyn, l6d, lam[6])]
    for i in range(7):
        g[:, i] = lam[i]
    assert g.dtype == ft
    return g


# ------------------------------------------------------------------ (c) the seeds of irbfn_train_seeds_st_fullint
def rollout(xu, dp, select=True):
    """all_states [B, T, 7] in the dtype of xu (oracle.integrate_st_mult / integrate_st_ks_mult)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return orc.integrate_st_mult(xu, dp) if select else orc.integrate_st_ks_mult(xu, dp)


def seeds_st_fullint(x, yp, y, dp, tie, select=True, ft=np.float64, B_total=None):
    """x [B, D >= 7], yp / y [B, 2T] -> (loss, gy [B, 2T], ambiguous [B]); initial state as train_step_oneint
    (_train_step_util.oneint_init); loss = mean|yp - y| + mean|S_pred[:, :, [0,1,3,4]] - S_act[:, :, [0,1,3,4]]|.
    ambiguous: an L1 difference, a pre-clip value or a control within MARGIN of its kink (as _train_step_util), or a clipped speed
    within MARGIN of the switch at 3 without being on it."""
    x, yp, y, dp = (np.asarray(a, ft) for a in (x, yp, y, dp))
    n, O = yp.shape
    B = n if B_total is None else B_total
    T = O // 2
    init = tu.oneint_init(x)
    xu_p, xu_a = np.hstack([init, yp]), np.hstack([init, y])
    pred, actual = rollout(xu_p, dp, select), rollout(xu_a, dp, select)
    dy, ds = yp - y, pred[:, :, STATE_IDX] - actual[:, :, STATE_IDX]
    loss = np.abs(dy).sum(dtype=ft) / ft(B * O) + np.abs(ds).sum(dtype=ft) / ft(B * T * 4)
    gs = np.zeros((n, T, 7), ft)
    gs[:, :, STATE_IDX] = np.sign(ds) / ft(B * T * 4)
    gy = np.sign(dy) / ft(B * O) + vjp_st_select(xu_p, dp, gs, tie, ft, select)[:, 7:]
    amb = tu._near_kink(dy) | tu._near_kink(ds)
    for u, st in ((yp, pred), (y, actual)):
        before = np.concatenate([init[:, None, :], st[:, :-1]], axis=1)            # the state each step starts from
        amb |= tu._near_bound(before[:, :, 2], -dp[11], dp[11]) | tu._near_bound(before[:, :, 3], -dp[12], dp[12])
        amb |= tu._near_bound(u[:, :T], -dp[10], dp[10]) | tu._near_bound(u[:, T:], -dp[9], dp[9])
        if select:
            V = np.clip(before[:, :, 3], -dp[12], dp[12])
            amb |= tu._near_bound(V, SWITCH, SWITCH)
    assert gy.dtype == ft and loss.dtype == ft and pred.dtype == ft
    return loss, gy, amb


# ------------------------------------------------------------------ (d) inputs away from the switch
def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def grid_controls(B, T, rng):
    """[a_0..a_{T-1}, sv_0..sv_{T-1}]: a_t in 2.5 * {-3..3} (|a| < a_max, a dt a multiple of 0.25), sv ~ N(0, 1)"""
    return np.hstack([2.5 * rng.integers(-3, 4, size=(B, T)), rng.normal(size=(B, T))])


def grid_rows(B, T, rng):
    """Rows [B, 7 + 2T] of grid (d), float64: v0 = 0.1 + 0.25 k, k = row % 27; dt = 0.1 (KAT-1), so every V_t is == 0.1 (mod 0.25)"""
    st = np.zeros((B, 7))
    st[:, 0:2] = rng.normal(size=(B, 2)) * 2
    st[:, 2] = rng.uniform(-0.35, 0.35, B)
    st[:, 3] = 0.1 + 0.25 * (np.arange(B) % 27)
    st[:, 4] = rng.uniform(-3, 3, B)
    st[:, 5] = 0.5 * rng.normal(size=B)
    st[:, 6] = 0.1 * rng.normal(size=B)
    return np.hstack([st, grid_controls(B, T, rng)])


def grid_inputs(B, T, seed):
    """grid_rows, float32-representable.  Asserts min|V_t - 3| >= 1e-3 on the float64 reference and drops no row."""
    xu = _f32(grid_rows(B, T, np.random.default_rng(seed)))
    assert_off_switch(xu)
    return xu


def clipped_speeds(xu, dp=DP, select=True):
    """[B, T]: the clipped speed every step of the float64 roll-out sees"""
    xu = np.asarray(xu, np.float64)
    T = (xu.shape[1] - 7) // 2
    if T == 0:
        return np.zeros((xu.shape[0], 0))
    st = rollout(xu, dp, select)
    v = np.hstack([xu[:, 3:4], st[:, :-1, 3]])
    return np.clip(v, -dp[12], dp[12])


def assert_off_switch(xu, dp=DP, margin=1e-3):
    V = clipped_speeds(xu, dp)
    if V.size:
        assert np.abs(V - SWITCH).min() >= margin, float(np.abs(V - SWITCH).min())
    return V


def seed_case(B, T, D, seed):
    """x [B, D], yp, y [B, 2T] for the seed kernels: x[:, 0] = v0 on the speed grid of (d), labels on its control grid,
    y_pred = y + N(0, 0.3) -- the predicted accelerations leave the grid; a predicted speed within MARGIN of the switch makes
    its row ambiguous (seeds_st_fullint).
    Two spreads are five times those of (d).  The entry point's initial state has heading 0 and steering angle 0, so the lateral
    position of the first states differs between the predicted and the labelled roll-out only in second order: dy_2 =
    dV sin(psi_1 + beta_1) dt.  With (d)'s beta0 ~ 0.1 N, psi_dot0 ~ 0.5 N and dV = 0.03 that is ~ 3e-4 N, MARGIN = 1e-5 catches
    3 % of it per early step, and 12-20 % of the select model's rows came out ambiguous in the float64 statement (T = 5, 6, 16).
    Here beta0 ~ 0.5 N, psi_dot0 ~ 2.5 N (x[:, 5], x[:, 6]) and the predictions' noise on the first two steps is N(0, 1.5): the
    early lateral differences are first order, and 1-2 % of the rows are ambiguous (4.3 % at the most, T = 6, B = 257; every
    test asserts _train_step_util.AMBIGUOUS_CAP = 5 %); MARGIN is the project's."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(B, D)) * 0.3
    x[:, 0] = 0.1 + 0.25 * (np.arange(B) % 27)
    x[:, 5] = 0.5 * rng.normal(size=B)
    x[:, 6] = 2.5 * rng.normal(size=B)
    y = grid_controls(B, T, rng)
    noise = rng.normal(size=(B, 2 * T)) * 0.3
    first = [c for t in range(min(T, 2)) for c in (t, T + t)]
    noise[:, first] *= 5.0
    return _f32(x), _f32(y + noise), _f32(y)
