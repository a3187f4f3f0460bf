"""The float64 statements of the training-step kernels (irbfn_amd/csrc/train_step.hip and the softmax_xent pair of
rbf_vjp.hip), shared by test_train_step_reference_cpu.py (which holds them to torch.autograd) and test_gpu_train_step.py
(which holds the kernels to them).  A plain module (no fixtures, no hooks).

  seeds_oneint / seeds_fullint / seeds_frenet_fullint : (loss, gy = d loss / d y_pred, ambiguous[B]) in float64, from the
      oracle's roll-outs (oracle/irbfn_oracle.py) and hand adjoints (oracle/hand_vjp.py); `tie` is the clip() gradient on a bound.
  *_f32 : the same lines evaluated in np.float32 -- "what a plain float32 evaluation makes of the same inputs", the error the
      float32 bounds are measured against.
  adam_clip, softmax_xent : optax.chain(clip_by_global_norm, adam) and optax.softmax_cross_entropy(...).mean(), any dtype.

Ambiguity.  |.| and clip() have kinks: a float32 evaluation whose argument sits within rounding of a kink may legitimately take
the other sign or side, and then its whole row of gy differs by O(1/B), not by rounding.  A row is `ambiguous` if some L1
difference d has 0 < |d| < MARGIN, or if some pre-clip value (steering angle and speed before their clips, the controls against
a_max / sv_max) lies within MARGIN of a bound without being exactly on it.  Exactly on a kink is NOT ambiguous: the float32
kernels get the float32 inputs widened, so a tie stays a tie (d = 0 gives sgn = 0, a bound gives `tie`)."""
import numpy as np

from oracle import hand_vjp as hv
from oracle import irbfn_oracle as orc
from _rollout_util import RTOL

MARGIN = 1e-5
AMBIGUOUS_CAP = 0.05
TWIN_CAP = 1e-4          # largest error of a float32 twin on unambiguous rows, of max |gy|: rounding, far below a flipped sign
FULLINT_BOUNDS = ((-orc.FULLINT_MAX_STEER, orc.FULLINT_MAX_STEER), (orc.FULLINT_MIN_SPEED, orc.FULLINT_MAX_SPEED))


# ------------------------------------------------------------------ ambiguity
def _near_kink(d):
    """some entry of a row's L1 differences is within MARGIN of 0 without being 0"""
    a = np.abs(d).reshape(d.shape[0], -1)
    return ((a > 0) & (a < MARGIN)).any(axis=1)


def _near_bound(v, lo, hi):
    """some entry of a row's pre-clip values is within MARGIN of a bound without being on it"""
    v = v.reshape(v.shape[0], -1)
    near = np.zeros(v.shape, bool)
    for b in (lo, hi):
        near |= (np.abs(v - b) < MARGIN) & (v != b)
    return near.any(axis=1)


# ------------------------------------------------------------------ the three compositions, float64
def oneint_init(x):
    z = np.zeros_like(x[:, 0])
    return np.stack([z, z, z, x[:, 0], z, x[:, 6], x[:, 5]], -1)               # train_nmpc.py:260-266


def frenet_init(x):
    return x[:, [0, 0, 1, 2, 3, 5, 6, 7]]                                        # train_nmpc_frenet.py:398


def seeds_oneint(x, yp, y, dp, tie, B_total=None):
    """loss_fn of train_step_oneint (scripts/train_nmpc.py:268-295): x [B, D >= 7], yp / y [B, O >= 2].
    B_total (here and below): the rows given are some rows of a batch of B_total rows -- the means divide by B_total, so gy is
    those rows' gy in the whole batch (rows are independent) and the loss is their share of the batch loss."""
    x, yp, y, dp = (np.asarray(a, np.float64) for a in (x, yp, y, dp))
    n, O = yp.shape
    B = n if B_total is None else B_total
    init = oneint_init(x)
    xu_p = np.hstack([init, yp[:, :2]])
    actual = orc.dynamic_st_onestep_aux(np.hstack([init, y[:, :2]]), dp)         # :275
    pred = orc.dynamic_st_onestep_aux(xu_p, dp)                                  # :276
    idx = [0, 1, 3, 4]
    ds = pred[:, idx] - actual[:, idx]
    loss = (0.5 * (yp - y) ** 2).sum() / (B * O) + (0.5 * ds ** 2).sum() / (B * 4)     # the two means of :286-292
    gs = np.zeros((n, 1, 7))
    gs[:, 0, idx] = ds / (B * 4)
    gy = (yp - y) / (B * O)
    gy[:, :2] += hv.vjp_st_ks(xu_p, dp, gs, tie)[:, 7:9]
    amb = np.zeros(n, bool)
    for u in (yp, y):
        amb |= _near_bound(u[:, 0], -dp[10], dp[10]) | _near_bound(u[:, 1], -dp[9], dp[9])
    return float(loss), gy, amb


def _fullint_preclip(v0, u, states):
    """[B, T] steering angle and speed before the clips of train_nmpc.py:363 / :365 along a roll-out of u"""
    T = u.shape[1] // 2
    zero = np.zeros((u.shape[0], 1))
    d_prev = np.hstack([zero, states[:, :-1, 2]])
    v_prev = np.hstack([np.clip(v0, orc.FULLINT_MIN_SPEED, orc.FULLINT_MAX_SPEED)[:, None], states[:, :-1, 3]])
    return d_prev + u[:, T:] * orc.FULLINT_DT, v_prev + u[:, :T] * orc.FULLINT_DT


def seeds_fullint(x, yp, y, tie, B_total=None):
    """loss_fn of train_step_fullint (scripts/train_nmpc.py:306-390): x [B, D >= 1] (column 0 = speed), yp / y [B, 2T]."""
    x, yp, y = (np.asarray(a, np.float64) for a in (x, yp, y))
    n, O = yp.shape
    B = n if B_total is None else B_total
    T = O // 2
    v0 = x[:, 0]
    sa, sp = orc.rollout_fullint(v0, y), orc.rollout_fullint(v0, yp)             # :329-347, :356-374
    cols = [0, T]
    dy, df = yp[:, cols] - y[:, cols], sp[:, -1] - sa[:, -1]
    loss = np.abs(dy).sum() / (2 * B) + np.abs(df).sum() / (5 * B)               # the two means of :386-390
    gs = np.zeros((n, T, 5))
    gs[:, -1] = np.sign(df) / (5 * B)
    _, gy = hv.vjp_fullint(v0, yp, gs, tie)
    gy[:, cols] += np.sign(dy) / (2 * B)
    amb = _near_kink(dy) | _near_kink(df)
    for u, st in ((yp, sp), (y, sa)):
        for pre, (lo, hi) in zip(_fullint_preclip(v0, u, st), FULLINT_BOUNDS):
            amb |= _near_bound(pre, lo, hi)
    return float(loss), gy, amb


def seeds_frenet_fullint(x, yp, y, dp, tie, B_total=None):
    """loss_fn of the Frenet train_step_fullint (scripts/train_nmpc_frenet.py:394-421): x [B, D >= 8], yp / y [B, 2T]."""
    x, yp, y, dp = (np.asarray(a, np.float64) for a in (x, yp, y, dp))
    n, O = yp.shape
    B = n if B_total is None else B_total
    T = O // 2
    init = frenet_init(x)
    xu_p = np.hstack([init, yp])
    actual = orc.integrate_frenet_mult(np.hstack([init, y]), dp)                 # :407
    pred = orc.integrate_frenet_mult(xu_p, dp)                                   # :408
    dy, ds = yp - y, pred - actual
    loss = np.abs(dy).sum() / (B * O) + np.abs(ds).sum() / (B * T * 8)           # the means of :402, :409, :412
    gy = np.sign(dy) / (B * O) + hv.vjp_frenet(xu_p, dp, np.sign(ds) / (B * T * 8), tie)[:, 8:]
    amb = _near_kink(dy) | _near_kink(ds)
    for u, st in ((yp, pred), (y, actual)):
        delta = np.hstack([init[:, 2:3], st[:, :-1, 2]])                         # the steering angle each step clips (:227)
        amb |= _near_bound(delta, -dp[11], dp[11])
        amb |= _near_bound(u[:, :T], -dp[10], dp[10]) | _near_bound(u[:, T:], -dp[9], dp[9])
    return float(loss), gy, amb


# ------------------------------------------------------------------ the same lines in one dtype (float32 twins)
def _clipgrad(v, lo, hi, tie, ft):
    return np.where((v > lo) & (v < hi), ft(1), np.where((v == lo) | (v == hi), ft(tie), ft(0))).astype(ft)


def _vjp_st_ks_1(xu, dp, gs, tie, ft):
    """oracle/hand_vjp.py: vjp_st_ks at T = 1, every operand of dtype ft; returns (d/da, d/dsv)"""
    dt, svm, am = dp[8], dp[9], dp[10]
    ma, ms = _clipgrad(xu[:, 7], -am, am, tie, ft), _clipgrad(xu[:, 8], -svm, svm, tie, ft)
    return ma * dt * gs[:, 3], ms * dt * gs[:, 2]


def _vjp_fullint(v0, u, g_final, tie, ft):
    """oracle/hand_vjp.py: vjp_fullint with the seed on the final state only, every operand of dtype ft"""
    B, T = u.shape[0], u.shape[1] // 2
    DT, WB, VMAX, VMIN, SMAX = (ft(c) for c in (0.1, 0.33, 7.0, 0.0, 0.4189))
    zero = np.zeros(B, ft)
    s = [zero, zero, zero, np.clip(v0, VMIN, VMAX), zero]
    pre = []
    for t in range(T):
        pre.append((s[2], s[3], s[4]))
        a, dv = u[:, t], u[:, T + t]
        x_ = s[0] + s[3] * np.cos(s[4]) * DT
        y_ = s[1] + s[3] * np.sin(s[4]) * DT
        d = np.clip(s[2] + dv * DT, -SMAX, SMAX)
        v = np.clip(s[3] + a * DT, VMIN, VMAX)
        s = [x_, y_, d, v, s[4] + (v / WB) * np.tan(d) * DT]
    lam = [g_final[:, i] for i in range(5)]
    gu = np.zeros_like(u)
    for t in range(T - 1, -1, -1):
        d0, v0_, psi = pre[t]
        dpre, vpre = d0 + u[:, T + t] * DT, v0_ + u[:, t] * DT
        d1, v1 = np.clip(dpre, -SMAX, SMAX), np.clip(vpre, VMIN, VMAX)
        md, mv = _clipgrad(dpre, -SMAX, SMAX, tie, ft), _clipgrad(vpre, VMIN, VMAX, tie, ft)
        td, cp, sp = np.tan(d1), np.cos(psi), np.sin(psi)
        Ld = lam[2] + lam[4] * (v1 / WB) * (ft(1) + td * td) * DT
        Lv = lam[3] + lam[4] * td * DT / WB
        gu[:, t] = mv * Lv * DT
        gu[:, T + t] = md * Ld * DT
        l2 = md * Ld
        l3 = mv * Lv + DT * (lam[0] * cp + lam[1] * sp)
        l4 = lam[4] + DT * v0_ * (-lam[0] * sp + lam[1] * cp)
        lam[2], lam[3], lam[4] = l2, l3, l4
    return gu


def _vjp_frenet(xu, dp, gs, tie, ft):
    """oracle/hand_vjp.py: vjp_frenet, every operand of dtype ft; returns the control columns"""
    B, T = xu.shape[0], (xu.shape[1] - 8) // 2
    LF, LR, dt, svm, am, sm = dp[3], dp[4], dp[8], dp[9], dp[10], dp[11]
    Lw = LR + LF
    g = np.zeros((B, 2 * T), ft)
    s = xu[:, :8]
    cur = s[:, 7]
    pre = []
    for t in range(T):
        pre.append((s[:, 1], s[:, 2], s[:, 3], s[:, 6]))
        s = orc.dynamic_frenet_onestep(s, np.stack([xu[:, 8 + t], xu[:, 8 + T + t]], -1), dp)
    lam = [np.zeros(B, ft) for _ in range(8)]
    for t in range(T - 1, -1, -1):
        lam = [lam[i] + gs[:, t, i] for i in range(8)]
        ey, d, vx, ep = pre[t]
        dc = np.clip(d, -sm, sm)
        md = _clipgrad(d, -sm, sm, tie, ft)
        ma, ms = _clipgrad(xu[:, 8 + t], -am, am, tie, ft), _clipgrad(xu[:, 8 + T + t], -svm, svm, tie, ft)
        ce, se, td = np.cos(ep), np.sin(ep), np.tan(dc)
        den = ft(1) - ey * cur
        d0 = vx * ce / den
        A = lam[0] * dt - lam[6] * dt * cur
        g[:, t] = ma * dt * lam[3]
        g[:, T + t] = ms * dt * lam[2]
        l1 = lam[1] + A * (vx * ce * cur / den ** 2)
        l2 = lam[2] + md * lam[6] * dt * vx * (ft(1) + td * td) / Lw
        l3 = lam[3] + A * ce / den + lam[1] * dt * se + lam[6] * dt * td / Lw
        l6 = lam[6] + A * (-vx * se / den) + lam[1] * dt * vx * ce
        l7 = lam[7] + A * (vx * ce * ey / den ** 2) - lam[6] * dt * d0
        lam[1], lam[2], lam[3], lam[6], lam[7] = l1, l2, l3, l6, l7
    return g


def seeds_oneint_typed(x, yp, y, dp, tie, ft=np.float32, B_total=None):
    x, yp, y, dp = (np.asarray(a, ft) for a in (x, yp, y, dp))
    n, O = yp.shape
    B = n if B_total is None else B_total
    init = oneint_init(x)
    xu_p = np.hstack([init, yp[:, :2]])
    actual = orc.dynamic_st_onestep_aux(np.hstack([init, y[:, :2]]), dp)
    pred = orc.dynamic_st_onestep_aux(xu_p, dp)
    idx = [0, 1, 3, 4]
    ds = pred[:, idx] - actual[:, idx]
    loss = (ft(0.5) * (yp - y) ** 2).sum(dtype=ft) / ft(B * O) + (ft(0.5) * ds ** 2).sum(dtype=ft) / ft(B * 4)
    gs = np.zeros((n, 7), ft)
    gs[:, idx] = ds / ft(B * 4)
    gy = (yp - y) / ft(B * O)
    ga, gsv = _vjp_st_ks_1(xu_p, dp, gs, tie, ft)
    gy[:, 0] += ga
    gy[:, 1] += gsv
    assert gy.dtype == ft and loss.dtype == ft
    return loss, gy


def seeds_fullint_typed(x, yp, y, tie, ft=np.float32, B_total=None):
    x, yp, y = (np.asarray(a, ft) for a in (x, yp, y))
    n, O = yp.shape
    B = n if B_total is None else B_total
    T = O // 2
    v0 = x[:, 0]
    sa, sp = orc.rollout_fullint(v0, y), orc.rollout_fullint(v0, yp)
    cols = [0, T]
    dy, df = yp[:, cols] - y[:, cols], sp[:, -1] - sa[:, -1]
    loss = np.abs(dy).sum(dtype=ft) / ft(2 * B) + np.abs(df).sum(dtype=ft) / ft(5 * B)
    gy = _vjp_fullint(v0, yp, np.sign(df) / ft(5 * B), tie, ft)
    gy[:, cols] += np.sign(dy) / ft(2 * B)
    assert gy.dtype == ft and loss.dtype == ft and sp.dtype == ft
    return loss, gy


def seeds_frenet_fullint_typed(x, yp, y, dp, tie, ft=np.float32, B_total=None):
    x, yp, y, dp = (np.asarray(a, ft) for a in (x, yp, y, dp))
    n, O = yp.shape
    B = n if B_total is None else B_total
    T = O // 2
    init = frenet_init(x)
    xu_p = np.hstack([init, yp])
    actual = orc.integrate_frenet_mult(np.hstack([init, y]), dp)
    pred = orc.integrate_frenet_mult(xu_p, dp)
    dy, ds = yp - y, pred - actual
    loss = np.abs(dy).sum(dtype=ft) / ft(B * O) + np.abs(ds).sum(dtype=ft) / ft(B * T * 8)
    gy = np.sign(dy) / ft(B * O) + _vjp_frenet(xu_p, dp, np.sign(ds) / ft(B * T * 8), tie, ft)
    assert gy.dtype == ft and loss.dtype == ft and pred.dtype == ft
    return loss, gy


def seeds_oneint_f32(x, yp, y, dp, tie, B_total=None):
    return seeds_oneint_typed(x, yp, y, dp, tie, np.float32, B_total)


def seeds_fullint_f32(x, yp, y, tie, B_total=None):
    return seeds_fullint_typed(x, yp, y, tie, np.float32, B_total)


def seeds_frenet_fullint_f32(x, yp, y, dp, tie, B_total=None):
    return seeds_frenet_fullint_typed(x, yp, y, dp, tie, np.float32, B_total)


# ------------------------------------------------------------------ optimiser and cross-entropy
def adam_clip(p, g, m, v, t, lr, b1, b2, eps, max_norm):
    """optax.chain(clip_by_global_norm(max_norm), adam(lr)) applied once (orc.clip_by_global_norm + orc.adam_update written
    out): t is the INCREMENTED count; max_norm <= 0 means no clip.  Every operand in the dtype of p.  -> (p_new, m, v)"""
    ft = p.dtype.type
    lr, b1, b2, eps, max_norm = (ft(c) for c in (lr, b1, b2, eps, max_norm))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        gn = np.sqrt((g * g).sum(dtype=ft))
        if max_norm > 0 and not (gn < max_norm):
            g = g / gn * max_norm
        m = b1 * m + (ft(1) - b1) * g
        v = b2 * v + (ft(1) - b2) * g * g
        mhat, vhat = m / (ft(1) - b1 ** ft(t)), v / (ft(1) - b2 ** ft(t))
        return p - lr * mhat / (np.sqrt(vhat) + eps), m, v


def softmax_xent(logits, labels):
    """optax.softmax_cross_entropy(logits, labels).mean() and its cotangent of the logits, by log-sum-exp, in the dtype of
    logits.  Labels need not sum to 1: d/dlogits = (softmax * sum_r labels - labels) / B."""
    ft = logits.dtype.type
    B = logits.shape[0]
    mx = logits.max(axis=1, keepdims=True)
    lse = mx + np.log(np.exp(logits - mx).sum(axis=1, keepdims=True, dtype=ft))
    lp = logits - lse
    loss = (-(labels * lp).sum(axis=1, dtype=ft)).mean(dtype=ft)
    g = (np.exp(lp) * labels.sum(axis=1, keepdims=True, dtype=ft) - labels) / ft(B)
    return loss, g


# ------------------------------------------------------------------ the bounds
def ratio32(got, ref, ref32, scale=None):
    """largest |err| / bound under the project's float32 rule (tests/_rollout_util.assert_states_close with the entries of the
    case as one trajectory and scale = max |ref|, or the scale given): bound = max(1e-5 (|ref| + scale), 4 x max |ref32 - ref| +
    1e-7 scale).  <= 1 passes.  Non-finite reference entries must be met exactly; a zero scale asks for zero error."""
    got, ref, ref32 = (np.asarray(a, np.float64).reshape(-1) for a in (got, ref, ref32))
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin], equal_nan=True)
    got, ref, ref32 = got[fin], ref[fin], ref32[fin]
    if ref.size == 0:
        return 0.0
    assert np.isfinite(got).all() and np.isfinite(ref32).all()
    err = np.abs(got - ref)
    own = scale is None
    scale = np.abs(ref).max() if own else scale
    if scale == 0:
        assert (err == 0).all()
        return 0.0
    bound = np.maximum(RTOL * (np.abs(ref) + scale), 4.0 * np.abs(ref32 - ref).max() + 1e-7 * scale)
    return float((err / bound).max())


def rel64(got, ref, tol):
    """largest |err| / tol over the finite reference entries; the others must be met exactly"""
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin], equal_nan=True)
    return float(np.abs(got[fin] - ref[fin]).max(initial=0.0) / tol)


# ------------------------------------------------------------------ inputs (float32-representable, returned as float64)
def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def fullint_case(B, T, D, seed):
    """x[:, 0] ~ U(-0.5, 7.5); labels N(0, 3) / N(0, 1); predictions = labels + N(0, 1) / N(0, 0.3)."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(B, D))
    x[:, 0] = rng.uniform(-0.5, 7.5, B)
    y = np.hstack([rng.normal(size=(B, T)) * 3.0, rng.normal(size=(B, T))])
    yp = y + np.hstack([rng.normal(size=(B, T)), rng.normal(size=(B, T)) * 0.3])
    return _f32(x), _f32(yp), _f32(y)


def frenet_case(B, T, D, seed):
    """x = [ey, delta, vx, vy, vx_goal, wz, epsi, cur] in the range of tests/_rollout_util.frenet_inputs (|ey * cur| << 1);
    labels N(0, 2) / N(0, 0.5); predictions = labels + N(0, 0.5) / N(0, 0.2)."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(B, D))
    x[:, :8] = x[:, :8] * [.2, .2, 1, .1, 1, .1, .15, .08] + [0, 0, 4, 0, 4, 0, 0, 0]
    y = np.hstack([rng.normal(size=(B, T)) * 2.0, rng.normal(size=(B, T)) * 0.5])
    yp = y + np.hstack([rng.normal(size=(B, T)) * 0.5, rng.normal(size=(B, T)) * 0.2])
    return _f32(x), _f32(yp), _f32(y)


def oneint_case(B, O, D, seed):
    """x = [v_c, ..., beta, angv] with v_c ~ U(-0.5, 7.5); labels N(0, 5) / N(0, 2) in the two control columns (a few per
    cent outside a_max = 9.51 / sv_max = 3.2), N(0, 1) in the others; predictions = labels + N(0, 1) / N(0, 0.3)."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(B, D)) * 0.3
    x[:, 0] = rng.uniform(-0.5, 7.5, B)
    y = rng.normal(size=(B, O)) * ([5.0, 2.0] + [1.0] * (O - 2))
    yp = y + rng.normal(size=(B, O)) * ([1.0, 0.3] + [0.5] * (O - 2))
    return _f32(x), _f32(yp), _f32(y)


def splice_rows(kind, x, yp, y, rows, dp=None):
    """Tie and zero rows written over `rows` = (r0, r1, r2) of a batch (fewer rows in a batch too small for all three).
    r0 / r1: the clip ties.  fullint: x = 0 (r0) or 7 (r1) with a_0 = 0 puts the first pre-clip speed exactly on VMIN / VMAX
    (label a_0 = +2 / -2, so that the labelled speed leaves the bound and the seed on the speed is not 0).
    oneint / Frenet: the controls exactly on +a_max (a_0) and -sv_max (the last steering rate), r1 with the signs swapped
    (labels 0 there).
    r2: y_pred == y in every column, so every L1 difference is exactly 0.  Returns the rows used as {name: row}."""
    B, O = yp.shape
    used = {}
    T = O // 2
    for name, r in zip(("tie_lo", "tie_hi", "zero"), rows):
        if r is None or r >= B or r in used.values():
            continue
        used[name] = r
        if name == "zero":
            yp[r] = y[r]
        elif kind == "fullint":
            x[r, 0] = 0.0 if name == "tie_lo" else 7.0
            yp[r, 0] = 0.0
            y[r, 0] = 2.0 if name == "tie_lo" else -2.0       # the label moves off the bound: the speed seed is not 0
        else:
            sgn = 1.0 if name == "tie_lo" else -1.0
            a_col, sv_col = (0, 1) if kind == "oneint" else (0, O - 1)
            yp[r, a_col] = sgn * dp[10]
            yp[r, sv_col] = -sgn * dp[9]
            y[r, a_col] = y[r, sv_col] = 0.0                  # the labelled controls are inside their bounds: the seeds are not 0
    return used
