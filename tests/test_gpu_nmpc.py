"""The batched NMPC solver (irbfn_nmpc_solve, K13: nmpc_solve_kernel<MODE, T>) against the float64 NumPy statement of its rule
(_nmpc_util.py, held to central differences and the oracle's hand adjoints by test_nmpc_cpu.py), the roll-out kernels it shares
its step with, and the Python layer on top of it (make_table, closed_loop).

Shapes: B in {1, 63, 65, 257} (one lane, either side of a wave = a block of this kernel, several blocks), T in {1, 5, 8} (the
smallest, the reference's, the largest instance), both models.  Problem families: _nmpc_util.family."""
import numpy as np
import pytest

from irbfn_amd import _lib, dynamics, kmeans, linear_fit, nmpc, simulate, tables
from irbfn_amd.model import WCRBFNet

import _nmpc_util as nu
import _simulate_util as su

pytestmark = pytest.mark.gpu
F32 = np.float32
DP = nu.DP.astype(F32).astype(np.float64)             # what the kernel gets, widened
MODES = [pytest.param(False, id="ks"), pytest.param(True, id="select")]
SHAPES = [(1, 1), (63, 5), (65, 8), (257, 5), (64, 1), (257, 8)]
SWITCH_BAND = 0.4                                     # m/s around V = 3: where ST_SELECT rows may creep along the switch
_cache = {}


def mode_of(select):
    return _lib.ROLLOUT_ST_SELECT if select else _lib.ROLLOUT_ST_KS


def weights(W):
    return nmpc.Weights(**W)


def problem(name, B, T, select):
    """(s0, goal, W) of a family, made once and read-only"""
    key = ("p", name, B, T, select)
    if key not in _cache:
        s0, goal, W = nu.family(name, B, T, seed=123 + B + T, select=select)
        s0.setflags(write=False)
        goal.setflags(write=False)
        _cache[key] = (s0, goal, W)
    return _cache[key]


def reference(name, B, T, select, ft):
    key = ("r", name, B, T, select, ft)
    if key not in _cache:
        s0, goal, W = problem(name, B, T, select)
        _cache[key] = nu.solve(s0, goal, DP, W, T, select, ft=ft, **nu.DEFAULTS)
    return _cache[key]


def run(name, B, T, select, **kw):
    s0, goal, W = problem(name, B, T, select)
    opts = dict(nu.DEFAULTS)
    opts.update(kw)
    return nmpc.solve(s0.astype(F32), goal.astype(F32), DP, T=T, weights=weights(W), mode=mode_of(select), **opts)


def host(res):
    g = None if res.grad is None else res.grad.cpu().numpy()
    return dict(u=res.controls.cpu().numpy(), cost0=res.cost0.cpu().numpy(), cost=res.cost.cpu().numpy(),
                status=res.status.cpu().numpy(), iters=res.iterations.cpu().numpy(), grad=g)


def same_bits(a, b, rows_a=slice(None), rows_b=slice(None)):
    for k in ("u", "cost0", "cost", "status", "iters", "grad"):
        if a[k] is None:
            assert b[k] is None
            continue
        assert a[k][rows_a].tobytes() == b[k][rows_b].tobytes(), k


def rolled_states(select, s0, u, T):
    xu = np.hstack([s0, u]).astype(F32)
    st = dynamics.rollout_forward(mode_of(select), xu, DP, T)
    return np.asarray(st, np.float64)


# ------------------------------------------------------------------ 1. the cost is the roll-out's
@pytest.mark.parametrize("select", MODES)
@pytest.mark.parametrize("B,T", SHAPES, ids=lambda v: str(v))
def test_cost_is_the_cost_of_the_rollout_of_the_returned_controls(gpu, B, T, select):
    """cost[:, 1] against the float64 cost of irbfn_rollout_forward's float32 states for the returned u.  The kernel's states are
    those bits; what differs is the float32 arithmetic of m = 8T - 2 terms: per term the subtraction, the square and the weight
    (3 roundings, the subtraction counted twice as it is squared: 4 x 2^-24 of the term), then m - 1 additions and the half:
    |error| <= (m + 4) 2^-24 cost <= m 2^-23 cost for m >= 4 (m = 6 at T = 1).  Measured: <= 5.1e-7 of the cost at every shape."""
    s0, goal, W = problem("stage", B, T, select)
    r = host(run("stage", B, T, select))
    states = rolled_states(select, s0, r["u"], T)
    W64 = nu.weights_as(W, np.float64)
    c64, _, m = nu.cost_from_states([states[:, t] for t in range(T)], r["u"].astype(np.float64), goal, W64)
    assert m == 8 * T - 2
    err = np.abs(r["cost"] - c64)
    print(f"[nmpc cost] B={B} T={T} select={select}: max err / cost {np.max(err / c64):.2e}, bound {m * 2.0 ** -23:.2e}")
    assert (err <= m * 2.0 ** -23 * c64).all()
    u0 = np.zeros((B, 2 * T))
    c0, _, _ = nu.cost_from_states([s for s in np.moveaxis(rolled_states(select, s0, u0, T), 1, 0)], u0, goal, W64)
    assert (np.abs(r["cost0"] - c0) <= m * 2.0 ** -23 * c0).all()


# ------------------------------------------------------------------ 2. the gradient
@pytest.mark.parametrize("select", MODES)
@pytest.mark.parametrize("B,T", SHAPES, ids=lambda v: str(v))
def test_gradient_at_the_start_is_the_rollout_vjp_of_the_residuals(gpu, B, T, select):
    """max_iter = 0: grad = J^T r at the clipped start, composed here from irbfn_rollout_vjp / irbfn_rollout_vjp_select seeded
    with the weighted residuals (float64 from the float32 states) plus the control terms.  Bound: the roll-out VJP tests' own,
    5e-5 max|ref| + 1e-6 (test_gpu_st_select_vjp.py)."""
    s0, goal, W = problem("stage", B, T, select)
    rng = np.random.default_rng(B + T)
    s0 = s0.copy()
    s0[:, 2] = rng.uniform(-0.3, 0.3, B)
    s0[:, 4:] = rng.normal(size=(B, 3)) * [1.0, 0.3, 0.05]
    s0 = s0.astype(F32).astype(np.float64)
    u0 = np.hstack([rng.uniform(-4, 4, (B, T)), rng.uniform(-1.5, 1.5, (B, T))]).astype(F32).astype(np.float64)
    res = nmpc.solve(s0.astype(F32), goal.astype(F32), DP, T=T, weights=weights(W), u0=u0.astype(F32), mode=mode_of(select),
                     max_iter=0, want_grad=True)
    r = host(res)
    assert np.array_equal(r["u"], u0.astype(F32)) and (r["status"] == nu.MAX_ITER).all() and (r["iters"] == 0).all()
    assert r["cost0"].tobytes() == r["cost"].tobytes() and np.isfinite(r["cost"]).all()
    W64 = nu.weights_as(W, np.float64)
    states = rolled_states(select, s0, u0, T)
    gs = np.zeros((B, T, 7))
    for t in range(T):
        e = nu.residual(states[:, t], goal)
        w = W64["qf"] if t == T - 1 else W64["q"]
        for k in range(4):
            gs[:, t, nu.COMP[k]] = w[k] * e[:, k]
    xu = np.hstack([s0, u0]).astype(F32)
    if select:
        back = dynamics.rollout_vjp_select(xu, DP, gs.astype(F32), T)
    else:
        back = dynamics.rollout_vjp(_lib.ROLLOUT_ST_KS, xu, DP, gs.astype(F32), T)
    ref = np.asarray(back, np.float64)[:, 7:]
    for o, k in ((0, 0), (T, 1)):
        ref[:, o:o + T] += W64["r"][k] * u0[:, o:o + T]
        d = W64["rd"][k] * np.diff(u0[:, o:o + T], axis=1)
        ref[:, o:o + T - 1] -= d
        ref[:, o + 1:o + T] += d
    err, tol = np.abs(r["grad"] - ref).max(), 5e-5 * np.abs(ref).max() + 1e-6
    print(f"[nmpc grad] B={B} T={T} select={select}: err {err:.3e} bound {tol:.3e} max|ref| {np.abs(ref).max():.3e}")
    assert np.isfinite(r["grad"]).all() and err <= tol
    # a start outside the box is clipped, and reported clipped
    far = nmpc.solve(s0.astype(F32), goal.astype(F32), DP, T=T, weights=weights(W), u0=(100.0 * u0).astype(F32),
                     mode=mode_of(select), max_iter=0)
    hi = np.concatenate([np.full(T, DP[10]), np.full(T, DP[9])]).astype(F32)
    assert np.array_equal(far.controls.cpu().numpy(), np.clip((100.0 * u0).astype(F32), -hi, hi))


# ------------------------------------------------------------------ 3. bounds and monotonicity
@pytest.mark.parametrize("select", MODES)
@pytest.mark.parametrize("B,T", [(63, 5), (257, 5), (65, 8), (1, 1)], ids=lambda v: str(v))
def test_sat_rows_stay_in_the_box_and_never_get_worse(gpu, B, T, select):
    r = host(run("sat", B, T, select))
    hi_a, hi_s = F32(DP[10]), F32(DP[9])
    assert (np.abs(r["u"][:, :T]) <= hi_a).all() and (np.abs(r["u"][:, T:]) <= hi_s).all()
    assert (r["cost"] <= r["cost0"]).all() and np.isfinite(r["cost"]).all()
    assert np.isin(r["status"], (nu.CONVERGED, nu.MAX_ITER, nu.STALLED)).all() and (r["iters"] <= nu.DEFAULTS["max_iter"]).all()
    if T == 5:
        on = (np.abs(r["u"][:, :T]) == hi_a).any(1) | (np.abs(r["u"][:, T:]) == hi_s).any(1)
        print(f"[nmpc sat] B={B} select={select}: rows with an active bound {on.sum()} / {B}, "
              f"status counts {np.bincount(r['status'], minlength=4)}")
        assert on.mean() > 0.9


# ------------------------------------------------------------------ 4. reach
def test_reach_comes_down_to_the_float32_floor(gpu):
    """Zero-residual problems (KS, T = 5, 257 rows): final / initial cost, the largest over the rows, against the same figure of
    the float32 run of the reference statement.  The floor is the squared float32 resolution of the states; the kernel's
    sin / cos are good to 2 ulp and its divisions and reciprocal square roots to 1 ulp where NumPy's are correctly rounded
    (1/2 ulp), so its state errors may be 4 x NumPy's and its floor 4^2 = 16 x: the factor is 16.
    Measured on the MI355X: kernel 1.12e-11, float32 statement 3.94e-11 (ratio 0.28; float64 statement 9.75e-29), all 257 rows
    converged."""
    B, T = 257, 5
    r = host(run("reach", B, T, False))
    ref32, ref64 = reference("reach", B, T, False, np.float32), reference("reach", B, T, False, np.float64)
    got = float((r["cost"].astype(np.float64) / r["cost0"]).max())
    bar = float((ref32["cost"].astype(np.float64) / ref32["cost0"]).max())
    print(f"[nmpc reach] final / initial cost: kernel {got:.2e}, float32 statement {bar:.2e}, "
          f"float64 statement {float((ref64['cost'] / ref64['cost0']).max()):.2e}; status counts "
          f"{np.bincount(r['status'], minlength=4)}")
    assert got <= 16.0 * bar
    assert (r["status"] != nu.NONFINITE).all()


# ------------------------------------------------------------------ 5. agreement with the reference
@pytest.mark.parametrize("select", MODES)
@pytest.mark.parametrize("name", ["reg", "stage", "sat"])
def test_final_cost_against_the_float64_reference(gpu, name, select):
    """Every row (257, T = 5, the same max_iter = 30): cost <= float64 reference cost (1 + margin).  The margin is the largest
    relative gap between the float32 and the float64 run of the reference statement, times 4: the kernel's roundings are up to
    4 x those of the float32 NumPy run (2 ulp trigonometry and 1 ulp division against correctly rounded ones).  The gap is taken
    separately over the rows the float64 statement converges and over those it leaves descending at max_iter: the first are
    fixed to tol, the second depend on the path, and one row of one kind must not loosen the bound of the other (on sat, KS, one
    converged row has a gap of 7e-4 where the 202 descending rows stay below 6e-7).  It is not taken per row: the kernel's
    roundings are not NumPy's, so the row that NumPy's float32 run moves most need not be the kernel's.
    Status, reg and stage.  ST_KS (the issue's family): CONVERGED on every row.  ST_SELECT: the float64 statement itself leaves
    2 of the 257 rows at max_iter -- rows that start within SWITCH_BAND = 0.4 m/s of the switch at V = 3 and creep along it (the
    mask is held constant within a linearisation) -- so the literal assertion cannot hold for the rule; held instead: every row
    the float64 statement converges is CONVERGED, and so is every row that starts outside the band (210 of 257)."""
    B, T = 257, 5
    s0 = problem(name, B, T, select)[0]
    r = host(run(name, B, T, select))
    ref32, ref64 = reference(name, B, T, select, np.float32), reference(name, B, T, select, np.float64)
    gaps = np.abs(ref32["cost"].astype(np.float64) - ref64["cost"]) / ref64["cost"]
    conv64 = ref64["status"] == nu.CONVERGED
    margin = np.zeros(B)
    for grp in (conv64, ~conv64):
        if grp.any():
            margin[grp] = 4.0 * gaps[grp].max()
    rel = (r["cost"].astype(np.float64) - ref64["cost"]) / ref64["cost"]
    for what, grp in (("converged", conv64), ("descending", ~conv64)):
        if grp.any():
            print(f"[nmpc agree] {name} select={select} {what} rows ({grp.sum()}): gap of the statement {gaps[grp].max():.2e}, margin "
                  f"{margin[grp].max():.2e}, kernel worst (cost - ref) / ref {rel[grp].max():.2e}, best {rel[grp].min():.2e}")
    print(f"[nmpc agree] {name} select={select}: iterations mean {r['iters'].mean():.1f} max {r['iters'].max()}; status counts "
          f"{np.bincount(r['status'], minlength=4)} (float64: {np.bincount(ref64['status'], minlength=4)})")
    assert (rel <= margin).all()
    if name != "sat":
        got = r["status"] == nu.CONVERGED
        if not select:
            assert conv64.all() and got.all()
        else:
            band = np.abs(s0[:, 3] - 3.0) < SWITCH_BAND
            assert conv64[~band].all()                             # the statement: only rows next to the switch creep
            assert got[conv64].all() and got[~band].all()
            assert np.isin(r["status"][~got], (nu.MAX_ITER, nu.STALLED)).all()


# ------------------------------------------------------------------ 6. row independence
@pytest.mark.parametrize("select", MODES)
def test_rows_do_not_depend_on_how_they_are_cut_into_calls(gpu, select):
    B, T = 257, 5
    s0, goal, W = problem("reg", B, T, select)
    per_car = np.tile(DP.astype(F32), (B, 1))
    call = lambda rows, dp=DP: host(nmpc.solve(s0[rows].astype(F32), goal[rows].astype(F32), dp, T=T, weights=weights(W),
                                               mode=mode_of(select), want_grad=True, **nu.DEFAULTS))
    whole = call(slice(None))
    same_bits(whole, call(slice(None)))
    for lo, hi in ((0, 63), (63, 128), (128, 257)):
        same_bits(whole, call(slice(lo, hi)), rows_a=slice(lo, hi))
    import torch
    same_bits(whole, call(slice(None), torch.from_numpy(per_car).cuda()))     # one parameter row per problem: the same bits


# ------------------------------------------------------------------ 7. isolation
@pytest.mark.parametrize("select", MODES)
def test_a_nonfinite_row_stays_alone(gpu, select):
    B, T = 65, 5
    s0, goal, W = problem("reg", B, T, select)
    rng = np.random.default_rng(9)
    u0 = np.hstack([rng.uniform(-12, 12, (B, T)), rng.uniform(-4, 4, (B, T))]).astype(F32)
    call = lambda s, g, u: host(nmpc.solve(s.astype(F32), g.astype(F32), DP, T=T, weights=weights(W), u0=u, mode=mode_of(select),
                                           want_grad=True, **nu.DEFAULTS))
    clean = call(s0, goal, u0)
    s_bad, g_bad, u_bad = s0.copy(), goal.copy(), u0.copy()
    s_bad[3, 3] = np.nan
    g_bad[40, 0] = np.inf
    u_bad[64, 2] = -np.inf
    dirty = call(s_bad, g_bad, u_bad)
    bad = [3, 40, 64]
    keep = np.setdiff1d(np.arange(B), bad)
    same_bits(clean, dirty, rows_a=keep, rows_b=keep)
    assert (dirty["status"][bad] == nu.NONFINITE).all() and (dirty["status"][keep] != nu.NONFINITE).all()
    assert np.isnan(dirty["cost"][bad]).all() and np.isnan(dirty["cost0"][bad]).all() and (dirty["iters"][bad] == 0).all()
    hi = np.concatenate([np.full(T, DP[10]), np.full(T, DP[9])]).astype(F32)
    assert np.array_equal(dirty["u"][bad], np.clip(u_bad[bad], -hi, hi))       # the clipped start


# ------------------------------------------------------------------ 8. defined statuses
@pytest.mark.parametrize("select", MODES)
def test_degenerate_problems_have_a_defined_status(gpu, select):
    B = 65
    s0, goal, W = problem("reg", B, 1, select)
    zero = nmpc.Weights(q=(0,) * 4, qf=(0,) * 4, r=(0, 0), rd=(0, 0))
    for T in (1, 5):
        g = goal if T == 1 else problem("reg", B, 5, select)[1]
        r = host(nmpc.solve(s0.astype(F32), g.astype(F32), DP, T=T, weights=zero, mode=mode_of(select), want_grad=True))
        assert (r["status"] == nu.CONVERGED).all() and (r["iters"] == 0).all() and (r["cost"] == 0).all() and (r["u"] == 0).all()
        assert (r["grad"] == 0).all()
    r = host(run("reg", B, 1, select))
    ref = reference("reg", B, 1, select, np.float64)
    assert np.isin(r["status"], (nu.CONVERGED, nu.MAX_ITER, nu.STALLED)).all() and np.isfinite(r["cost"]).all()
    assert np.isfinite(r["u"]).all() and (r["cost"] <= r["cost0"]).all()
    print(f"[nmpc T=1] select={select}: status counts {np.bincount(r['status'], minlength=4)} (float64 statement "
          f"{np.bincount(ref['status'], minlength=4)})")
    with pytest.raises(ValueError):
        nmpc.solve(s0.astype(F32), goal.astype(F32), DP, T=9)


# ------------------------------------------------------------------ 9. make_table -> fit
def test_a_label_table_can_be_fitted(gpu, tmp_path):
    """2^12 queries of the reg family -> make_table -> kmeans centres -> closed-form output layer: the fitted net beats the mean
    predictor on the table.  A smoke test of the chain."""
    N, T, K = 4096, 5, 64
    s0, goal, W = nu.family("reg", N, T, seed=77)
    x = np.zeros((N, 7), F32)
    x[:, 0] = s0[:, 3]
    x[:, 1:5] = goal
    path = str(tmp_path / "labels.npz")
    inputs, outputs = nmpc.make_table(x, DP, T=T, weights=weights(W), mode=_lib.ROLLOUT_ST_KS, save=path)
    assert inputs.shape == (N, 7) and outputs.shape == (N, T, 2) and inputs.dtype == F32 and outputs.dtype == F32
    li, lo = tables.load_table(path)
    assert np.array_equal(li, inputs) and np.array_equal(lo, outputs)
    xi, yo, valid = tables.remove_infeasible(inputs, outputs)
    failed = (outputs == tables.INFEASIBLE).all(axis=(1, 2))
    print(f"[nmpc table] {failed.sum()} of {N} rows not converged")
    assert len(valid) == N - failed.sum() and len(valid) > 0.9 * N and (np.abs(yo) <= DP[10]).all()
    y = tables.flatten_outputs(yo)
    km = kmeans.fit(xi, K, max_iter=20, seed=1)
    centers = km.centers.cpu().numpy()
    cfg = dict(in_features=7, out_features=2 * T, num_kernels=K, basis_func="gaussian", num_regions=1, lower_bounds=[[-50.0]] * 7,
               upper_bounds=[[50.0]] * 7, dimension_ranges=[[0] * 7], activation_idx=list(range(7)), delta=[100.0] * 7)
    net = WCRBFNet.from_config(cfg)
    p = net.init()
    p["params"]["rbf_list"]["centers"] = centers[None].astype(F32)
    p["params"]["rbf_list"]["log_sigs"] = np.zeros((1, K), F32)
    new, fit = linear_fit.fit_linear(net, p, xi, y)
    out = np.asarray(net.apply(new, xi), np.float64)
    rms_net = np.sqrt(((out - y) ** 2).mean())
    rms_mean = np.sqrt(((y - y.mean(0)) ** 2).mean())
    print(f"[nmpc table] RMS control error: fitted net {rms_net:.4f}, mean predictor {rms_mean:.4f}")
    assert rms_net < rms_mean


# ------------------------------------------------------------------ 10. closed loop
def test_closed_loop_on_a_straight_line(gpu):
    """16 cars on a straight lattice line at 4 m/s (ST_SELECT: the dynamic branch): 8 start on it, 8 a quarter of a metre beside
    it.  All keep driving and make progress; no car ends farther from the line than it started, and no car's rms deviation
    exceeds its starting one.  On a plant with half the friction the call runs and the cars that steer end elsewhere."""
    import torch
    wp = su.straight_track(120, step=0.5, v=4.0)
    track = simulate.Track(wp, wrap=False, lookahead=2.0, max_reacquire=5.0)
    B = 16
    st = np.zeros((B, 7), F32)
    st[:, 0] = 1.25 + 0.5 * np.arange(B)
    st[:, 1] = 2.0 + np.where(np.arange(B) < 8, 0.0, np.where(np.arange(B) % 2 == 0, 0.25, -0.25))
    st[:, 3] = 4.0
    d0 = np.abs(st[:, 1].astype(np.float64) - 2.0)
    ticks = 30
    res = nmpc.closed_loop(track, st, ticks, DP, T=5, mode=_lib.ROLLOUT_ST_SELECT)
    assert (res.status == _lib.SIM_OK).all() and (res.ticks == ticks + 1).all() and (res.fail_tick == -1).all()
    assert (res.progress > 0).all()
    d1 = (res.state[:, 1].double() - 2.0).abs().cpu().numpy()
    rms = res.rms_dev.cpu().numpy()
    print(f"[nmpc loop] progress {res.progress.min().item():.2f}..{res.progress.max().item():.2f} m, distance from the line "
          f"start {d0.max():.3f} -> end {d1.max():.3f}, rms_dev max {rms.max():.3f}")
    assert (d1 <= d0).all() and (rms <= d0).all()
    assert res.summary()["status"]["ok"] == B
    slick = np.tile(DP.astype(F32), (B, 1))
    slick[:, 0] *= 0.5
    res2 = nmpc.closed_loop(track, st, ticks, DP, plant_params=torch.from_numpy(slick).cuda(), T=5, mode=_lib.ROLLOUT_ST_SELECT)
    assert torch.isfinite(res2.state).all() and (res2.ticks == ticks + 1).all()
    assert torch.equal(res2.state[:8], res.state[:8])              # no steering, no side force: friction does not matter
    assert not torch.equal(res2.state[8:], res.state[8:])
    ks = nmpc.closed_loop(track, st, 5, DP, T=3, n_sub=2, mode=_lib.ROLLOUT_ST_KS, record_every=5)
    assert tuple(ks.states.shape) == (1, B, 7) and torch.equal(ks.states[0], ks.state) and (ks.status == _lib.SIM_OK).all()
