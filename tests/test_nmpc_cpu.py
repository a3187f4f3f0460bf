"""The batched NMPC solver without a GPU: the float64 statements of _nmpc_util.py against central differences and the oracle's
hand adjoints, the reference solver on the problem families, every argument check of irbfn_amd.nmpc and of the C entry point,
and the -999 fill of a label table."""
import ctypes as C

import numpy as np
import pytest

from irbfn_amd import _lib, nmpc, tables
from oracle import hand_vjp

import _nmpc_util as nu
import _st_select_util as ss

MODES = [pytest.param(False, id="ks"), pytest.param(True, id="select")]


def _probe_states():
    """states on either side of the switch at V = 3, inside and outside the clips of delta (0.4189) and V (7)"""
    rng = np.random.default_rng(5)
    rows = []
    for v in (-8.0, -2.0, 0.7, 2.9, 3.1, 5.0, 6.9, 7.5):
        for d in (-0.6, -0.3, 0.05, 0.4, 0.5):
            rows.append([rng.normal(), rng.normal(), d, v, rng.uniform(-3, 3), 0.5 * rng.normal(), 0.1 * rng.normal()])
    return np.array(rows)


@pytest.mark.parametrize("select", MODES)
def test_step_jacobian_against_central_differences(select):
    s = _probe_states()
    B = s.shape[0]
    rng = np.random.default_rng(6)
    a, sv = rng.uniform(-9, 9, B), rng.uniform(-3, 3, B)          # inside the control box
    Fx, Fa, Fsv = nu.step_jacobian(s, a, nu.DP, select)
    h = 1e-6
    worst = 0.0
    for j in range(9):
        sp, sm, ap, am, vp, vm = s.copy(), s.copy(), a.copy(), a.copy(), sv.copy(), sv.copy()
        if j < 7:
            sp[:, j] += h
            sm[:, j] -= h
            col = Fx[:, :, j]
        elif j == 7:
            ap, am, col = a + h, a - h, Fa
        else:
            vp, vm, col = sv + h, sv - h, Fsv
        fd = (nu.step(sp, ap, vp, nu.DP, select) - nu.step(sm, am, vm, nu.DP, select)) / (2 * h)
        err = np.abs(fd - col) / (1.0 + np.abs(col))
        worst = max(worst, float(err.max()))
    print(f"select={select}: worst |fd - J| / (1 + |J|) = {worst:.2e}")
    # central differences at h = 1e-6: truncation h^2 f''' / 6 and rounding 2^-53 |s'| / h, both below 1e-8 for these states
    assert worst < 1e-7


@pytest.mark.parametrize("select", MODES)
@pytest.mark.parametrize("T", [1, 5, 8])
def test_gradient_is_the_hand_adjoint_of_the_residuals(select, T):
    """g = J^T r from the forward sensitivities == the oracle's reverse-mode adjoints seeded with the weighted residuals"""
    B = 64
    rng = np.random.default_rng(7 + T)
    s0, goal, _ = nu.family("stage", B, T, seed=11 + T, select=select)
    s0[:, 2] = rng.uniform(-0.5, 0.5, B)                          # some rows outside the steering clip
    s0[:, 4:] = rng.normal(size=(B, 3)) * [1.0, 0.5, 0.1]
    u = np.hstack([rng.uniform(-9, 9, (B, T)), rng.uniform(-3, 3, (B, T))])
    W = nu.weights_as(nu.WEIGHTS["stage"], np.float64)
    c, g, H = nu.linearize(u, s0, goal, nu.DP, W, select)
    states = nu.rollout(u, s0, nu.DP, select)
    gs = np.zeros((B, T, 7))
    for t in range(T):
        e = nu.residual(states[t], goal)
        w = W["qf"] if t == T - 1 else W["q"]
        for k in range(4):
            gs[:, t, nu.COMP[k]] = w[k] * e[:, k]
    xu = np.hstack([s0, u])
    back = ss.vjp_st_select(xu, nu.DP, gs, 0.5, np.float64, True) if select else hand_vjp.vjp_st_ks(xu, nu.DP, gs, 0.5)
    want = back[:, 7:].copy()
    for o, k in ((0, 0), (T, 1)):
        want[:, o:o + T] += W["r"][k] * u[:, o:o + T]
        d = W["rd"][k] * np.diff(u[:, o:o + T], axis=1)
        want[:, o:o + T - 1] -= d
        want[:, o + 1:o + T] += d
    scale = np.abs(want).max(axis=1, keepdims=True)
    assert (np.abs(g - want) <= 1e-12 * scale).all(), float((np.abs(g - want) / scale).max())
    assert np.isfinite(H).all() and np.abs(H - np.swapaxes(H, 1, 2)).max() <= 1e-12 * np.abs(H).max()
    assert np.allclose(c, nu.cost(u, s0, goal, nu.DP, W, select), rtol=0, atol=0)


def test_reference_reaches_zero_on_reach():
    """Zero-residual problems: Gauss-Newton steps lower the cost by orders of magnitude each, so a row that stops (tol = 1e-6 or 30
    iterations) has come down to rounding.  Bar: 1e-9 of the initial cost in float64, 1e-7 in float32 (2^-24 ~ 6e-8 relative
    state errors squared would give 4e-15; the bar leaves room for the rows that end at max_iter)."""
    s0, goal, W = nu.family("reach", 512, 5, seed=123)
    for ft, bar in ((np.float64, 1e-9), (np.float32, 1e-7)):
        r = nu.solve(s0, goal, nu.DP, W, 5, False, ft=ft)
        ratio = (r["cost"] / r["cost0"]).max()
        print(f"{ft.__name__}: final / initial cost <= {ratio:.2e}, status counts {np.bincount(r['status'], minlength=4)}")
        assert ratio <= bar
        assert (r["status"] != nu.NONFINITE).all()


@pytest.mark.parametrize("select", MODES)
@pytest.mark.parametrize("name", ["reach", "reg", "stage", "sat"])
def test_reference_cost_never_rises_and_stays_in_the_box(name, select):
    s0, goal, W = nu.family(name, 128, 5, seed=123, select=select)
    r = nu.solve(s0, goal, nu.DP, W, 5, select, history=True)
    assert (np.diff(r["costs"], axis=0) <= 0).all()
    assert (np.abs(r["u"][:, :5]) <= nu.DP[10]).all() and (np.abs(r["u"][:, 5:]) <= nu.DP[9]).all()
    assert np.array_equal(r["costs"][-1], r["cost"]) and np.array_equal(r["costs"][0], r["cost0"])
    if name in ("reg", "stage") and not select:
        assert (r["status"] == nu.CONVERGED).all() and r["iters"].max() <= 8
    if name == "sat":
        on = (np.abs(r["u"][:, :5]) == nu.DP[10]).any(1) | (np.abs(r["u"][:, 5:]) == nu.DP[9]).any(1)
        assert on.all()                                           # every row has an active bound


def test_one_sided_convergence_test_stalls_float32_rows():
    """Why the rule tests |c - c+| <= tol c on rejected steps too.  With the test on accepted steps only (c - c+ <= tol c), a
    float32 row at its minimum moves by rounding alone: trial steps that come out an ulp higher are rejected, lambda climbs to
    lambda_max and the row is called stalled, although the float64 run of the same rule converges it.  512 reg rows, KS, T = 5:
    the two-sided rule converges every row in both precisions; the one-sided one converges every float64 row and stalls float32
    rows (69 when this was written) whose costs the two-sided rule reaches to float32 rounding."""
    s0, goal, W = nu.family("reg", 512, 5, seed=123)
    two32 = nu.solve(s0, goal, nu.DP, W, 5, False, ft=np.float32)
    one32 = nu.solve(s0, goal, nu.DP, W, 5, False, ft=np.float32, two_sided=False)
    one64 = nu.solve(s0, goal, nu.DP, W, 5, False, two_sided=False)
    two64 = nu.solve(s0, goal, nu.DP, W, 5, False)
    stalled = one32["status"] == nu.STALLED
    print(f"one-sided float32: status counts {np.bincount(one32['status'], minlength=4)}; two-sided float32: "
          f"{np.bincount(two32['status'], minlength=4)}")
    assert (two32["status"] == nu.CONVERGED).all() and (two64["status"] == nu.CONVERGED).all()
    assert (one64["status"] == nu.CONVERGED).all()
    assert stalled.sum() >= 10 and (one32["status"][~stalled] == nu.CONVERGED).all()
    # the stalled rows were at their minimum: the two-sided rule ends within float32 rounding of the same cost
    rel = np.abs(two32["cost"].astype(np.float64) - one32["cost"]) / one32["cost"]
    print(f"stalled rows: two-sided against one-sided final cost, largest relative difference {rel[stalled].max():.2e}")
    assert rel[stalled].max() <= 38 * 2.0 ** -23                  # m = 8T - 2 terms, as the cost test of the kernel


def test_select_rows_that_do_not_converge_start_next_to_the_switch():
    """ST_SELECT, reg and stage, the rows of test_gpu_nmpc.py: the float64 statement leaves a few rows at max_iter; all of them
    start within 0.4 m/s of the switch at V = 3 (test_gpu_nmpc.SWITCH_BAND), and they are few."""
    B, T = 257, 5
    for name in ("reg", "stage"):
        s0, goal, W = nu.family(name, B, T, seed=123 + B + T, select=True)
        dp = nu.DP.astype(np.float32).astype(np.float64)
        r = nu.solve(s0, goal, dp, W, T, True)
        bad = r["status"] != nu.CONVERGED
        print(f"{name}: {bad.sum()} of {B} rows not converged, start speeds {s0[bad, 3]}")
        assert (np.abs(s0[bad, 3] - 3.0) < 0.4).all() and bad.sum() <= B // 50


def test_reference_statuses_of_degenerate_rows():
    s0, goal, W = nu.family("reg", 8, 1, seed=3)
    zero = dict(q=(0,) * 4, qf=(0,) * 4, r=(0, 0), rd=(0, 0))
    r = nu.solve(s0, goal, nu.DP, zero, 1, False)
    assert (r["status"] == nu.CONVERGED).all() and (r["iters"] == 0).all() and (r["cost"] == 0).all()
    r = nu.solve(s0, goal, nu.DP, W, 1, False)
    assert np.isin(r["status"], (nu.CONVERGED, nu.MAX_ITER, nu.STALLED)).all() and np.isfinite(r["cost"]).all()
    s0[2, 3] = np.nan
    goal[5, 0] = np.inf
    r = nu.solve(s0, goal, nu.DP, W, 1, False)
    assert list(np.where(r["status"] == nu.NONFINITE)[0]) == [2, 5]
    assert np.isnan(r["cost"][[2, 5]]).all() and np.isfinite(np.delete(r["cost"], [2, 5])).all()


# ------------------------------------------------------------------ argument checks, no GPU
def _ok(B=3, T=5):
    return np.zeros((B, 7), np.float32), np.zeros((B, 4), np.float32), nu.DP


def test_python_side_validation_errors():
    s0, goal, dp = _ok()
    bad = [
        (dict(state0=np.zeros((3, 6))), "state0"),
        (dict(state0=np.zeros(7)), "state0"),
        (dict(goal=np.zeros((3, 3))), "goal"),
        (dict(goal=np.zeros((2, 4))), "goal"),
        (dict(u0=np.zeros((3, 8))), "u0"),
        (dict(dyn_params=None), "dyn_params"),
        (dict(dyn_params=np.zeros(12)), "dyn_params"),
        (dict(dyn_params=np.zeros((2, 13))), "dyn_params"),
        (dict(T=0), "horizon"),
        (dict(T=9), "horizon"),
        (dict(T=2.5), "horizon"),
        (dict(mode=_lib.ROLLOUT_FULLINT), "model"),
        (dict(max_iter=-1), "max_iter"),
        (dict(max_iter=1.5), "max_iter"),
        (dict(lambda0=-1.0), "lambda0"),
        (dict(lambda_min=float("nan")), "lambda_min"),
        (dict(lambda_min=1.0, lambda_max=0.5), "lambda_min"),
        (dict(tol=float("inf")), "tol"),
        (dict(eps=-1e-6), "eps"),
        (dict(weights=nmpc.Weights(q=(1, 1, 1))), "weights.q"),
        (dict(weights=nmpc.Weights(qf=(1, 1, -1, 1))), "weights.qf"),
        (dict(weights=nmpc.Weights(r=(float("nan"), 0))), "weights.r"),
        (dict(weights=nmpc.Weights(rd=(0, float("inf")))), "weights.rd"),
    ]
    for kw, word in bad:
        args = dict(state0=s0, goal=goal, dyn_params=dp)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            nmpc.solve(**args)
    with pytest.raises(TypeError, match="Weights"):
        nmpc.solve(s0, goal, dp, weights=dict(q=(1, 1, 1, 1)))
    with pytest.raises(ValueError, match="queries"):
        nmpc.solve_queries(np.zeros((3, 6)), dp)
    with pytest.raises(TypeError, match="Track"):
        nmpc.closed_loop(object(), s0, 3, dp)
    from irbfn_amd.simulate import Track
    import _simulate_util as su
    tr = Track(su.straight_track(10), wrap=False)
    for kw, word in ((dict(ticks=-1), "ticks"), (dict(n_sub=0), "ticks"), (dict(T=9), "horizon"), (dict(max_iter=-2), "max_iter"),
                     (dict(plant_params=np.zeros((2, 13))), "plant_params")):
        args = dict(track=tr, state0=s0, ticks=3, dyn_params=dp)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            nmpc.closed_loop(**args)
    with pytest.raises(ValueError, match="state0"):
        nmpc.closed_loop(tr, np.zeros((3, 5)), 3, dp)
    for kw in (dict(u0=np.zeros((3, 10))), dict(want_grad=True), dict(nonsense=1)):
        with pytest.raises(TypeError, match="closed_loop"):
            nmpc.closed_loop(tr, s0, 3, dp, **kw)


def test_c_entry_point_decides_bad_arguments_before_any_launch():
    lib = _lib.load()
    opt = nmpc._options(nmpc.Weights(), 30, 1e-3, 1e-9, 1e6, 1e-6, 1e-6)
    one = C.c_void_p(64)                                          # never dereferenced: every call below returns before a launch
    dp = (C.c_float * 13)(*nu.DP)
    call = lambda mode=_lib.ROLLOUT_ST_KS, T=5, s=one, g=one, dh=dp, dd=None, o=C.byref(opt), u=one, c=one, i=one, B=4: \
        lib.irbfn_nmpc_solve(mode, T, s, g, None, dh, dd, o, u, c, i, None, B, None)
    assert call(B=0) == 0
    assert call(B=0, s=None, g=None, u=None, c=None, i=None, dh=None) == 0
    assert call(B=-1) == -1
    assert call(mode=_lib.ROLLOUT_FRENET_LS) == -1 and call(mode=99) == -1
    assert call(o=None) == -1
    for T in (0, 9, -3):
        assert call(T=T) == -2
    for name in ("s", "g", "u", "c", "i"):
        assert call(**{name: None}) == -1
    assert call(dh=None) == -1
    for field, v in (("lambda0", -1.0), ("lambda_min", float("nan")), ("lambda_max", float("inf")), ("tol", -1e-3), ("eps", -1.0)):
        o2 = nmpc._options(nmpc.Weights(), 30, 1e-3, 1e-9, 1e6, 1e-6, 1e-6)
        setattr(o2, field, v)
        assert call(o=C.byref(o2)) == -1, field
    for field, n in (("q", 4), ("qf", 4), ("r", 2), ("rd", 2)):
        for v in (-1.0, float("nan"), float("inf")):
            o2 = nmpc._options(nmpc.Weights(), 30, 1e-3, 1e-9, 1e6, 1e-6, 1e-6)
            getattr(o2, field)[n - 1] = v
            assert call(o=C.byref(o2)) == -1, (field, v)
    o2 = nmpc._options(nmpc.Weights(), 30, 1e-3, 1e-9, 1e6, 1e-6, 1e-6)
    o2.lambda_min, o2.lambda_max = 2.0, 1.0
    assert call(o=C.byref(o2)) == -1
    o2 = nmpc._options(nmpc.Weights(), 30, 1e-3, 1e-9, 1e6, 1e-6, 1e-6)
    o2.max_iter = -1
    assert call(o=C.byref(o2)) == -1
    assert C.sizeof(_lib.NmpcOptions) == 18 * 4


# ------------------------------------------------------------------ label tables
def test_query_problem_follows_the_training_convention():
    x = np.arange(14, dtype=np.float32).reshape(2, 7) + 1          # [v, x_g, y_g, th_g, v_g, beta, psi_dot]
    s0, goal = nmpc.query_problem(x)
    assert np.array_equal(s0, [[0, 0, 0, 1, 0, 7, 6], [0, 0, 0, 8, 0, 14, 13]])
    assert np.array_equal(goal, x[:, 1:5]) and s0.dtype == np.float32


def test_infeasible_fill_and_round_trip_through_load_table(tmp_path):
    T = 5
    rng = np.random.default_rng(2)
    u = rng.normal(size=(6, 2 * T)).astype(np.float32)
    ok = np.array([True, False, True, True, False, True])
    x = rng.normal(size=(6, 7)).astype(np.float32)
    out = nmpc.fill_infeasible(u, ok)
    assert out.shape == (6, T, 2) and out.dtype == np.float32
    assert (out[~ok] == tables.INFEASIBLE).all()
    assert np.array_equal(out[ok][:, :, 0], u[ok][:, :T]) and np.array_equal(out[ok][:, :, 1], u[ok][:, T:])
    assert np.array_equal(tables.flatten_outputs(out)[ok], u[ok])
    path = str(tmp_path / "table.npz")
    np.savez(path, inputs=x, outputs=out)
    xi, yo = tables.load_table(path, drop_infeasible=True)
    assert np.array_equal(xi, x[ok]) and np.array_equal(yo, out[ok])
    xi, yo = tables.load_table(path)                               # the Cartesian trainer keeps every row
    assert xi.shape[0] == 6
    mi, mo = tables.mirror(xi, yo)
    assert mi.shape[0] == 12 and np.array_equal(mo[6:, :, 1], -yo[:, :, 1])
