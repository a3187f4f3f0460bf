"""The Frenet NMPC solver (irbfn_nmpc_solve_frenet, K15: nmpc_solve_kernel<FRENET_LS, T>) against the float64 NumPy statement of
its rule (_nmpc_frenet_util.py, held to central differences and the oracle's hand adjoint by test_nmpc_frenet_cpu.py), the roll-out
kernels it shares its step with, and the Python layer on top of it (make_table_frenet, closed_loop_frenet).  It mirrors
test_gpu_nmpc.py test for test.

Shapes: B in {1, 63, 65, 257} (one lane, either side of a wave = a block of this kernel, several blocks), T in {1, 5, 8} (the
smallest, the reference's, the largest instance).  Problem families: _nmpc_frenet_util.family, seed 123 + T."""
import numpy as np
import pytest

from irbfn_amd import _lib, dynamics, kmeans, linear_fit, nmpc, simulate, tables
from irbfn_amd.model import WCRBFNet

import _frenet_sim_util as fs
import _nmpc_frenet_util as fu
import _simulate_util as su

pytestmark = pytest.mark.gpu
F32 = np.float32
FR = _lib.ROLLOUT_FRENET_LS
DP = fu.DP.astype(F32).astype(np.float64)             # what the kernel gets, widened
SHAPES = [(1, 1), (63, 5), (65, 8), (257, 5), (64, 1), (257, 8)]
_cache = {}


def weights(W):
    return nmpc.FrenetWeights(**W)


def problem(name, B, T):
    """(s0, goal, W) of a family, made once and read-only"""
    key = ("p", name, B, T)
    if key not in _cache:
        s0, goal, W = fu.family(name, B, T, seed=123 + T)
        s0.setflags(write=False)
        goal.setflags(write=False)
        _cache[key] = (s0, goal, W)
    return _cache[key]


def reference(name, B, T, ft):
    key = ("r", name, B, T, ft)
    if key not in _cache:
        s0, goal, W = problem(name, B, T)
        _cache[key] = fu.solve(s0, goal, DP, W, T, ft=ft, **fu.DEFAULTS)
    return _cache[key]


def run(name, B, T, **kw):
    s0, goal, W = problem(name, B, T)
    opts = dict(fu.DEFAULTS)
    opts.update(kw)
    return nmpc.solve_frenet(s0.astype(F32), goal.astype(F32), DP, T=T, weights=weights(W), **opts)


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


def rolled_states(s0, u, T):
    """irbfn_rollout_forward(FRENET_LS, [state0 | u]) [B,T,8], the float32 states widened"""
    xu = np.hstack([s0, u]).astype(F32)
    return np.asarray(dynamics.rollout_forward(FR, xu, DP, T), np.float64)


def box(T):
    return np.concatenate([np.full(T, DP[10]), np.full(T, DP[9])]).astype(F32)


# ------------------------------------------------------------------ 1. the cost is the roll-out's
@pytest.mark.parametrize("B,T", SHAPES, ids=lambda v: str(v))
def test_cost_is_the_cost_of_the_rollout_of_the_returned_controls(gpu, B, T):
    """cost[:, 1] against the float64 cost of irbfn_rollout_forward's float32 states for the returned u, within m 2^-23 cost,
    m = 8T - 2 terms: the derivation of test_gpu_nmpc.py term for term (per term the subtraction counted twice, the square and the
    weight, then m - 1 additions and the half; a term with weight 0 is exactly 0 and only makes the bound looser than needed)."""
    s0, goal, W = problem("stage", B, T)
    r = host(run("stage", B, T))
    states = rolled_states(s0, r["u"], T)
    W64 = fu.weights_as(W, np.float64)
    as_st = lambda st: [st[:, t][:, fu.AS_ST] for t in range(T)]
    c64, _, m = fu.cost_from_states(as_st(states), r["u"].astype(np.float64), goal, W64)
    assert m == 8 * T - 2
    err = np.abs(r["cost"] - c64)
    print(f"[frenet nmpc cost] B={B} T={T}: max err / cost {np.max(err / c64):.2e}, bound {m * 2.0 ** -23:.2e}")
    assert (err <= m * 2.0 ** -23 * c64).all()
    u0 = np.zeros((B, 2 * T))
    c0, _, _ = fu.cost_from_states(as_st(rolled_states(s0, u0, T)), u0, goal, W64)
    assert (np.abs(r["cost0"] - c0) <= m * 2.0 ** -23 * c0).all()


# ------------------------------------------------------------------ 2. the gradient
@pytest.mark.parametrize("B,T", SHAPES, ids=lambda v: str(v))
def test_gradient_at_the_start_is_the_rollout_vjp_of_the_residuals(gpu, B, T):
    """max_iter = 0: grad = J^T r at the clipped start, composed here from irbfn_rollout_vjp(FRENET_LS) seeded with the weighted
    residuals (float64 from the float32 states) plus the control terms.  Bound: the Frenet roll-out VJP test's own, per row
    1e-4 max|ref row| + 1e-6 (test_gpu_parity.py: test_rollout_vjps_match_hand_adjoints)."""
    s0, goal, _ = problem("stage", B, T)
    W = dict(q=(0.5, 1, 0.5, 0.1), qf=(10, 10, 5, 1), r=(0.01, 0.1), rd=(0.01, 0.1))      # every residual weighted, s too
    rng = np.random.default_rng(B + T)
    s0 = s0.copy()
    s0[:, 2] = rng.uniform(-0.5, 0.5, B)                           # some rows outside the steering clip
    s0[:, 4:6] = rng.normal(size=(B, 2)) * 0.3
    s0 = s0.astype(F32).astype(np.float64)
    u0 = np.hstack([rng.uniform(-4, 4, (B, T)), rng.uniform(-1.5, 1.5, (B, T))]).astype(F32).astype(np.float64)
    res = nmpc.solve_frenet(s0.astype(F32), goal.astype(F32), DP, T=T, weights=weights(W), u0=u0.astype(F32), max_iter=0,
                            want_grad=True)
    r = host(res)
    assert np.array_equal(r["u"], u0.astype(F32)) and (r["status"] == fu.MAX_ITER).all() and (r["iters"] == 0).all()
    assert r["cost0"].tobytes() == r["cost"].tobytes() and np.isfinite(r["cost"]).all()
    W64 = fu.weights_as(W, np.float64)
    states = rolled_states(s0, u0, T)
    gs = np.zeros((B, T, 8))
    for t in range(T):
        e = fu.residual(states[:, t], goal)
        w = W64["qf"] if t == T - 1 else W64["q"]
        for k in range(4):
            gs[:, t, fu.COMP[k]] = w[k] * e[:, k]
    xu = np.hstack([s0, u0]).astype(F32)
    ref = np.asarray(dynamics.rollout_vjp(FR, xu, DP, gs.astype(F32), T), np.float64)[:, 8:]
    for o, k in ((0, 0), (T, 1)):
        ref[:, o:o + T] += W64["r"][k] * u0[:, o:o + T]
        d = W64["rd"][k] * np.diff(u0[:, o:o + T], axis=1)
        ref[:, o:o + T - 1] -= d
        ref[:, o + 1:o + T] += d
    err = np.abs(r["grad"] - ref)
    tol = 1e-4 * np.abs(ref).max(axis=1, keepdims=True) + 1e-6
    print(f"[frenet nmpc grad] B={B} T={T}: worst err / bound {(err / tol).max():.3e}, max|ref| {np.abs(ref).max():.3e}")
    assert np.isfinite(r["grad"]).all() and (err <= tol).all()
    # a start outside the box is clipped, and reported clipped
    far = nmpc.solve_frenet(s0.astype(F32), goal.astype(F32), DP, T=T, weights=weights(W), u0=(100.0 * u0).astype(F32), max_iter=0)
    assert np.array_equal(far.controls.cpu().numpy(), np.clip((100.0 * u0).astype(F32), -box(T), box(T)))


# ------------------------------------------------------------------ 3. bounds and monotonicity
@pytest.mark.parametrize("B,T", [(63, 5), (257, 5), (65, 8), (1, 1)], ids=lambda v: str(v))
def test_sat_rows_stay_in_the_box_and_never_get_worse(gpu, B, T):
    r = host(run("sat", B, T))
    hi_a, hi_s = F32(DP[10]), F32(DP[9])
    assert (np.abs(r["u"][:, :T]) <= hi_a).all() and (np.abs(r["u"][:, T:]) <= hi_s).all()
    assert (r["cost"] <= r["cost0"]).all() and np.isfinite(r["cost"]).all()
    assert np.isin(r["status"], (fu.CONVERGED, fu.MAX_ITER, fu.STALLED)).all() and (r["iters"] <= fu.DEFAULTS["max_iter"]).all()
    if T == 5:
        on = (np.abs(r["u"][:, :T]) == hi_a).any(1) | (np.abs(r["u"][:, T:]) == hi_s).any(1)
        print(f"[frenet nmpc sat] B={B}: rows with an active bound {on.sum()} / {B}, status counts {np.bincount(r['status'], minlength=4)}")
        assert on.mean() > 0.9


# ------------------------------------------------------------------ 4. reach
def test_reach_comes_down_to_the_float32_floor(gpu):
    """Zero-residual problems (T = 5, 257 rows): final / initial cost, the largest over the rows, against the same figure of the
    float32 run of the statement, within the factor 16 of test_gpu_nmpc.py: test_reach_comes_down_to_the_float32_floor (2-ulp
    trigonometry and 1-ulp division against correctly rounded ones: state errors up to 4 x, squared).  The Frenet step has one
    more division than the single-track one (by 1 - ey curv), an IEEE one in the kernel as in NumPy, so the factor carries over."""
    B, T = 257, 5
    r = host(run("reach", B, T))
    ref32, ref64 = reference("reach", B, T, np.float32), reference("reach", B, T, np.float64)
    got = float((r["cost"].astype(np.float64) / r["cost0"]).max())
    bar = float((ref32["cost"].astype(np.float64) / ref32["cost0"]).max())
    print(f"[frenet nmpc reach] final / initial cost: kernel {got:.2e}, float32 statement {bar:.2e}, float64 statement "
          f"{float((ref64['cost'] / ref64['cost0']).max()):.2e}; status counts {np.bincount(r['status'], minlength=4)}")
    assert got <= 16.0 * bar
    assert (r["status"] != fu.NONFINITE).all()


# ------------------------------------------------------------------ 5. agreement with the reference
@pytest.mark.parametrize("name", ["reg", "stage", "sat"])
def test_final_cost_against_the_float64_reference(gpu, name):
    """Every row (257, T = 5, the same max_iter = 30): cost <= float64 statement's cost (1 + margin), margin = 4 x the largest
    relative gap between the float32 and the float64 run of the statement, taken separately over the rows the float64 statement
    converges and over those it leaves descending at max_iter -- test_gpu_nmpc.py: test_final_cost_against_the_float64_reference,
    word for word.  reg and stage: every row CONVERGED (the statement converges all 257 in both precisions)."""
    B, T = 257, 5
    r = host(run(name, B, T))
    ref32, ref64 = reference(name, B, T, np.float32), reference(name, B, T, np.float64)
    gaps = np.abs(ref32["cost"].astype(np.float64) - ref64["cost"]) / ref64["cost"]
    conv64 = ref64["status"] == fu.CONVERGED
    margin = np.zeros(B)
    for grp in (conv64, ~conv64):
        if grp.any():
            margin[grp] = 4.0 * gaps[grp].max()
    rel = (r["cost"].astype(np.float64) - ref64["cost"]) / ref64["cost"]
    for what, grp in (("converged", conv64), ("descending", ~conv64)):
        if grp.any():
            print(f"[frenet nmpc agree] {name} {what} rows ({grp.sum()}): gap of the statement {gaps[grp].max():.2e}, margin "
                  f"{margin[grp].max():.2e}, kernel worst (cost - ref) / ref {rel[grp].max():.2e}, best {rel[grp].min():.2e}")
    print(f"[frenet nmpc agree] {name}: iterations mean {r['iters'].mean():.1f} max {r['iters'].max()}; status counts "
          f"{np.bincount(r['status'], minlength=4)} (float64: {np.bincount(ref64['status'], minlength=4)})")
    assert (rel <= margin).all()
    if name != "sat":
        assert conv64.all() and (r["status"] == fu.CONVERGED).all()


# ------------------------------------------------------------------ 6. row independence
def test_rows_do_not_depend_on_how_they_are_cut_into_calls(gpu):
    import torch
    B, T = 257, 5
    s0, goal, W = problem("reg", B, T)
    per_car = np.tile(DP.astype(F32), (B, 1))
    call = lambda rows, dp=DP: host(nmpc.solve_frenet(s0[rows].astype(F32), goal[rows].astype(F32), dp, T=T, weights=weights(W),
                                                      want_grad=True, **fu.DEFAULTS))
    whole = call(slice(None))
    same_bits(whole, call(slice(None)))
    for lo, hi in ((0, 1), (1, 64), (64, 65), (65, 257)):          # cut at 1, 64 and 65
        same_bits(whole, call(slice(lo, hi)), rows_a=slice(lo, hi))
    same_bits(whole, call(slice(None), torch.from_numpy(per_car).cuda()))     # one parameter row per problem: the same bits


# ------------------------------------------------------------------ 7. isolation
def test_a_bad_row_stays_alone(gpu):
    """a NaN, an Inf and two rows outside the frame (beyond the centre of curvature, and on it) in one wave and in the next
    block: NONFINITE, NaN costs, the clipped start; every other row keeps the bits of the run without them"""
    B, T = 65, 5
    s0, goal, W = problem("reg", B, T)
    rng = np.random.default_rng(9)
    u0 = np.hstack([rng.uniform(-12, 12, (B, T)), rng.uniform(-4, 4, (B, T))]).astype(F32)
    call = lambda s, g, u: host(nmpc.solve_frenet(s.astype(F32), g.astype(F32), DP, T=T, weights=weights(W), u0=u, want_grad=True,
                                                  **fu.DEFAULTS))
    clean = call(s0, goal, u0)
    s_bad, g_bad, u_bad = s0.copy(), goal.copy(), u0.copy()
    s_bad[3, 3] = np.nan
    g_bad[40, 3] = np.inf
    u_bad[64, 2] = -np.inf
    s_bad[17, 1], s_bad[17, 7] = 4.0, 0.3                          # ey curv = 1.2
    s_bad[33, 1], s_bad[33, 7] = -2.0, -0.5                        # ey curv = 1
    dirty = call(s_bad, g_bad, u_bad)
    bad = [3, 17, 33, 40, 64]
    keep = np.setdiff1d(np.arange(B), bad)
    same_bits(clean, dirty, rows_a=keep, rows_b=keep)
    assert (dirty["status"][bad] == fu.NONFINITE).all() and (dirty["status"][keep] != fu.NONFINITE).all()
    assert np.isnan(dirty["cost"][bad]).all() and np.isnan(dirty["cost0"][bad]).all() and (dirty["iters"][bad] == 0).all()
    assert np.array_equal(dirty["u"][bad], np.clip(u_bad[bad], -box(T), box(T)))       # the clipped start


def test_rows_next_to_the_centre_of_curvature_stay_inside_the_frame(gpu):
    """_nmpc_frenet_util.edge_family, 256 rows, T = 5: a quarter of the rows leave the frame with the controls at rest and trial
    steps of others do.  Held exactly, through irbfn_rollout_forward's float32 states (the kernel's own bits): a row is
    NONFINITE if and only if its roll-out at rest starts a step from 1 - ey curv <= 0 (float32, no fused product), and every
    other row's result is finite, no worse than its start, and its roll-out starts every step inside."""
    B, T = 256, 5
    s0, goal, W = fu.edge_family(B)
    r = host(nmpc.solve_frenet(s0.astype(F32), goal.astype(F32), DP, T=T, weights=weights(W), **fu.DEFAULTS))

    def inside(u):
        st = np.asarray(dynamics.rollout_forward(FR, np.hstack([s0, u]).astype(F32), DP, T), F32)
        starts = np.concatenate([s0.astype(F32)[:, None], st[:, :-1]], axis=1)
        with np.errstate(invalid="ignore", over="ignore"):
            return ((F32(1) - starts[:, :, 1] * starts[:, :, 7]) > 0).all(axis=1)
    out = r["status"] == fu.NONFINITE
    ref64 = fu.solve(s0, goal, DP, W, T, **fu.DEFAULTS)
    print(f"[frenet nmpc edge] status counts {np.bincount(r['status'], minlength=4)} (float64 statement "
          f"{np.bincount(ref64['status'], minlength=4)})")
    assert np.array_equal(out, ~inside(np.zeros((B, 2 * T), F32)))
    assert out.sum() >= 10 and (~out).sum() >= 10
    assert np.isfinite(r["cost"][~out]).all() and (r["cost"][~out] <= r["cost0"][~out]).all()
    assert inside(r["u"])[~out].all()
    assert np.isnan(r["cost"][out]).all() and (r["u"][out] == 0).all() and (r["iters"][out] == 0).all()


# ------------------------------------------------------------------ 8. argument checks and defined statuses
def test_argument_checks_and_degenerate_problems(gpu):
    import ctypes as C
    import torch
    B, T = 65, 5
    s0, goal, W = problem("reg", B, T)
    sd, gd = torch.from_numpy(s0.astype(F32)).cuda(), torch.from_numpy(goal.astype(F32)).cuda()
    u = torch.full((B, 2 * T), 7.0, dtype=torch.float32, device="cuda")
    cost = torch.full((B, 2), 7.0, dtype=torch.float32, device="cuda")
    info = torch.full((B, 2), 7, dtype=torch.int32, device="cuda")
    lib = _lib.load()
    dp = (C.c_float * 13)(*DP)
    mk = lambda: nmpc._options(weights(W), 30, 1e-3, 1e-9, 1e6, 1e-6, 1e-6)
    call = lambda T=T, o=None, B=B: lib.irbfn_nmpc_solve_frenet(T, sd.data_ptr(), gd.data_ptr(), None, dp, None, o, u.data_ptr(),
                                                                cost.data_ptr(), info.data_ptr(), None, B, None)
    ok = mk()
    assert call(T=0, o=C.byref(ok)) == -2 and call(T=9, o=C.byref(ok)) == -2
    neg = mk()
    neg.qf[1] = -1.0
    order = mk()
    order.lambda_min, order.lambda_max = 2.0, 1.0
    assert call(o=C.byref(neg)) == -1 and call(o=None) == -1 and call(o=C.byref(order)) == -1
    assert call(o=C.byref(ok), B=0) == 0
    torch.cuda.synchronize()
    assert (u == 7.0).all() and (cost == 7.0).all() and (info == 7).all()      # nothing was launched
    with pytest.raises(ValueError):
        nmpc.solve_frenet(sd, gd, DP, T=9)
    zero = nmpc.FrenetWeights(q=(0,) * 4, qf=(0,) * 4, r=(0, 0), rd=(0, 0))
    r = host(nmpc.solve_frenet(sd, gd, DP, T=T, weights=zero, want_grad=True))
    assert (r["status"] == fu.CONVERGED).all() and (r["iters"] == 0).all() and (r["cost"] == 0).all() and (r["u"] == 0).all()
    assert (r["grad"] == 0).all()


# ------------------------------------------------------------------ 9. make_table_frenet -> fit
def test_a_frenet_label_table_can_be_fitted(gpu, tmp_path):
    """2^12 queries of the reg family laid out as the Frenet planner's queries -> make_table_frenet -> kmeans centres ->
    closed-form output layer of an 8-input, 2T-output net: on held-out rows the fitted net beats the mean predictor.  The two
    figures are printed here; a test does not rewrite a tracked file, so profiles/nmpc_frenet.txt gets them from the `table` step of
    tools/nmpc_frenet_timing.py, which runs this chain (measured: 0.6023 against 2.5497, 1 of 4096 rows not converged)."""
    N, T, K = 4096, 5, 64
    s0, goal, W = fu.family("reg", N, T, seed=77)
    x = np.zeros((N, 8), F32)
    x[:, 0:3], x[:, 4], x[:, 6:8] = s0[:, 1:4], goal[:, 3], s0[:, 6:8]
    st, gl = nmpc.frenet_query_problem(x)
    assert np.array_equal(st, s0.astype(F32)) and np.array_equal(gl, goal.astype(F32))
    path = str(tmp_path / "labels.npz")
    inputs, outputs = nmpc.make_table_frenet(x, DP, T=T, weights=weights(W), save=path)
    assert inputs.shape == (N, 8) and outputs.shape == (N, T, 2) and inputs.dtype == F32 and outputs.dtype == F32
    li, lo = tables.load_table(path)
    assert np.array_equal(li, inputs) and np.array_equal(lo, outputs)
    xi, yo, valid = tables.remove_infeasible(inputs, outputs)
    failed = (outputs == tables.INFEASIBLE).all(axis=(1, 2))
    print(f"[frenet nmpc table] {failed.sum()} of {N} rows not converged")
    assert len(valid) == N - failed.sum() and len(valid) >= 0.95 * N and (np.abs(yo) <= DP[10]).all()
    y = tables.flatten_outputs(yo)
    n_fit = (3 * len(xi)) // 4                                     # the last quarter is held out
    km = kmeans.fit(xi[:n_fit], K, max_iter=20, seed=1)
    centers = km.centers.cpu().numpy()
    cfg = dict(in_features=8, out_features=2 * T, num_kernels=K, basis_func="gaussian", num_regions=1, lower_bounds=[[-50.0]] * 8,
               upper_bounds=[[50.0]] * 8, dimension_ranges=[[0] * 8], activation_idx=list(range(8)), delta=[100.0] * 8)
    net = WCRBFNet.from_config(cfg)
    p = net.init()
    p["params"]["rbf_list"]["centers"] = centers[None].astype(F32)
    p["params"]["rbf_list"]["log_sigs"] = np.zeros((1, K), F32)
    new, fit = linear_fit.fit_linear(net, p, xi[:n_fit], y[:n_fit])
    out = np.asarray(net.apply(new, xi[n_fit:]), np.float64)
    rms_net = np.sqrt(((out - y[n_fit:]) ** 2).mean())
    rms_mean = np.sqrt(((y[n_fit:] - y[:n_fit].mean(0)) ** 2).mean())
    print(f"[frenet nmpc table] held-out RMS control error: fitted net {rms_net:.4f}, mean predictor {rms_mean:.4f}")
    assert rms_net < rms_mean


# ------------------------------------------------------------------ 10. closed loop
def _seeded(track, s, B):
    """B kinematic cars at 3 m/s at arc lengths s: lateral offsets in +-0.3 m, heading offsets in +-0.1 rad, none of them 0"""
    k = np.arange(B)
    ey = np.where(k % 2 == 0, 1.0, -1.0) * (0.06 + 0.24 * k / (B - 1))
    epsi = np.where(k % 4 < 2, 1.0, -1.0) * (0.02 + 0.08 * ((k * 7) % B) / (B - 1))
    x, y, psi = track.pose_at(s, ey, epsi)
    return fs.ks_state(x, y, psi, 0.0, 3.0).astype(F32), ey


def _hand_loop(track, st, ticks, T, mode):
    """closed_loop_frenet written out: advance_frenet + solve_frenet per tick -> (state, status)"""
    import torch
    B = st.shape[0]
    state = torch.from_numpy(st).cuda().clone()
    seg = track.seed(state[:, :2].double()).contiguous()
    status = torch.zeros(B, dtype=torch.int32, device="cuda")
    rec = simulate.new_record(B, torch)
    x = torch.zeros((B, 8), dtype=torch.float32, device="cuda")
    m = torch.zeros(B, dtype=torch.int32, device="cuda")
    pose = torch.zeros((B, 8), dtype=torch.float64, device="cuda")
    goal = torch.zeros((B, 4), dtype=torch.float64, device="cuda")
    simulate.advance_frenet(track, state, seg, status, rec, x, m, mode=mode, tick=0, frenet_out=pose, goal_out=goal)
    warm = None
    for k in range(ticks):
        s8 = pose.float()
        s8[:, 0] = 0.0
        g4 = torch.zeros((B, 4), dtype=torch.float32, device="cuda")
        g4[:, 3] = goal[:, 3].float()
        ctrl = nmpc.solve_frenet(s8, g4, DP, T=T, u0=warm).controls
        simulate.advance_frenet(track, state, seg, status, rec, x, m, controls=ctrl, plant_params=DP, mode=mode, tick=k + 1,
                                frenet_out=pose, goal_out=goal)
        warm = nmpc.shift_controls(ctrl, T)
    return state, status


def test_closed_loop_on_a_straight_line_and_on_a_circle(gpu):
    """16 kinematic cars (ST_KS plant) at the line's 3 m/s, 60 ticks.  Straight line: every car keeps driving and ends nearer
    the line than it started; the loop written out by hand gives the same bits.  Circle of radius 10 m (a 400-gon): every car
    keeps driving and every figure is finite; the deviations are printed, not judged."""
    import torch
    B, ticks, T, mode = 16, 60, 5, _lib.ROLLOUT_ST_KS
    track = simulate.Track(su.straight_track(120, step=0.5, v=3.0), wrap=False, lookahead=2.0, max_reacquire=5.0)
    st, ey0 = _seeded(track, 2.0 + 0.5 * np.arange(B), B)
    res = nmpc.closed_loop_frenet(track, st, ticks, DP, T=T, mode=mode)
    assert (res.status == _lib.SIM_OK).all() and (res.ticks == ticks + 1).all() and (res.fail_tick == -1).all()
    assert (res.progress > 0).all() and res.summary()["status"]["ok"] == B
    d1 = (res.state[:, 1].double() - 2.0).abs().cpu().numpy()
    print(f"[frenet nmpc loop] straight: |ey| start {np.abs(ey0).min():.3f}..{np.abs(ey0).max():.3f} -> end {d1.min():.2e}..{d1.max():.2e}, "
          f"progress {res.progress.min().item():.2f}..{res.progress.max().item():.2f} m")
    assert (d1 < np.abs(ey0)).all()
    state, status = _hand_loop(track, st, ticks, T, mode)
    assert torch.equal(state.view(torch.int32), res.state.view(torch.int32)) and torch.equal(status, res.status)
    rec = nmpc.closed_loop_frenet(track, st, 5, DP, T=3, n_sub=2, mode=mode, record_every=5)
    assert tuple(rec.states.shape) == (1, B, 7) and torch.equal(rec.states[0], rec.state) and (rec.status == _lib.SIM_OK).all()
    circle = simulate.Track(fs.ngon(400, 10.0), wrap=True, lookahead=2.0, max_reacquire=5.0)
    sc, eyc = _seeded(circle, 1.0 + 1.5 * np.arange(B), B)
    rc = nmpc.closed_loop_frenet(circle, sc, ticks, DP, T=T, mode=mode)
    fr = simulate.to_frenet(circle, rc.state)[0].cpu().numpy()
    print(f"[frenet nmpc loop] circle R = 10 m: |ey| start {np.abs(eyc).min():.3f}..{np.abs(eyc).max():.3f} -> end "
          f"{np.abs(fr[:, 1]).min():.2e}..{np.abs(fr[:, 1]).max():.2e}, rms_dev max {rc.rms_dev.max().item():.3f}, "
          f"|epsi| end max {np.abs(fr[:, 6]).max():.3f}")
    assert (rc.status == _lib.SIM_OK).all() and torch.isfinite(rc.state).all()
    for v in (rc.rms_dev, rc.max_dev, rc.mean_abs_dv, rc.progress, rc.laps):
        assert torch.isfinite(v).all()
