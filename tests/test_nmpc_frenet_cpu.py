"""The Frenet NMPC solver (K15) without a GPU: the float64 statements of _nmpc_frenet_util.py against central differences and
the oracle's hand adjoint, the statement's convergence on the problem families, the frame guard, the query convention and every
argument check of irbfn_amd.nmpc's Frenet layer and of the C entry point."""
import ctypes as C
import os

import numpy as np
import pytest

from irbfn_amd import _lib, nmpc
from oracle import hand_vjp

import _nmpc_frenet_util as fu

DP32 = fu.DP.astype(np.float32).astype(np.float64)      # what the kernel gets, widened
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _probe_states():
    """states inside and outside the clip of delta (0.4189), on both sides of the line, on left and right bends, slow and fast"""
    rng = np.random.default_rng(5)
    rows = []
    for vx in (-2.0, 0.7, 3.0, 6.5):
        for d in (-0.6, -0.3, 0.05, 0.4, 0.5):
            for cur in (-0.3, 0.0, 0.25):
                rows.append([rng.normal(), rng.uniform(-0.8, 0.8), d, vx, 0.3 * rng.normal(), 0.3 * rng.normal(),
                             rng.uniform(-1.2, 1.2), cur])
    return np.array(rows)


def test_step_jacobian_against_central_differences():
    """all seven state columns that a step reads or moves (s, ey, delta, vx, epsi) and the two controls; vy, wz and curv are not
    columns of the sensitivities, the first two because no entry depends on them, curv because it never moves"""
    s = _probe_states()
    B = s.shape[0]
    rng = np.random.default_rng(6)
    a, sv = rng.uniform(-9, 9, B), rng.uniform(-3, 3, B)          # inside the control box
    Fx, Fa, Fsv = fu.step_jacobian(s, fu.DP)
    h = 1e-6
    worst = 0.0
    for j in (0, 1, 2, 3, 4, 5, 6, "a", "sv"):
        sp, sm, ap, am, vp, vm = s.copy(), s.copy(), a.copy(), a.copy(), sv.copy(), sv.copy()
        if j == "a":
            ap, am, col = a + h, a - h, Fa
        elif j == "sv":
            vp, vm, col = sv + h, sv - h, Fsv
        else:
            sp[:, j] += h
            sm[:, j] -= h
            col = Fx[:, :, j]
        fd = (fu.step(sp, ap, vp, fu.DP) - fu.step(sm, am, vm, fu.DP)) / (2 * h)
        err = np.abs(fd - col) / (1.0 + np.abs(col))
        worst = max(worst, float(err.max()))
    print(f"worst |fd - J| / (1 + |J|) = {worst:.2e}")
    # central differences at h = 1e-6: truncation h^2 f''' / 6 and rounding 2^-53 |s'| / h, both below 1e-8 for these states
    assert worst < 1e-7
    assert (Fx[:, 7, :7] == 0).all() and (Fx[:, 4:6, [0, 1, 2, 3, 6, 7]] == 0).all()      # vy, wz, curv never move


@pytest.mark.parametrize("T", [1, 5, 8])
def test_gradient_is_the_hand_adjoint_of_the_residuals(T):
    """g = J^T r from the forward sensitivities == the oracle's reverse-mode adjoint (hand_vjp.vjp_frenet) seeded with the weighted
    residuals"""
    B = 64
    rng = np.random.default_rng(7 + T)
    s0, goal, _ = fu.family("reach", B, T, seed=11 + T)
    s0 = s0.copy()
    s0[:, 2] = rng.uniform(-0.5, 0.5, B)                          # some rows outside the steering clip
    s0[:, 4:6] = rng.normal(size=(B, 2)) * 0.3
    u = np.hstack([rng.uniform(-9, 9, (B, T)), rng.uniform(-3, 3, (B, T))])
    Wd = dict(q=(0.5, 1, 0.5, 0.1), qf=(10, 10, 5, 1), r=(0.01, 0.1), rd=(0.01, 0.1))     # every residual weighted
    W = fu.weights_as(Wd, np.float64)
    c, g, H = fu.linearize(u, s0, goal, fu.DP, W)
    states, inside = fu.rollout(u, s0, fu.DP)
    assert inside.all()
    gs = np.zeros((B, T, 8))
    for t in range(T):
        e = fu.residual(states[t], goal)
        w = W["qf"] if t == T - 1 else W["q"]
        for k in range(4):
            gs[:, t, fu.COMP[k]] = w[k] * e[:, k]
    xu = np.hstack([s0, u])
    want = hand_vjp.vjp_frenet(xu, fu.DP, gs, 0.5)[:, 8:].copy()
    for o, k in ((0, 0), (T, 1)):
        want[:, o:o + T] += W["r"][k] * u[:, o:o + T]
        d = W["rd"][k] * np.diff(u[:, o:o + T], axis=1)
        want[:, o:o + T - 1] -= d
        want[:, o + 1:o + T] += d
    scale = np.abs(want).max(axis=1, keepdims=True)
    assert (np.abs(g - want) <= 1e-12 * scale).all(), float((np.abs(g - want) / scale).max())
    assert np.isfinite(H).all() and np.abs(H - np.swapaxes(H, 1, 2)).max() <= 1e-12 * np.abs(H).max()
    assert np.array_equal(c, fu.cost(u, s0, goal, fu.DP, W))


@pytest.fixture(scope="module")
def runs():
    """the statement on the families of test_gpu_nmpc_frenet.py: 257 rows, T = 5, seed 123 + T, both precisions, made once"""
    out = {}
    for name in ("reg", "stage", "reach", "sat"):
        s0, goal, W = fu.family(name, 257, 5, seed=128)
        for ft in (np.float64, np.float32):
            out[name, ft] = fu.solve(s0, goal, DP32, W, 5, ft=ft, history=True, **fu.DEFAULTS)
    return out


@pytest.mark.parametrize("name", ["reg", "stage", "reach", "sat"])
def test_statement_cost_never_rises_and_stays_in_the_box(runs, name):
    for ft in (np.float64, np.float32):
        r = runs[name, ft]
        assert (np.diff(r["costs"], axis=0) <= 0).all()
        assert (np.abs(r["u"][:, :5]) <= ft(DP32[10])).all() and (np.abs(r["u"][:, 5:]) <= ft(DP32[9])).all()
        assert np.array_equal(r["costs"][-1], r["cost"]) and np.array_equal(r["costs"][0], r["cost0"])
        assert (r["status"] != fu.NONFINITE).all()


def test_statement_converges_every_reg_stage_and_reach_row_at_T5(runs):
    """T = 5, 257 rows: every row converges in both precisions; reg takes 5.6 iterations a row, stage 5.3; reach comes down to
    rounding (final / initial cost <= 1e-28 in float64, <= 1e-10 in float32: the squared resolution of the states with room for
    the row count)"""
    for name, mean in (("reg", 5.6), ("stage", 5.3)):
        for ft in (np.float64, np.float32):
            r = runs[name, ft]
            print(f"{name} {ft.__name__}: status counts {np.bincount(r['status'], minlength=4)}, iterations mean {r['iters'].mean():.2f}")
            assert (r["status"] == fu.CONVERGED).all()
            assert abs(r["iters"].mean() - mean) < 0.1
    for ft, bar in ((np.float64, 1e-28), (np.float32, 1e-10)):
        r = runs["reach", ft]
        ratio = float((r["cost"] / r["cost0"]).max())
        print(f"reach {ft.__name__}: final / initial cost <= {ratio:.2e}")
        assert (r["status"] == fu.CONVERGED).all() and ratio <= bar


def test_statement_sat_rows_end_on_a_bound(runs):
    for ft in (np.float64, np.float32):
        r = runs["sat", ft]
        on = (np.abs(r["u"][:, :5]) == ft(DP32[10])).any(1) | (np.abs(r["u"][:, 5:]) == ft(DP32[9])).any(1)
        print(f"sat {ft.__name__}: rows with an active bound {on.sum()} / 257, status counts {np.bincount(r['status'], minlength=4)}")
        assert on.mean() > 0.9 and (r["cost"] <= r["cost0"]).all()
        assert np.isin(r["status"], (fu.CONVERGED, fu.MAX_ITER, fu.STALLED)).all()


def test_statement_at_T8_leaves_a_few_rows_at_max_iter():
    """T = 8 (seed 131): reg leaves 1 row of 257 at max_iter and reach 11, in float64 -- so 'every row converges' is asserted at
    T = 5 only.  Held here: reach leaves some rows and neither leaves more than a tenth (a row on the edge may fall either way
    with the host's sin and cos)."""
    for name, least in (("reg", 0), ("reach", 1)):
        s0, goal, W = fu.family(name, 257, 8, seed=131)
        r = fu.solve(s0, goal, DP32, W, 8, **fu.DEFAULTS)
        counts = np.bincount(r["status"], minlength=4)
        print(f"{name} T = 8: status counts {counts}")
        assert least <= counts[fu.MAX_ITER] <= 25 and counts[fu.CONVERGED] == 257 - counts[fu.MAX_ITER]


def test_a_start_outside_the_frame_is_nonfinite_and_stays_alone():
    """ey curv = 1.2: the start lies beyond the centre of curvature.  The row is NONFINITE with NaN costs and its clipped start;
    the rows next to it are what they are without it."""
    B, T = 8, 5
    s0, goal, W = fu.family("reg", B, T, seed=3)
    rng = np.random.default_rng(4)
    u0 = np.hstack([rng.uniform(-12, 12, (B, T)), rng.uniform(-4, 4, (B, T))])
    clean = fu.solve(s0, goal, DP32, W, T, u0=u0)
    bad = s0.copy()
    bad[3, 1], bad[3, 7] = 4.0, 0.3
    bad[6, 1], bad[6, 7] = -2.0, -0.5                               # ey curv = 1: on the centre itself
    r = fu.solve(bad, goal, DP32, W, T, u0=u0)
    assert list(np.where(r["status"] == fu.NONFINITE)[0]) == [3, 6]
    assert np.isnan(r["cost"][[3, 6]]).all() and np.isnan(r["cost0"][[3, 6]]).all() and (r["iters"][[3, 6]] == 0).all()
    hi = np.concatenate([np.full(T, DP32[10]), np.full(T, DP32[9])])
    assert np.array_equal(r["u"][[3, 6]], np.clip(u0[[3, 6]], -hi, hi))
    keep = np.setdiff1d(np.arange(B), [3, 6])
    for k in ("u", "cost0", "cost", "status", "iters", "grad"):
        assert np.array_equal(r[k][keep], clean[k][keep]), k


def test_a_trial_step_that_leaves_the_frame_is_rejected(monkeypatch):
    """rows next to the centre of curvature whose goal lies beyond it (edge_family): the cost of a trial step outside the frame
    is +inf, the step is rejected, the cost never rises and the result stays inside.  The trial costs are watched through
    fu.cost, which solve calls for nothing else."""
    B, T = 256, 5
    s0, goal, W = fu.edge_family(B)
    left = np.zeros(B, bool)
    plain = fu.cost

    def watched(*a):
        c = plain(*a)
        left[:] |= np.isinf(c)
        return c
    monkeypatch.setattr(fu, "cost", watched)
    r = fu.solve(s0, goal, DP32, W, T, history=True)
    ok = r["status"] != fu.NONFINITE
    print(f"edge: status counts {np.bincount(r['status'], minlength=4)}, rows with a trial step outside the frame {(left & ok).sum()}")
    assert (~ok).sum() >= 10 and (left & ok).sum() >= 10                        # both kinds are there
    assert np.array_equal(~ok, ~fu.rollout(np.zeros((B, 2 * T)), s0, DP32)[1])  # NONFINITE: the rows that leave at rest
    assert np.isfinite(r["cost"][ok]).all() and (np.diff(r["costs"][:, ok], axis=0) <= 0).all()
    assert fu.rollout(r["u"], s0, DP32)[1][ok].all()


# ------------------------------------------------------------------ the Python layer, no GPU
def test_frenet_query_problem_takes_the_query_literally():
    x = np.arange(16, dtype=np.float32).reshape(2, 8) + 1          # [ey, delta, vx, vy, vx_goal, wz, epsi, curv]
    x[1, 0] = -x[1, 0]                                             # right of the line: not mirrored
    s0, goal = nmpc.frenet_query_problem(x)
    assert np.array_equal(s0, [[0, 1, 2, 3, 4, 6, 7, 8], [0, -9, 10, 11, 12, 14, 15, 16]])
    assert np.array_equal(goal, [[0, 0, 0, 5], [0, 0, 0, 13]]) and s0.dtype == np.float32 and goal.dtype == np.float32
    with pytest.raises(ValueError, match="queries"):
        nmpc.frenet_query_problem(np.zeros((3, 7)))
    with pytest.raises(ValueError, match="queries"):
        nmpc.solve_queries_frenet(np.zeros((3, 7)), fu.DP)
    with pytest.raises(ValueError, match="queries"):
        nmpc.make_table_frenet(np.zeros(8), fu.DP)


def test_frenet_weights_leave_progress_free():
    w = nmpc.FrenetWeights()
    assert tuple(w.q) == (0.0, 1.0, 0.5, 0.1) and tuple(w.qf) == (0.0, 10.0, 5.0, 1.0)
    assert tuple(w.r) == tuple(nmpc.Weights().r) and tuple(w.rd) == tuple(nmpc.Weights().rd)
    assert isinstance(w, nmpc.Weights)


def test_python_side_validation_errors():
    s0, goal, dp = np.zeros((3, 8), np.float32), np.zeros((3, 4), np.float32), fu.DP
    bad = [
        (dict(state0=np.zeros((3, 7))), "state0"),
        (dict(state0=np.zeros(8)), "state0"),
        (dict(goal=np.zeros((3, 3))), "goal"),
        (dict(goal=np.zeros((2, 4))), "goal"),
        (dict(u0=np.zeros((3, 8))), "u0"),
        (dict(dyn_params=None), "dyn_params"),
        (dict(dyn_params=np.zeros(12)), "dyn_params"),
        (dict(dyn_params=np.zeros((2, 13))), "dyn_params"),
        (dict(T=0), "horizon"),
        (dict(T=9), "horizon"),
        (dict(T=2.5), "horizon"),
        (dict(max_iter=-1), "max_iter"),
        (dict(lambda0=-1.0), "lambda0"),
        (dict(lambda_min=1.0, lambda_max=0.5), "lambda_min"),
        (dict(tol=float("inf")), "tol"),
        (dict(eps=-1e-6), "eps"),
        (dict(weights=nmpc.FrenetWeights(q=(1, 1, 1))), "weights.q"),
        (dict(weights=nmpc.FrenetWeights(qf=(1, 1, -1, 1))), "weights.qf"),
        (dict(weights=nmpc.FrenetWeights(rd=(0, float("inf")))), "weights.rd"),
    ]
    for kw, word in bad:
        args = dict(state0=s0, goal=goal, dyn_params=dp)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            nmpc.solve_frenet(**args)
    with pytest.raises(TypeError, match="Weights"):
        nmpc.solve_frenet(s0, goal, dp, weights=dict(q=(1, 1, 1, 1)))
    with pytest.raises(TypeError):
        nmpc.solve_frenet(s0, goal, dp, mode=_lib.ROLLOUT_ST_KS)   # there is no mode to choose
    with pytest.raises(TypeError, match="Track"):
        nmpc.closed_loop_frenet(object(), np.zeros((3, 7)), 3, dp)
    from irbfn_amd.simulate import Track
    import _simulate_util as su
    tr = Track(su.straight_track(10), wrap=False)
    c0 = np.zeros((3, 7), np.float32)
    for kw, word in ((dict(ticks=-1), "ticks"), (dict(n_sub=0), "ticks"), (dict(T=9), "horizon"), (dict(max_iter=-2), "max_iter"),
                     (dict(plant_params=np.zeros((2, 13))), "plant_params"), (dict(mode=_lib.ROLLOUT_FRENET_LS), "plant"),
                     (dict(dyn_params=np.zeros(12)), "dyn_params")):
        args = dict(track=tr, state0=c0, ticks=3, dyn_params=dp)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            nmpc.closed_loop_frenet(**args)
    with pytest.raises(ValueError, match="state0"):
        nmpc.closed_loop_frenet(tr, np.zeros((3, 8)), 3, dp)       # the cars are single-track states
    for kw in (dict(u0=np.zeros((3, 10))), dict(want_grad=True), dict(nonsense=1)):
        with pytest.raises(TypeError, match="closed_loop_frenet"):
            nmpc.closed_loop_frenet(tr, c0, 3, dp, **kw)


def test_the_cartesian_entry_points_still_refuse_the_frenet_model():
    with pytest.raises(ValueError, match="model"):
        nmpc.solve(np.zeros((3, 7), np.float32), np.zeros((3, 4), np.float32), fu.DP, mode=_lib.ROLLOUT_FRENET_LS)
    with pytest.raises(ValueError, match="state0"):
        nmpc.solve(np.zeros((3, 8), np.float32), np.zeros((3, 4), np.float32), fu.DP)


def test_header_declares_the_entry_point_and_lib_binds_it():
    text = open(os.path.join(ROOT, "include", "irbfn_hip.h")).read()
    assert "int irbfn_nmpc_solve_frenet(int T, const float* state0_dev /*[B,8]*/" in text
    assert "#define IRBFN_ABI_VERSION 1" in text
    lib = _lib.load()
    fn = lib.irbfn_nmpc_solve_frenet
    assert fn.restype is C.c_int and len(fn.argtypes) == 13
    assert lib.irbfn_abi_version() == 1


def test_c_entry_point_decides_bad_arguments_before_any_launch():
    lib = _lib.load()
    mk = lambda: nmpc._options(nmpc.FrenetWeights(), 30, 1e-3, 1e-9, 1e6, 1e-6, 1e-6)
    opt = mk()
    one = C.c_void_p(64)                                          # never dereferenced: every call below returns before a launch
    dp = (C.c_float * 13)(*fu.DP)
    call = lambda T=5, s=one, g=one, dh=dp, dd=None, o=C.byref(opt), u=one, c=one, i=one, B=4: \
        lib.irbfn_nmpc_solve_frenet(T, s, g, None, dh, dd, o, u, c, i, None, B, None)
    assert call(B=0) == 0
    assert call(B=0, s=None, g=None, u=None, c=None, i=None, dh=None) == 0
    assert call(B=-1) == -1
    assert call(o=None) == -1
    for T in (0, 9, -3):
        assert call(T=T) == -2
    for name in ("s", "g", "u", "c", "i"):
        assert call(**{name: None}) == -1
    assert call(dh=None) == -1
    for field, v in (("lambda0", -1.0), ("lambda_min", float("nan")), ("lambda_max", float("inf")), ("tol", -1e-3), ("eps", -1.0)):
        o2 = mk()
        setattr(o2, field, v)
        assert call(o=C.byref(o2)) == -1, field
    for field, n in (("q", 4), ("qf", 4), ("r", 2), ("rd", 2)):
        for v in (-1.0, float("nan"), float("inf")):
            o2 = mk()
            getattr(o2, field)[n - 1] = v
            assert call(o=C.byref(o2)) == -1, (field, v)
    o2 = mk()
    o2.lambda_min, o2.lambda_max = 2.0, 1.0
    assert call(o=C.byref(o2)) == -1
    o2 = mk()
    o2.max_iter = -1
    assert call(o=C.byref(o2)) == -1
    # negative weights are bad arguments whatever T is: the weights are looked at first, as in irbfn_nmpc_solve
    o2 = mk()
    o2.q[0] = -1.0
    assert call(o=C.byref(o2), T=9) == -1
