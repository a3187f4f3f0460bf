"""The oracle's line-by-line restatements of the planner front end (oracle/irbfn_oracle.py: plan_query_cartesian,
lut_grid_lookup, lut_nearest, nearest_point, intersect_point) against the high-precision statements of the operations in
tests/_planner_front_util.py.  The kernels are compared with the restatements (tests/test_gpu_planner_front.py); a mistake the
restatement shared with a kernel would show here.  No GPU."""
import numpy as np
import pytest

import _planner_front_util as pf
from oracle import irbfn_oracle as orc


# ------------------------------------------------------------------ Cartesian queries
def test_cartesian_restatement_matches_the_mpmath_rotation():
    import mpmath as mp
    pose, goal, special = pf.cartesian_case(257)
    gl0, gl1, gt, mag = pf.rotate_mp(pose, goal)
    with np.errstate(invalid="ignore"):
        ref = [orc.plan_query_cartesian(pose[b], goal[b], unfused=True) for b in range(257)]
    rx, rm = np.stack([r[0] for r in ref]).astype(np.float64), np.array([r[1] for r in ref])
    fin = np.isfinite(gl0)
    assert set(np.flatnonzero(~fin)) == {special["nan_pose"], special["inf_pose"]}
    band = 8 * pf.U64 * mag
    clear = fin & (np.abs(gl1) > band)
    assert clear.sum() >= 0.99 * (fin.sum() - len(special))
    np.testing.assert_array_equal(rm[clear], gl1[clear] < 0)
    assert not rm[~fin].any() and np.isnan(rx[~fin][:, 1:4]).all()
    assert (np.abs(rx[fin, 1] - gl0[fin]) <= pf.ulp32(gl0[fin]) / 2 + band[fin]).all()
    assert (np.abs(rx[fin, 2] - np.abs(gl1[fin])) <= pf.ulp32(gl1[fin]) / 2 + band[fin]).all()
    # column 3: (+-gt) mod pi with pi the double, exactly, then float32; the restatement rounds r + pi once more in float64
    with mp.workprec(200):
        p = mp.mpf(float(np.pi))
        for b in np.flatnonzero(fin):
            g = mp.mpf(float(-gt[b] if rm[b] else gt[b]))
            r = float(g - mp.floor(g / p) * p)
            assert abs(rx[b, 3] - r) <= pf.ulp32(r) / 2 + 2 * pf.U64 * np.pi, (b, rx[b, 3], r)
    assert (rx[fin, 3] >= 0).all() and (rx[fin, 3] <= np.float32(np.pi)).all()
    # the rows built on purpose: a zero remainder is +0.0 whatever the sign of gt; gl1 = -0.0 does not mirror
    for name in ("gt_0pi_on", "gt_1pi_on", "gt_-1pi_on", "gt_3pi_on", "gt_neg_zero", "gt_pos_zero", "gt_neg_zero_mirrored",
                 "gt_pos_zero_mirrored"):
        assert pf.bits32(ref[special[name]][0][3]) == 0, name
    row = special["gl1_neg_zero"]
    assert not rm[row] and pf.bits32(ref[row][0][2]) == 0x80000000
    assert rm[special["gt_neg_zero_mirrored"]] and not rm[special["gt_neg_zero"]]


def test_straight_ahead_goal_never_mirrors_in_numpy():
    """s * dx + c * dy with every product rounded is exactly 0 when the goal lies on the heading: the two products are the
    same two factors in the other order.  A fused multiply-add keeps the rounding error of one product and mirrors about half."""
    pose, goal = pf.straight_ahead()
    ref = [orc.plan_query_cartesian(pose[b], goal[b], unfused=True) for b in range(pose.shape[0])]
    assert not any(r[1] for r in ref)
    assert all(r[0][2] == 0 for r in ref)
    lit = [orc.plan_query_cartesian(pose[b], goal[b]) for b in range(pose.shape[0])]      # np.dot: fused or not, the BLAS's choice
    assert all(abs(float(r[0][2])) <= 16 * pf.U64 * 4 for r in lit)


# ------------------------------------------------------------------ table look-ups
@pytest.mark.parametrize("lens", [(1,), (2, 1, 3, 17), (17, 3, 2, 1, 1, 2, 3)])
def test_grid_lookup_restatement_matches_a_linear_scan(lens):
    axes = pf.grid_axes(lens, seed=len(lens))
    q = pf.grid_queries(axes, 300, seed=1)
    for shape in ([len(a) for a in axes], [max(1, len(a) - 1) for a in axes]):
        for b in range(q.shape[0]):
            assert orc.lut_grid_lookup(axes, shape, q[b])[1] == pf.grid_lookup_scan(axes, shape, q[b])


def test_lut_nearest_restatement_matches_brute_force():
    rng = np.random.default_rng(5)
    for D in (3, 8):
        inputs = rng.uniform(-3, 3, size=(4000, D)).astype(np.float32).astype(np.float64)
        q = rng.uniform(-3.2, 3.2, size=(50, D)).astype(np.float32).astype(np.float64)
        q[0] = inputs[1234]
        rd, ri = orc.lut_nearest(inputs, q)
        d2 = pf.nearest_bruteforce(inputs, q)
        np.testing.assert_array_equal(ri, d2.argmin(axis=1))
        np.testing.assert_allclose(rd, np.sqrt(d2.min(axis=1)), rtol=1e-14, atol=0)
    with pytest.raises(ValueError):                    # scipy gives no answer to copy for a NaN query
        orc.lut_nearest(inputs, np.full((1, 8), np.nan))


# ------------------------------------------------------------------ nearest point on a polyline
def _nearest_rows(traj, pts):
    return [orc.nearest_point(pts[b], traj, skip_nan=True) for b in range(pts.shape[0])]


@pytest.mark.parametrize("kind,N", [("race", 200), ("open", 129), ("open", 3), ("open", 2), ("closed", 66)])
def test_nearest_point_restatement_finds_the_true_nearest_segment(kind, N):
    rng = np.random.default_rng(N)
    traj = pf.race_line(N) if kind == "race" else pf.staircase(N, kind)
    pts = traj[rng.integers(0, N, 300)] + rng.normal(size=(300, 2)) * 0.8
    d, t = pf.polyline_distances(pts, traj)
    d32, t32 = pf.polyline_distances32(pts, traj)
    seglen = np.hypot(*(traj[1:] - traj[:-1]).T)
    # what a float32 evaluation of the operation does, at worst over the case, to a distance and to the place of a projection
    tol = np.full(300, 4 * np.abs(d32.astype(pf.LD) - d).max())
    tol_p = np.full(300, 4 * (np.abs(t32.astype(pf.LD) - t) * seglen).max())
    ref = _nearest_rows(traj, pts)
    differs = 0
    for b, (rp, rd, rt, rk) in enumerate(ref):
        k = int(d[b].argmin())
        assert d[b, rk] - d[b, k] <= tol[b], (b, rk, k)
        differs += rk != k
        assert abs(rd - d[b, rk]) <= tol[b] and abs(rt - t[b, rk]) * seglen[rk] <= tol_p[b]
        S, V = traj[rk], traj[rk + 1] - traj[rk]
        assert np.abs(rp - (S + float(t[b, rk]) * V)).max() <= tol_p[b]
    assert differs <= 0.05 * len(ref)
    assert float(tol.max()) < 1e-4                                   # rounding, not a wrong segment


def test_nearest_point_ties_go_to_the_first_segment():
    for N, variant, ks in ((66, "open", (1, 63)), (200, "open", (1, 63, 127)), (66, "closed", (1,))):
        traj = pf.staircase(N, variant)
        for k in ks + ((64,) if N > 65 and variant == "open" else ()):
            for p in (pf.corner_tie_point(traj, k), traj[k]):
                d, _ = pf.polyline_distances(p[None], traj)
                assert d[0, k - 1] == d[0, k] == d[0].min()
                assert orc.nearest_point(p, traj)[3] == k - 1
    traj = pf.staircase(200, "replay")
    rng = np.random.default_rng(0)
    pts = traj[rng.integers(0, 64, 50)] + rng.normal(size=(50, 2)) * 0.5
    d, _ = pf.polyline_distances(pts, traj)
    for b in range(50):
        k = orc.nearest_point(pts[b], traj)[3]
        assert k < 64 and d[b, k] == d[b, k + 64]
    traj = pf.staircase(66, "closed")
    for p in (traj[0], traj[0] + [-0.25, 0.25]):
        d, _ = pf.polyline_distances(p[None], traj)
        assert d[0, 0] == d[0, 64] == d[0].min()
        assert orc.nearest_point(p, traj)[3] == 0


def test_argmin_returns_the_nan_segment_and_skip_nan_does_not():
    traj = pf.staircase(10)
    traj[4] = traj[3]                                   # segment 3 has no length: t = 0 / 0
    p = traj[7] + [0.25, 0.25]
    with np.errstate(invalid="ignore", divide="ignore"):
        lit = orc.nearest_point(p, traj)
        skip = orc.nearest_point(p, traj, skip_nan=True)
        assert lit[3] == 3 and np.isnan(lit[1])
        d, _ = pf.polyline_distances(p[None], traj)
        assert skip[3] == int(d[0].argmin()) == 6 and skip[1] == float(d[0].min())
        nan = orc.nearest_point(p, np.full((5, 2), np.nan), skip_nan=True)
    assert np.array_equal(nan[0], [0.0, 0.0]) and nan[1] == np.inf and nan[2] == 0.0 and nan[3] == 0


# ------------------------------------------------------------------ circle / polyline intersection
@pytest.mark.parametrize("closed,N,B", [(True, 200, 500), (False, 200, 500), (True, 65, 120), (False, 3, 60), (False, 2, 60)])
def test_intersect_point_restatement_against_the_exact_solver(closed, N, B):
    traj, pts, ts, radius, ref = pf.intersect_reference(closed, N, B)
    flagged = 0
    for wrap in (True, False):
        for b in range(B):
            rp, ri, rt = ref[wrap][b]
            i, t, flag, dt = pf.first_hit_exact(pts[b], radius, traj, float(ts[b]), wrap)
            flagged += flag
            if flag:
                continue
            assert (ri is None) == (i is None), (b, ri, i)
            if i is None:
                continue
            assert ri == i, (b, ri, i)                              # no earlier segment has a root the exact solver accepts
            S, V = pf.segment_ends(traj, np.array([i]))
            L = float(np.hypot(*V[0].astype(np.float64)))
            tol = L * (dt + 4 * pf.U32) + 2 * float(pf.ulp32(np.abs(rp).max()))
            assert abs(float(rt) - float(t)) * L <= tol
            on_circle = abs(np.hypot(*(rp.astype(np.float64) - pts[b])) - float(np.float32(radius)))
            d_seg, _ = pf.polyline_distances(rp.astype(np.float64)[None], np.stack([S[0], S[0] + V[0]]).astype(np.float64))
            assert on_circle <= tol and float(d_seg[0, 0]) <= tol, (b, on_circle, float(d_seg[0, 0]), tol)
    assert flagged <= 0.05 * 2 * B, flagged


@pytest.mark.parametrize("closed", [True, False])
def test_intersect_case_holds_every_category(closed):
    n = pf.case_categories(*pf.intersect_reference(closed, 200, 500))
    for name, c in n.items():
        if name == "wrap_closing" and not closed:
            continue
        assert c >= 40, n
