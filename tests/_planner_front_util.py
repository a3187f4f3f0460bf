"""High-precision statements of the OPERATIONS behind the planner front end (irbfn_amd/csrc/planner_front.hip), and the
inputs its tests share.  test_planner_front_reference_cpu.py holds the oracle's line-by-line restatements
(oracle/irbfn_oracle.py: plan_query_*, lut_*, nearest_point, intersect_point) to these statements; test_gpu_planner_front.py
holds the kernels to the restatements.  A plain module (no fixtures, no hooks).

  rotate_mp            : rotation of (goal - pose) into the vehicle frame and the heading difference, mpmath at 200 bits.
  polyline_distances   : true distance of points to every segment of a polyline, np.longdouble (64-bit mantissa).
  polyline_distances32 : the same operation evaluated in float32 -- the "float32 twin" whose error says how close two true
                         distances must be before a float32 projection may order them differently.
  circle_roots         : roots of |S + t V - P| = r for every segment, np.longdouble, on the segment end points the
                         reference defines (float32 way-points, end point + 1e-6f).
  first_hit_exact      : first accepted root in the reference's search order, with a per-row flag "near tangent or near an
                         end point": the accept / reject pattern changes when a and c move by the float32 rounding of the
                         reference's own a (3 ulp) and of the |S|^2 term of c (3 ulp).
"""
import functools

import numpy as np

from oracle import irbfn_oracle as orc

LD = np.longdouble
U32 = 2.0 ** -24           # unit round-off of float32
U64 = 2.0 ** -53


# ------------------------------------------------------------------ rotation and mirror
def rotate_mp(pose, goal):
    """pose [B,7], goal [B,4] (float64) -> (gl0, gl1, gt, mag): goal offset in the vehicle frame, rounded once from 200-bit
    values to float64; gt = goal heading - theta rounded once; mag = |dx| + |dy| of the exact offset."""
    import mpmath as mp
    B = pose.shape[0]
    out = np.full((B, 4), np.nan)
    with mp.workprec(200):
        for b in range(B):
            vals = [pose[b, 0], pose[b, 1], pose[b, 4], goal[b, 0], goal[b, 1], goal[b, 2]]
            if not np.isfinite(vals).all():
                continue
            x, y, th, gx, gy, gth = (mp.mpf(float(v)) for v in vals)
            dx, dy = gx - x, gy - y
            c, s = mp.cos(-th), mp.sin(-th)
            out[b] = [float(c * dx - s * dy), float(s * dx + c * dy), float(gth - th), float(abs(dx) + abs(dy))]
    return out[:, 0], out[:, 1], out[:, 2], out[:, 3]


def ulp32(v):
    """spacing of float32 at |v| (float64 array)"""
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def poses(rng, B, pos=50.0, heading=3.2):
    """random (pose [B,7], goal [B,4]): goals 0.3 .. 3.5 m away, within +-1.2 rad of the heading"""
    pose = np.stack([rng.uniform(-pos, pos, B), rng.uniform(-pos, pos, B), rng.uniform(-0.4, 0.4, B), rng.uniform(0, 7, B),
                     rng.uniform(-heading, heading, B), rng.uniform(-2, 2, B), rng.uniform(-0.3, 0.3, B)], axis=1)
    d = rng.uniform(0.3, 3.5, B)
    ang = pose[:, 4] + rng.uniform(-1.2, 1.2, B)
    goal = np.stack([pose[:, 0] + d * np.cos(ang), pose[:, 1] + d * np.sin(ang), pose[:, 4] + rng.uniform(-4, 4, B),
                     rng.uniform(0.5, 7, B)], axis=1)
    return pose, goal


def cartesian_case(B):
    """Inputs of the Cartesian query tests: thirds of the rows with headings in +-3.2 / +-1000 rad and positions up to 50 m /
    1e6 m; then, as far as B allows, rows 0..: gt = k pi (as a double) and its two neighbours, gt = -0.0 and +0.0,
    gl1 = -0.0 (heading 0, goal straight ahead at dy = -0.0), and near the end one pose row with NaN position and heading and
    one with an Inf heading (columns 1-3 are NaN there).
    -> (pose, goal, special) with special = {name: row}."""
    rng = np.random.default_rng(1000 + B)
    pose, goal = poses(rng, B)
    n = B // 3
    if n:
        p2, g2 = poses(rng, n, pos=50.0, heading=1000.0)
        p3, g3 = poses(rng, n, pos=1e6, heading=3.2)
        pose[:n], goal[:n] = p2, g2
        pose[n:2 * n], goal[n:2 * n] = p3, g3
    special = {}
    r = 0

    def take(name):
        nonlocal r
        if r >= B:
            return None
        special[name] = r
        r += 1
        return r - 1
    for k in (0, 1, -1, 3):
        for step, tag in ((0, "on"), (1, "above"), (-1, "below")):
            row = take(f"gt_{k}pi_{tag}")
            if row is None:
                continue
            v = k * np.pi
            if step:
                v = np.nextafter(v, np.inf * step)
            pose[row, 4] = 0.0                    # gt = goal heading - 0 exactly
            goal[row, 2] = v
            goal[row, :2] = pose[row, :2] + [1.0, 0.5 if (k + step) % 2 else -0.5]   # mirrored and unmirrored rows
    for name, gth, th in (("gt_neg_zero", -0.0, 0.0), ("gt_pos_zero", 0.0, 0.0), ("gt_neg_zero_mirrored", -0.0, 0.0),
                          ("gt_pos_zero_mirrored", 0.0, 0.0)):
        row = take(name)
        if row is not None:
            pose[row, 4], goal[row, 2] = th, gth
            goal[row, :2] = pose[row, :2] + [1.0, -0.5 if name.endswith("mirrored") else 0.5]
    row = take("gl1_neg_zero")
    if row is not None:                           # heading 0: s = -0.0, c = 1, dx = 2, dy = -0.0 -> gl1 = -0.0: no mirror
        pose[row, :2], pose[row, 4] = [3.0, 0.0], 0.0
        goal[row, :2] = [5.0, -0.0]
    if B >= 8:
        special["nan_pose"], special["inf_pose"] = B - 3, B - 5
        pose[B - 3, [0, 4]] = np.nan
        pose[B - 5, 4] = np.inf
    return pose, goal, special


def straight_ahead(n=2000):
    """a pose at the origin with n headings in +-3.2 rad, the goal two metres straight ahead: gl1 is exactly 0 wherever
    sin(-theta) = -sin(theta) and both products are rounded"""
    th = np.linspace(-3.2, 3.2, n)
    pose = np.zeros((n, 7))
    pose[:, 4] = th
    goal = np.stack([2 * np.cos(th), 2 * np.sin(th), th, np.ones(n)], axis=1)
    return pose, goal


# ------------------------------------------------------------------ nearest point on a polyline
def polyline_distances(points, traj, ft=LD):
    """points [B,2], traj [N,2] -> (dist [B,N-1], t [B,N-1]) of the operation itself in dtype ft: orthogonal projection onto
    each segment's line, clamped to the segment; a zero-length segment is its point."""
    P, W = np.asarray(points, ft), np.asarray(traj, ft)
    S, V = W[:-1], W[1:] - W[:-1]
    l2 = (V * V).sum(axis=1)
    L = P[:, None, :] - S[None, :, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.where(l2 > 0, (L * V[None]).sum(axis=2) / l2, ft(0))
    t = np.clip(t, ft(0), ft(1))
    E = L - t[..., None] * V[None]
    return np.sqrt((E * E).sum(axis=2)), t


def polyline_distances32(points, traj):
    """the float32 twin: way-points, point and every operation in float32"""
    return polyline_distances(np.asarray(points, np.float32), np.asarray(traj, np.float32), np.float32)


def staircase(N, variant="open"):
    """Way-points on the quarter-integer lattice: step i is (+a_i, 0) for even i and (0, -a_i) for odd i, a_i = 1 + (i % 3) / 4.
    'open'    : as is.
    'replay'  : way-point 64 + i repeats way-point i (and 128 + i): segments i, i + 64, i + 128 coincide, every point ties
                between two rounds of one lane.
    'closed'  : the last way-point is the first again: segments 0 and N - 2 share it."""
    step = np.zeros((max(N - 1, 1), 2))
    a = 1.0 + (np.arange(N - 1) % 3) / 4.0
    step[0::2, 0] = a[0::2]
    step[1::2, 1] = -a[1::2]
    traj = np.vstack([np.zeros((1, 2)), np.cumsum(step, axis=0)])[:N] + [2.0, -1.0]
    if variant == "replay":
        traj = traj[np.arange(N) % 64]
    elif variant == "closed":
        traj[N - 1] = traj[0]
    return traj


def corner_tie_point(traj, k):
    """a point a quarter off the convex side of the staircase corner at way-point k (0 < k < N - 1): segments k - 1 and k both
    project onto the way-point itself, at the same distance sqrt(1 / 8) exactly"""
    return traj[k] + ([0.25, 0.25] if k % 2 else [-0.25, -0.25])


# ------------------------------------------------------------------ circle / polyline intersection
def segment_ends(traj, idx):
    """(S, V) float32 of segments idx (any integer, taken modulo N) as the reference defines them: float32 way-points, the end
    point moved by +1e-6f (planner_utils.py:160-163)"""
    t32 = np.asarray(traj, np.float64).astype(np.float32)
    n = t32.shape[0]
    idx = np.asarray(idx)
    S = t32[idx % n]
    E = t32[(idx + 1) % n] + np.float32(1e-6)
    return S, E - S


def circle_roots(point, radius, S, V, da=0.0, dc=0.0):
    """-> (t1, t2, a) longdouble per segment (NaN where the line misses the circle); da relative, dc absolute perturbations"""
    S, V, P = np.asarray(S, LD), np.asarray(V, LD), np.asarray(point, LD)
    r = LD(np.float32(radius))
    a = (V * V).sum(axis=1) * (1 + LD(da))
    d = S - P
    b = 2 * (V * d).sum(axis=1)
    c = (d * d).sum(axis=1) - r * r + LD(dc)
    disc = b * b - 4 * a * c
    with np.errstate(invalid="ignore", divide="ignore"):
        sq = np.sqrt(np.where(disc >= 0, disc, np.nan))
        return (-b - sq) / (2 * a), (-b + sq) / (2 * a), a


def search_order(N, ts, wrap):
    """segment indices in the reference's search order from t_start = ts (planner_utils.py:155, :176, :205-206)"""
    start_i = int(ts)
    order = list(range(start_i, N - 1))
    if wrap:
        order += list(range(-1, start_i))
    return np.array(order, dtype=np.int64), start_i


def _accept(t1, t2, first_mask, start_t):
    lo = np.where(first_mask, LD(start_t), LD(0))
    with np.errstate(invalid="ignore"):
        ok1 = (t1 >= 0) & (t1 <= 1) & (t1 >= lo)
        ok2 = (t2 >= 0) & (t2 <= 1) & (t2 >= lo)
    return ok1, ok2


def first_hit_exact(point, radius, traj, ts=0.0, wrap=False):
    """-> (i, t, flagged, dt): the first segment in search order with an accepted root, that root (longdouble), whether the
    row is near a tangent or an end point (see the module docstring), and the largest move of the returned root under those
    perturbations (0 if there is no hit).  i = None where nothing is hit."""
    N = np.asarray(traj).shape[0]
    order, start_i = search_order(N, ts, wrap)
    if order.size == 0:
        return None, None, False, 0.0
    start_t = np.float32(ts % 1.0)
    S, V = segment_ends(traj, order)
    first = np.zeros(order.size, bool)
    first[0] = order[0] == start_i and start_i < N - 1
    s2 = (S.astype(LD) ** 2).sum(axis=1)
    da, dc = 3 * U32, 3 * U32 * s2

    def solve(ea, ec):
        t1, t2, _ = circle_roots(point, radius, S, V, ea * da, ec * dc)
        ok1, ok2 = _accept(t1, t2, first, start_t)
        return np.where(ok1, t1, np.where(ok2, t2, np.nan)), ok1, ok2

    t0, ok1, ok2 = solve(0, 0)
    hit = np.flatnonzero(ok1 | ok2)
    k = int(hit[0]) if hit.size else order.size - 1
    flagged, dt = False, 0.0
    for ea in (-1, 1):
        for ec in (-1, 1):
            tp, p1, p2 = solve(ea, ec)
            if not (np.array_equal(p1[:k + 1], ok1[:k + 1]) and np.array_equal(p2[:k + 1], ok2[:k + 1])):
                flagged = True
            elif hit.size:
                dt = max(dt, float(abs(tp[k] - t0[k])))
    if not hit.size:
        return None, None, flagged, 0.0
    return int(order[k]), t0[k], flagged, dt


def race_line(N):
    """a closed line (the closing segment N-1 -> 0 is an ordinary one), way-points about 0.35 .. 0.75 m apart at N = 200"""
    th = np.linspace(0, 2 * np.pi, N, endpoint=False)
    return np.stack([20 * np.cos(th) + 3 * np.cos(3 * th), 12 * np.sin(th)], axis=1)


def open_line(N):
    """an open line: one arch of a sine, way-points about 0.5 m apart, above its closing chord"""
    s = np.arange(N) * 0.5
    return np.stack([s, 8.0 * np.sin(np.pi * s / max(s[-1], 1.0))], axis=1)


def case_radius(traj):
    """0.4 of the shortest segment: a circle about a point on a segment reaches that segment and at most its neighbours"""
    return float(0.4 * np.hypot(*(traj[1:] - traj[:-1]).T).min())


def on_segment(traj, j, u, off=0.0):
    """the point at parameter u of segment j (modulo N), moved `off` along the segment's left normal"""
    n = traj.shape[0]
    s, e = traj[j % n], traj[(j + 1) % n]
    v = e - s
    return s + u * v + off * np.array([-v[1], v[0]]) / np.hypot(*v)


CATEGORIES = ("first_t2", "first_skipped", "round2", "round3", "wrap_closing", "wrap_before_start", "start_at_end")


def intersect_case(traj, closed, B, per=44, seed=0):
    """-> (points [B,2], t_start [B], radius, category [B] of names or '').  Every category of CATEGORIES gets `per` rows where
    the line allows it (N >= 200 for the rounds; a closed line for wrap_closing); the rest are random points near the line.
      first_t2          : start on the hit segment between its two roots: the second root is returned
      first_skipped     : start on the segment behind both roots; the circle reaches no later segment, but (wrap) the
                          segment before the start: wrap_before_start, and without wrap nothing
      round2 / round3   : the start lies 64 .. 127 / 128 .. 191 segments before the only segments the circle reaches
      wrap_closing      : the circle reaches the closing segment only, the start is elsewhere
      start_at_end      : start_i = N - 1, N and N + 5: nothing forward, everything in the wrap loop"""
    rng = np.random.default_rng(seed + 7 * traj.shape[0])
    N = traj.shape[0]
    nseg = N if closed else N - 1
    radius = case_radius(traj)
    pts = np.empty((B, 2))
    ts = np.empty(B)
    cat = np.array([""] * B, dtype=object)
    j = rng.integers(0, N - 1, B)
    for b in range(B):                                   # random: near the line, start a little before
        pts[b] = on_segment(traj, int(j[b]), rng.uniform(0, 1), rng.normal() * 0.5 * radius)
        ts[b] = max(0.0, j[b] - rng.integers(0, 6) + rng.uniform(0, 1))
    if B < 8:
        return pts, ts, radius, cat
    r = 0

    def rows(name, ok=True):
        nonlocal r
        if not ok:
            return range(0)
        n = min(per, B - r)
        out = range(r, r + n)
        cat[r:r + n] = name
        r += n
        return out
    for b in rows("first_t2"):
        jj = int(rng.integers(0, N - 1))
        pts[b], ts[b] = on_segment(traj, jj, 0.5, 0.02), jj + 0.5
    for name in ("first_skipped", "wrap_before_start"):
        for b in rows(name, N >= 3):
            jj = int(rng.integers(1, N - 1))
            pts[b], ts[b] = on_segment(traj, jj, 0.15, 0.02), jj + 0.9
    for name, lo in (("round2", 64), ("round3", 128)):
        for b in rows(name, N >= 200):
            back = int(rng.integers(lo + 2, lo + 60))
            jj = int(rng.integers(back, N - 1))
            pts[b], ts[b] = on_segment(traj, jj, 0.5, 0.02), jj - back + rng.uniform(0, 1)
    for b in rows("wrap_closing", closed and N >= 8):
        pts[b], ts[b] = on_segment(traj, -1, 0.5, 0.02), N // 2 + rng.uniform(0, 1)
    for b in rows("start_at_end"):
        jj = int(rng.integers(0, nseg))
        pts[b], ts[b] = on_segment(traj, jj, 0.5, 0.02), (N - 1, N, N + 5)[b % 3] + rng.uniform(0, 1)
    return pts, ts, radius, cat


def count_categories(N, ts, ref_wrap, ref_nowrap, roots_first):
    """How many rows of a case fall into each category, judged on the reference's own answers.  ref_wrap / ref_nowrap: per row
    the (point, index, t) of the restatement with and without wrap; roots_first: per row the exact (t1, t2) of segment
    start_i (NaN where there is none)."""
    n = dict.fromkeys(CATEGORIES + ("wrap_off_none",), 0)
    for b in range(len(ts)):
        start_i, start_t = int(ts[b]), np.float32(ts[b] % 1.0)
        (_, iw, tw), (_, io, _) = ref_wrap[b], ref_nowrap[b]
        t1, t2 = roots_first[b]
        if iw is None:
            continue
        n["wrap_off_none"] += io is None
        n["start_at_end"] += start_i >= N - 1
        if start_i >= N - 1:
            continue
        n["first_t2"] += iw == start_i and t1 < start_t <= tw
        n["first_skipped"] += iw != start_i and 0 <= t2 <= 1 and t2 < start_t
        n["round2"] += 64 <= iw - start_i < 128
        n["round3"] += 128 <= iw - start_i < 192
        n["wrap_closing"] += iw == -1
        n["wrap_before_start"] += iw == start_i - 1 and iw >= 0
    return n


@functools.lru_cache(maxsize=None)
def intersect_reference(closed, N, B):
    """The shared intersect_point case of a line: -> (traj, points, t_start, radius, ref) with ref[True] / ref[False] the
    restatement's (point, index, t) per row with and without wrap, and ref[None] those from t_start = 0 with wrap.  Computed
    once per process; nobody writes into it."""
    traj = race_line(N) if closed else open_line(N)
    pts, ts, radius, _ = intersect_case(traj, closed, B)
    ref = {w: [orc.intersect_point(pts[b], radius, traj, float(ts[b]), w) for b in range(B)] for w in (True, False)}
    ref[None] = [orc.intersect_point(pts[b], radius, traj, 0.0, True) for b in range(B)]
    return traj, pts, ts, radius, ref


def case_categories(traj, pts, ts, radius, ref):
    """count_categories of a case, with the exact roots of every row's first searched segment"""
    N = traj.shape[0]
    roots = []
    for b in range(pts.shape[0]):
        if int(ts[b]) < N - 1:
            S, V = segment_ends(traj, np.array([int(ts[b])]))
            t1, t2, _ = circle_roots(pts[b], radius, S, V)
            roots.append((float(t1[0]), float(t2[0])))
        else:
            roots.append((np.nan, np.nan))
    return count_categories(N, ts, ref[True], ref[False], roots)


# ------------------------------------------------------------------ table look-ups
def grid_lookup_scan(keys, shape, x):
    """per axis min(shape_d - 1, number of keys <= v), NaN counting as above every key; -> flat row-major index (Python int)"""
    flat = 0
    for d, v in enumerate(x):
        i = len(keys[d]) if v != v else sum(1 for k in keys[d] if k <= v)
        flat = flat * int(shape[d]) + min(int(shape[d]) - 1, i)
    return flat


def grid_axes(lens, seed=0):
    """sorted float64 keys per axis with the given lengths; every axis holds the key 0.0 (so that -0.0 meets it)"""
    rng = np.random.default_rng(seed)
    return [np.sort(np.concatenate([[0.0], rng.uniform(-2, 2, n - 1)])) for n in lens]


def grid_queries(axes, B, seed=0):
    """[B, D] float64: random in and around the key range, then rows that put, on one axis at a time, every key, the double
    below the first key, the double above the last key, +-Inf, -0.0 and NaN (the other axes random)"""
    rng = np.random.default_rng(seed + B)
    D = len(axes)
    lo = np.array([a[0] for a in axes]) - 0.5
    hi = np.array([a[-1] for a in axes]) + 0.5
    q = rng.uniform(lo, hi, size=(B, D))
    r = 0
    for d in range(D):
        a = axes[d]
        for v in [*a, np.nextafter(a[0], -np.inf), np.nextafter(a[-1], np.inf), np.inf, -np.inf, -0.0, np.nan]:
            if r >= B:
                return q
            q[r, d] = v
            r += 1
    return q


def nearest_bruteforce(inputs, q, ft=np.float64, chunk=1 << 16):
    """inputs [N,D], q [B,D] -> d2 [B,N] in dtype ft, the sum taken in index order of d as a plain loop would"""
    X, Q = np.asarray(inputs, ft), np.asarray(q, ft)
    out = np.empty((Q.shape[0], X.shape[0]), ft)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, X.shape[0], chunk):
            acc = np.zeros((Q.shape[0], min(chunk, X.shape[0] - s)), ft)
            for d in range(X.shape[1]):
                t = X[None, s:s + chunk, d] - Q[:, None, d]
                acc += t * t
            out[:, s:s + chunk] = acc
    return out
