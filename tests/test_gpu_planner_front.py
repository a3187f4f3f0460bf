"""The eight kernels of irbfn_amd/csrc/planner_front.hip at their own boundaries, against the restatements of
oracle/irbfn_oracle.py (held to high-precision statements of the operations by tests/test_planner_front_reference_cpu.py).

Every kernel is called through its C ABI on buffers that are NaN (or a sentinel integer) before the call and that carry GUARD
rows past B, which must come back untouched: an element a kernel leaves unwritten, or a row it writes past the batch, shows.
The Python wrappers are then held to the same bits.  Bounds:
  * Cartesian columns 1-2: |got - mpmath| <= ulp32(ref) / 2 + 8 x 2^-53 (|dx| + |dy|) (two products and one sum in float64 with
    sin / cos good to a few ulp, then one rounding to float32), and within one float32 ulp of the NumPy restatement; column 3
    and the pass-through columns bit for bit; flags equal to the sign of the mpmath gl1 outside the band 8 x 2^-53 (|dx| + |dy|).
  * Frenet, un-mirror, grid look-up, nearest_point, intersect_point: bit for bit.
  * lut_nearest: exact duplicates resolve to the lowest index bit for bit; otherwise the row found is at most 4 x the error of
    a float32 evaluation of the squared distances (measured per query) farther than the float64 minimum.
Each test prints its largest err / bound (pytest -s; profiles/planner_front_parity.txt)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _planner_front_util as pf
from irbfn_amd import _lib, explicit_planner, planner, planner_utils
from irbfn_amd.model import WCRBFNet, _ptr, _stream_ptr
from oracle import irbfn_oracle as orc

pytestmark = pytest.mark.gpu

GUARD = 4                                # rows past B in every buffer (a block of the way-point kernels holds four rows)
SENT = -77
NULL = C.c_void_p(None)
# share of the 2000 straight-ahead headings with gl1 == 0 and no mirror, measured on MI355X (profiles/planner_front_parity.txt)
STRAIGHT_AHEAD_MEASURED = 0.951


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _pad(a, dtype, fill=0.5):
    """the array with GUARD more rows of `fill`, on the device"""
    a = np.ascontiguousarray(a, dtype)
    return _dev(np.concatenate([a, np.full((GUARD,) + a.shape[1:], fill, dtype)]), dtype)


def _out(B, cols, dtype):
    shape = (B + GUARD,) + ((cols,) if cols else ())
    if dtype in (torch.int32, torch.int64):
        return torch.full(shape, SENT, dtype=dtype, device="cuda")
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _take(B, *bufs):
    """host copies of the first B rows; the guard rows must be as they were"""
    torch.cuda.synchronize()
    res = []
    for t in bufs:
        a = t.cpu().numpy()
        g = a[B:]
        assert (g == SENT).all() if a.dtype.kind == "i" else np.isnan(g).all(), "rows past B were written"
        res.append(a[:B])
    return res


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    nan = np.isnan(a) & np.isnan(b) if a.dtype.kind == "f" else np.zeros(a.shape, bool)
    bad = (a.view(u) != b.view(u)) & ~nan
    assert not bad.any(), (np.argwhere(bad)[:5].tolist(), a[bad][:5], b[bad][:5])


# ------------------------------------------------------------------ query builders
def call_cartesian(pose, goal, state0=True):
    B = pose.shape[0]
    x, s0, m = _out(B, 7, torch.float32), _out(B, 7, torch.float32), _out(B, 0, torch.int32)
    pd, gd = _pad(pose, np.float64), _pad(goal, np.float64)          # held until the results are back
    st = _lib.load().irbfn_plan_queries_cartesian(_ptr(pd), _ptr(gd), _ptr(x), _ptr(s0) if state0 else NULL, _ptr(m), B,
                                                  _stream_ptr(torch))
    assert st == 0
    x, s0, m = _take(B, x, s0, m)
    assert state0 or np.isnan(s0).all()
    return x, s0, m


def _check_column3_and_passthrough(x, m, pose, goal):
    with np.errstate(invalid="ignore"):
        gt = goal[:, 2] - pose[:, 4]
        c3 = np.where(m != 0, (-gt) % np.pi, gt % np.pi).astype(np.float32)
    _same_bits(x[:, 3], c3)
    _same_bits(x[:, [0, 4, 5, 6]], np.stack([pose[:, 3], goal[:, 3], pose[:, 6], pose[:, 5]], axis=1).astype(np.float32))


@pytest.mark.parametrize("B", [1, 255, 256, 257, 4099])
def test_cartesian_queries(gpu, B):
    pose, goal, special = pf.cartesian_case(B)
    x, s0, m = call_cartesian(pose, goal)
    x2, _, m2 = call_cartesian(pose, goal, state0=False)
    _same_bits(x, x2)
    np.testing.assert_array_equal(m, m2)
    wx, ws, wm = (t.cpu().numpy() for t in planner.build_queries(pose, goal))
    _same_bits(wx, x), _same_bits(ws, s0), np.testing.assert_array_equal(wm, m)
    _same_bits(s0, pose.astype(np.float32))
    assert np.isin(m, (0, 1)).all()
    _check_column3_and_passthrough(x, m, pose, goal)
    gl0, gl1, gt, mag = pf.rotate_mp(pose, goal)
    fin = np.isfinite(gl0)
    assert (m[~fin] == 0).all() and np.isnan(x[~fin][:, 1:4]).all()
    band = 8 * pf.U64 * mag
    clear = fin & (np.abs(gl1) > band)
    assert (~clear & fin).sum() <= len(special) + 0.01 * B
    np.testing.assert_array_equal(m[clear], (gl1[clear] < 0).astype(np.int32))
    g = x.astype(np.float64)
    r1 = np.abs(g[fin, 1] - gl0[fin]) / (pf.ulp32(gl0[fin]) / 2 + band[fin])
    r2 = np.abs(g[fin, 2] - np.abs(gl1[fin])) / (pf.ulp32(gl1[fin]) / 2 + band[fin])
    print(f"cartesian B={B}: err/bound column 1 {r1.max(initial=0):.3f}, column 2 {r2.max(initial=0):.3f}; "
          f"rows in the flag band {(~clear & fin).sum()}")
    assert r1.max(initial=0) <= 1 and r2.max(initial=0) <= 1
    with np.errstate(invalid="ignore"):
        ref = np.stack([orc.plan_query_cartesian(pose[b], goal[b], unfused=True)[0] for b in range(B)]).astype(np.float64)
    assert (np.abs(g[fin][:, 1:3] - ref[fin][:, 1:3]) <= pf.ulp32(ref[fin][:, 1:3])).all()
    assert (g[fin, 2] >= 0).all()
    if "gl1_neg_zero" in special:
        row = special["gl1_neg_zero"]
        assert m[row] == 0 and pf.bits32(x[row, 2]) == 0x80000000
    for name in ("gt_neg_zero", "gt_1pi_on", "gt_-1pi_on", "gt_pos_zero_mirrored"):
        if name in special:
            assert pf.bits32(x[special[name], 3]) == 0, name          # a zero remainder is +0.0, as in NumPy
    if "nan_pose" in special:
        assert not fin[special["nan_pose"]] and not fin[special["inf_pose"]] and fin[special["nan_pose"] + 1]


def test_goal_straight_ahead_does_not_mirror(gpu):
    """s * dx + c * dy is exactly 0 in NumPy at every heading; a fused multiply-add leaves the rounding error of one product and
    mirrors about half of the rows.  The device's sin / cos need not equal NumPy's at every heading, so the share of exact
    zeros is measured (profiles/planner_front_parity.txt) and at least half of it asserted; a fused kernel gives none."""
    pose, goal = pf.straight_ahead()
    x, _, m = call_cartesian(pose, goal)
    share = float(((x[:, 2] == 0) & (m == 0)).mean())
    print(f"straight ahead: gl1 == 0 and no mirror at {share:.4f} of {len(m)} headings; mirrored {float((m != 0).mean()):.4f}")
    _check_column3_and_passthrough(x, m, pose, goal)                   # every row consistent with the flag it reports
    assert (x[:, 2] >= 0).all() and (x[:, 2] <= 16 * pf.U64 * 4).all()
    assert (np.signbit(x[:, 2]) <= (m == 0)).all()
    assert np.abs(x[:, 1] - 2.0).max() <= pf.ulp32(2.0)
    assert share >= STRAIGHT_AHEAD_MEASURED / 2


@pytest.mark.parametrize("B", [1, 256, 257])
def test_frenet_queries(gpu, B):
    rng = np.random.default_rng(B)
    fr = np.stack([rng.uniform(0, 100, B), rng.uniform(-0.8, 0.8, B), rng.uniform(-0.4, 0.4, B), rng.uniform(0.5, 7, B),
                   rng.uniform(-1, 1, B), rng.uniform(-2, 2, B), rng.uniform(-0.6, 0.6, B), rng.uniform(-0.5, 0.5, B)], axis=1)
    ey = [np.nextafter(-0.05, -1.0), -0.05, np.nextafter(-0.05, 0.0), np.nan, -0.0, 0.0]
    fr[:len(ey), 1] = ey[:B]
    vg = rng.uniform(0.5, 7, B)
    lib = _lib.load()
    got = {}
    fd, vd = _pad(fr, np.float64), _pad(vg, np.float64)
    for with_s0 in (True, False):
        x, s0, m = _out(B, 8, torch.float32), _out(B, 8, torch.float32), _out(B, 0, torch.int32)
        assert lib.irbfn_plan_queries_frenet(_ptr(fd), _ptr(vd), _ptr(x), _ptr(s0) if with_s0 else NULL, _ptr(m), B,
                                             _stream_ptr(torch)) == 0
        got[with_s0] = _take(B, x, s0, m)
    x, s0, m = got[True]
    _same_bits(got[False][0], x), np.testing.assert_array_equal(got[False][2], m)
    assert np.isnan(got[False][1]).all()
    ref = [orc.plan_query_frenet(fr[b], vg[b]) for b in range(B)]
    _same_bits(x, np.stack([r[0] for r in ref]))
    _same_bits(s0, np.stack([r[2] for r in ref]))
    np.testing.assert_array_equal(m, np.array([r[1] for r in ref], np.int32))
    assert m[0] == 1 and (B < 6 or (m[1:6] == 0).all())
    wx, ws, wm = (t.cpu().numpy() for t in planner.build_queries_frenet(fr, vg))
    _same_bits(wx, x), _same_bits(ws, s0), np.testing.assert_array_equal(wm, m)


@pytest.mark.parametrize("O,sv0", [(2, 1), (10, 5), (16, 8), (100, 50)])
@pytest.mark.parametrize("B", [1, 256, 257])
def test_unmirror_flips_the_sign_bit_of_the_steering_controls(gpu, B, O, sv0):
    """un-mirror through the controls-only planning tick: the controls with flags equal, bit for bit, the controls without
    flags with the sign bit of columns [sv0, O) of the flagged rows flipped -- a +0.0 column becomes -0.0, a NaN row stays NaN."""
    rng = np.random.default_rng(B + O)
    D, K = 7, 64
    cfg = {"in_features": D, "out_features": O, "num_kernels": K, "basis_func": "gaussian", "num_regions": 1,
           "lower_bounds": [[-1.0]] * D, "upper_bounds": [[1.0]] * D, "dimension_ranges": [[0] * D],
           "activation_idx": list(range(D)), "delta": [5.0] * D}
    W = (rng.normal(size=(K, O)) * 0.2).astype(np.float32)
    bias = (rng.normal(size=(O,)) * 0.1).astype(np.float32)
    W[:, O - 1], bias[O - 1] = 0.0, 0.0                               # a control that is exactly zero
    P = {"params": {"rbf_list": {"centers": rng.uniform(-1.2, 1.2, size=(1, K, D)).astype(np.float32),
                                 "log_sigs": rng.uniform(-0.5, 0.3, size=(1, K)).astype(np.float32)},
                    "linear": {"kernel": W, "bias": bias}}}
    x = rng.uniform(-1, 1, size=(B, D)).astype(np.float32)
    x[B // 2] = np.nan                                                # a NaN row of controls
    mirror = rng.choice(np.array([0, 0, 1, -1, 7, -2 ** 31], np.int64), size=B).astype(np.int32)
    mirror[B // 2], mirror[0] = 1, 1
    net = WCRBFNet.from_config(cfg)
    xt = torch.from_numpy(x).cuda()
    plain, none = planner.plan_tick(net, P, xt, None, rollout=False)
    plain = plain.cpu().numpy()
    flipped, _ = planner.plan_tick(net, P, xt, torch.from_numpy(mirror).cuda(), rollout=False)
    assert none is None and (plain[np.arange(B) != B // 2, O - 1] == 0).all() and np.isnan(plain[B // 2]).any()
    want = plain.view(np.uint32).copy()
    want[np.ix_(mirror != 0, np.arange(sv0, O))] ^= np.uint32(0x80000000)
    got = flipped.cpu().numpy()
    np.testing.assert_array_equal(got.view(np.uint32), want)
    np.testing.assert_array_equal(got, orc.unmirror_controls(plain, mirror, sv0))
    assert (B * (O - sv0)) % 256 != 0 or B == 256


# ------------------------------------------------------------------ grid look-up
def call_grid(axes, shape, q, table=None):
    """irbfn_lut_grid_lookup -> (idx [B], out [B, OW] or None)"""
    B, D = q.shape
    off = (C.c_int32 * (D + 1))(*np.concatenate(([0], np.cumsum([len(a) for a in axes]))).astype(np.int32))
    shp = (C.c_int32 * D)(*shape)
    keys = _dev(np.concatenate(axes), np.float64)
    idx = _out(B, 0, torch.int64)
    OW = 0 if table is None else table.shape[1]
    out = _out(B, OW, torch.float32) if OW else None
    tab = _dev(table, np.float32) if OW else None
    qd = _pad(q, np.float64)
    st = _lib.load().irbfn_lut_grid_lookup(_ptr(keys), off, shp, _ptr(tab) if OW else NULL, _ptr(qd), _ptr(idx),
                                           _ptr(out) if OW else NULL, B, D, OW, _stream_ptr(torch))
    assert st == 0
    if OW:
        idx, out = _take(B, idx, out)
        return idx, out
    return _take(B, idx)[0], None


GRID_LENS = {1: (17,), 7: (17, 3, 2, 1, 1, 2, 3), 16: (1, 2, 3, 17, 1, 2, 1, 2, 1, 1, 2, 1, 1, 3, 1, 2)}


@pytest.mark.parametrize("B", [1, 256, 257])
@pytest.mark.parametrize("D", [1, 7, 16])
def test_grid_lookup(gpu, D, B):
    axes = pf.grid_axes(GRID_LENS[D], seed=D)
    rng = np.random.default_rng(D)
    qall = pf.grid_queries(axes, 257, seed=D)
    q = qall[rng.permutation(257)[:B]] if B < 257 else qall
    for shape in ([len(a) for a in axes], [max(1, len(a) - 1) for a in axes]):     # the second: shape[d] < len(keys)
        table = rng.normal(size=(int(np.prod(shape)), 3)).astype(np.float32)
        idx, out = call_grid(axes, shape, q, table)
        ref = np.array([orc.lut_grid_lookup(axes, shape, q[b])[1] for b in range(B)], np.int64)
        np.testing.assert_array_equal(idx, ref)
        _same_bits(out, table[ref])
        idx2, _ = call_grid(axes, shape, q)                                       # index only
        np.testing.assert_array_equal(idx2, ref)
    if B == 257:
        assert np.isnan(q).any() and np.isinf(q).any() and (np.signbit(q) & (q == 0)).any()
    if D == 7:                                                                    # the wrapper, on the same full grid
        inputs = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, D)
        shape = [len(a) for a in axes]
        outputs = rng.normal(size=(inputs.shape[0], 2, 2))
        tab = explicit_planner.ExplicitTable(inputs, outputs)
        assert tab.is_grid and tab.shape == shape
        widx, wout = tab.grid_lookup(q)
        ref = np.array([orc.lut_grid_lookup(axes, shape, q[b])[1] for b in range(B)], np.int64)
        np.testing.assert_array_equal(widx.cpu().numpy(), ref)
        _same_bits(wout.cpu().numpy(), outputs.reshape(len(inputs), -1).astype(np.float32)[ref])


def test_grid_lookup_index_past_2_to_31(gpu):
    """D = 8 with 16 keys per axis: 2^32 cells; the flat index only (no table)"""
    axes = pf.grid_axes((16,) * 8, seed=8)
    q = pf.grid_queries(axes, 257, seed=8)
    q[200:] = np.array([a[-1] for a in axes]) + 1.0                               # the last cell: 2^32 - 1
    q[200:, 7] = np.random.default_rng(0).uniform(-2, 2, 57)
    shape = [16] * 8
    idx, _ = call_grid(axes, shape, q)
    ref = np.array([orc.lut_grid_lookup(axes, shape, q[b])[1] for b in range(257)], np.int64)
    assert (ref >= 2 ** 31).sum() > 57 and ref.max() >= 2 ** 32 - 16
    np.testing.assert_array_equal(idx, ref)


# ------------------------------------------------------------------ exact nearest neighbour
def call_nearest(inputs_dev, table_dev, q, N, D, OW):
    B = q.shape[0]
    lib = _lib.load()
    need = lib.irbfn_lut_nearest_workspace_bytes(N, B)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    idx, dist, out = _out(B, 0, torch.int64), _out(B, 0, torch.float32), _out(B, OW, torch.float32)
    qd = _pad(q, np.float32)
    st = lib.irbfn_lut_nearest(_ptr(inputs_dev), _ptr(table_dev), _ptr(qd), _ptr(idx), _ptr(dist), _ptr(out), N, B, D, OW,
                               _ptr(ws), need, _stream_ptr(torch))
    assert st == 0
    return _take(B, idx, dist, out)


def nearest_case(D, N):
    """-> (inputs [N,D] f32, q [9,D] f32, planted [8,D]): queries 0-3 have an exact copy of themselves planted at row 0, N - 1,
    the first row of the last (partial) block and in the grid-stride tail (past 2048 x 256 rows; else N / 2); queries 4-7 have
    their nearest row (the query + 2^-10) planted TWICE -- in neighbouring lanes, in two waves, in two blocks as far apart as N
    allows up to 70 (70 at N = 524 588: past the final kernel's stride of 64; 63 at N = 16 385, whose 65th block holds one row,
    and that row is the planted copy of query 2) and in two grid-stride rounds (else near both ends); query 8 is left alone.
    Where a small N makes plants collide the later one stays; the test reads the expected rows off the table."""
    rng = np.random.default_rng(1000 * D + N % 9973)
    inputs = rng.uniform(-3, 3, size=(N, D)).astype(np.float32)
    q = rng.uniform(-3.2, 3.2, size=(9, D)).astype(np.float32)
    last = ((N - 1) // 256) * 256
    tail = 524288 + 7 if N > 524288 + 7 else N // 2
    blocks = min(70, max(1, (N - 1 - 90) // 256))
    pairs = [(70, 71), (80, 80 + 64), (90, 90 + 256 * blocks), (100, 100 + 524288 if N > 100 + 524288 else N - 2)]
    planted = np.concatenate([q[:4], q[4:8] + np.float32(2.0 ** -10)])
    for b, pair in zip(range(4, 8), pairs):
        for n in pair:
            inputs[min(max(n, 0), N - 1)] = planted[b]
    for b, n in zip(range(4), (0, N - 1, last, tail)):
        inputs[n] = planted[b]
    return inputs, q, planted


def _dist_bound(tol, true):
    """bound on |sqrtf(d2) - true| when the float32 d2 is within tol of true^2: tol / true (sqrt(tol) near 0) + one rounding"""
    return tol / max(true, np.sqrt(tol), 1e-30) + 2.0 ** -23 * true


@pytest.mark.parametrize("N", [1, 255, 256, 257, 16385, 524288 + 300])
@pytest.mark.parametrize("D", [3, 4, 7, 8])
def test_lut_nearest(gpu, D, N):
    OW = 3
    inputs, q, planted = nearest_case(D, N)
    table = np.random.default_rng(N).normal(size=(N, OW)).astype(np.float32)
    ind, tab = _dev(inputs, np.float32), _dev(table, np.float32)
    idx, dist, out = call_nearest(ind, tab, q, N, D, OW)
    d64 = pf.nearest_bruteforce(inputs, q)
    d32 = pf.nearest_bruteforce(inputs, q, np.float32)
    tol = 4 * np.abs(d32.astype(np.float64) - d64).max(axis=1)            # per query: the float32 twin's error of a squared distance
    ri = d64.argmin(axis=1)
    worst = 0.0
    for b in range(9):
        gi = int(idx[b])
        assert 0 <= gi < N
        assert d64[b, gi] - d64[b, ri[b]] <= tol[b], (b, gi, ri[b])       # another row only as a float32 near-tie
        same = np.flatnonzero((inputs == inputs[gi]).all(axis=1))
        assert gi == same[0], (b, gi, same[:4])                           # exact duplicates: the lowest index
        true = np.sqrt(d64[b, gi])
        bound = _dist_bound(tol[b], true)
        worst = max(worst, abs(float(dist[b]) - true) / bound if bound else float(dist[b] != true))
        assert abs(float(dist[b]) - true) <= bound
        if tol[b] > 0 and gi != ri[b]:
            worst = max(worst, (d64[b, gi] - d64[b, ri[b]]) / tol[b])
    _same_bits(out, table[idx])
    for b in range(8):                                                    # the planted rows: the lowest index that holds them
        rows = np.flatnonzero((inputs == planted[b]).all(axis=1))
        if rows.size:
            assert idx[b] == rows[0] and (b >= 4 or dist[b] == 0), (b, idx[b], rows[:4])
    if N > 524288:
        np.testing.assert_array_equal(idx[:8], [0, N - 1, ((N - 1) // 256) * 256, 524288 + 7, 70, 80, 90, 100])
    print(f"lut_nearest D={D} N={N}: rows other than the float64 argmin {(idx != ri).sum()} of 9, largest err/bound {worst:.3f}")
    for B in (1, 7, 8):                                                   # a query's answer does not depend on its tile
        for lo in (range(9) if B == 1 else (0, 9 - B)):
            i2, d2, o2 = call_nearest(ind, tab, q[lo:lo + B], N, D, OW)
            np.testing.assert_array_equal(i2, idx[lo:lo + B])
            _same_bits(d2, dist[lo:lo + B]), _same_bits(o2, out[lo:lo + B])
    if N == 257:                                                          # the wrapper
        t = explicit_planner.ExplicitTable(inputs, table.reshape(N, 1, OW))
        wi, wd, wo = (v.cpu().numpy() for v in t.nearest(q))
        np.testing.assert_array_equal(wi, idx), _same_bits(wd, dist), _same_bits(wo, out)


@pytest.mark.parametrize("D", [3, 4, 7, 8])
def test_lut_nearest_without_a_finite_distance(gpu, D):
    """a NaN or Inf query gets index -1, distance NaN and a NaN row, its neighbours their answers; an Inf or NaN table row is
    never chosen; a table of Inf rows gives -1 for every query"""
    rng = np.random.default_rng(D)
    N, OW = 1000, 5
    inputs = rng.uniform(-3, 3, size=(N, D)).astype(np.float32)
    q = rng.uniform(-3, 3, size=(9, D)).astype(np.float32)
    inputs[0, 0], inputs[500, D - 1], inputs[999, 0], inputs[300] = np.inf, -np.inf, np.nan, np.nan
    bad = {1: np.nan, 3: np.inf, 4: -np.inf, 8: np.nan}
    for b, v in bad.items():
        q[b, b % D] = v
    table = rng.normal(size=(N, OW)).astype(np.float32)
    ind, tab = _dev(inputs, np.float32), _dev(table, np.float32)
    idx, dist, out = call_nearest(ind, tab, q, N, D, OW)
    d64 = pf.nearest_bruteforce(inputs, q)
    with np.errstate(invalid="ignore"):
        d32 = pf.nearest_bruteforce(inputs, q, np.float32).astype(np.float64)
        err = np.abs(d32 - d64)
    tol = 4 * np.where(np.isfinite(err), err, 0.0).max(axis=1)           # the float32 twin's error over the finite rows
    d64[~np.isfinite(d64)] = np.inf
    for b in range(9):
        if b in bad:
            assert idx[b] == -1 and np.isnan(dist[b]) and np.isnan(out[b]).all()
        else:
            assert idx[b] == d64[b].argmin() and idx[b] not in (0, 300, 500, 999)
            _same_bits(out[b], table[idx[b]])
            true = np.sqrt(d64[b].min())
            assert abs(dist[b] - true) <= _dist_bound(tol[b], true)
    wi, wd, wo = (v.cpu().numpy() for v in explicit_planner.ExplicitTable(inputs, table.reshape(N, 1, OW)).nearest(q))
    np.testing.assert_array_equal(wi, idx), _same_bits(wd, dist), _same_bits(wo, out)
    inf = _dev(np.full((3, D), np.inf), np.float32)
    idx, dist, out = call_nearest(inf, tab, q, 3, D, OW)
    assert (idx == -1).all() and np.isnan(dist).all() and np.isnan(out).all()


def test_lut_nearest_refuses_a_batch_past_the_grid(gpu):
    """B = 2^34 needs 2^31 query tiles: more than any grid holds.  Refused before anything is touched: the buffers are dummies."""
    lib = _lib.load()
    B, N = 2 ** 34, 1000
    buf = [torch.full((16,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(6)]
    idx = torch.full((16,), SENT, dtype=torch.int64, device="cuda")
    st = lib.irbfn_lut_nearest(_ptr(buf[0]), _ptr(buf[1]), _ptr(buf[2]), _ptr(idx), _ptr(buf[3]), _ptr(buf[4]), N, B, 8, 1,
                               _ptr(buf[5]), lib.irbfn_lut_nearest_workspace_bytes(N, B), _stream_ptr(torch))
    torch.cuda.synchronize()
    assert st == -1                                                        # IRBFN_ERR_BAD_ARG
    assert all(torch.isnan(t).all() for t in buf) and (idx == SENT).all()


# ------------------------------------------------------------------ nearest point on a polyline
def call_nearest_point(pts, traj):
    B, N = pts.shape[0], traj.shape[0]
    proj, dist, t, seg = _out(B, 2, torch.float64), _out(B, 0, torch.float64), _out(B, 0, torch.float64), _out(B, 0, torch.int32)
    pd, td = _pad(pts, np.float64), _dev(traj, np.float64)
    st = _lib.load().irbfn_nearest_point(_ptr(pd), _ptr(td), _ptr(proj), _ptr(dist), _ptr(t), _ptr(seg), B, N, _stream_ptr(torch))
    assert st == 0
    return _take(B, proj, dist, t, seg)


def nearest_point_case(N, variant, B):
    """-> (traj, points, ties {row: segment that must win}): random points about the line, then as far as B and N allow the
    exact ties: off the corners at way-points 1, 64 and 65 (segments 0 / 1, 63 / 64, 64 / 65), on those way-points, on and off
    the shared first / last way-point of the closed line, and a NaN point."""
    rng = np.random.default_rng(N + B)
    traj = pf.staircase(N, variant)
    pts = traj[rng.integers(0, N, B)] + np.round(rng.normal(size=(B, 2)) * 3) / 4 + rng.normal(size=(B, 2)) * (rng.random((B, 1)) < 0.5)
    ties = {}
    rows = iter(range(B))
    if variant == "open":
        for k in (1, 64, 65):
            if k < N - 1:
                for p in (pf.corner_tie_point(traj, k), traj[k]):
                    r = next(rows, None)
                    if r is not None:
                        pts[r], ties[r] = p, k - 1
    if variant == "closed" and N >= 4:
        for p in (traj[0], traj[0] + [-0.25, 0.25]):
            r = next(rows, None)
            if r is not None:
                pts[r], ties[r] = p, 0
    if B >= 5:
        pts[B - 2] = np.nan
        ties.pop(B - 2, None)
    return traj, pts, ties


def _check_nearest_point(traj, pts, ties=()):
    got = call_nearest_point(pts, traj)
    with np.errstate(invalid="ignore", divide="ignore"):
        ref = [orc.nearest_point(pts[b], traj, skip_nan=True) for b in range(pts.shape[0])]
    want = (np.stack([r[0] for r in ref]), np.array([r[1] for r in ref]), np.array([r[2] for r in ref], np.float64),
            np.array([r[3] for r in ref], np.int32))
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)                               # NaN equal to NaN
    for r, k in dict(ties).items():
        assert got[3][r] == k
    wrapped = [v.cpu().numpy() for v in planner_utils.nearest_point(pts, traj)]
    for g, w in zip(got, wrapped):
        np.testing.assert_array_equal(g, w)
    return got


@pytest.mark.parametrize("B", [1, 2, 3, 5, 500])
@pytest.mark.parametrize("N", [2, 3, 64, 65, 66, 129, 200])
def test_nearest_point(gpu, N, B):
    for variant in ("open", "closed", "replay"):
        if (variant == "closed" and N < 4) or (variant == "replay" and N < 66):
            continue
        traj, pts, ties = nearest_point_case(N, variant, B)
        got = _check_nearest_point(traj, pts, ties)
        if variant == "replay":
            assert (got[3] < 64).all()                                      # the first of the coinciding segments


def test_nearest_point_skips_nan_segments(gpu):
    """a repeated way-point (t = 0 / 0), a NaN way-point, and nothing but NaN: the documented defaults"""
    rng = np.random.default_rng(3)
    for N in (10, 130):
        traj = pf.staircase(N)
        traj[4] = traj[3]
        traj[N - 3] = np.nan
        pts = traj[rng.integers(0, N - 4, 7)] + rng.normal(size=(7, 2))
        pts[0] = traj[3]
        got = _check_nearest_point(traj, pts)
        assert np.isfinite(got[1]).all() and not np.isin(got[3], (3, N - 4, N - 3)).any()
        with np.errstate(invalid="ignore", divide="ignore"):
            assert orc.nearest_point(pts[1], traj)[3] == 3                 # np.argmin: the first NaN
        proj, dist, t, seg = _check_nearest_point(np.full((N, 2), np.nan), pts)
        assert (proj == 0).all() and (dist == np.inf).all() and (t == 0).all() and (seg == 0).all()


# ------------------------------------------------------------------ circle / polyline intersection
def call_intersect(pts, radius, traj, ts, wrap):
    B, N = pts.shape[0], traj.shape[0]
    fp, fi, ft, found = _out(B, 2, torch.float32), _out(B, 0, torch.int32), _out(B, 0, torch.float32), _out(B, 0, torch.int32)
    pd, td = _pad(pts, np.float64), _dev(traj, np.float64)
    sd = _pad(ts, np.float64) if ts is not None else None
    st = _lib.load().irbfn_intersect_point(_ptr(pd), _ptr(td), _ptr(sd) if ts is not None else NULL, float(radius), int(wrap),
                                           _ptr(fp), _ptr(fi), _ptr(ft), _ptr(found), B, N, _stream_ptr(torch))
    assert st == 0
    return _take(B, fp, fi, ft, found)


def _check_intersect(got, ref):
    fp, fi, ft, found = got
    hit = np.array([r[1] is not None for r in ref])
    np.testing.assert_array_equal(found, hit.astype(np.int32))
    assert np.isnan(fp[~hit]).all() and np.isnan(ft[~hit]).all()
    rows = np.flatnonzero(hit)
    if rows.size:
        np.testing.assert_array_equal(fi[rows], np.array([ref[b][1] for b in rows], np.int32))
        _same_bits(ft[rows], np.array([ref[b][2] for b in rows], np.float32))
        _same_bits(fp[rows], np.stack([ref[b][0] for b in rows]).astype(np.float32))


@pytest.mark.parametrize("B", [1, 3, 500])
@pytest.mark.parametrize("N", [2, 3, 65, 200])
@pytest.mark.parametrize("closed", [False, True])
def test_intersect_point(gpu, closed, N, B):
    traj, pts, ts, radius, ref = pf.intersect_reference(closed, N, B if N >= 65 else min(B, 60))
    B = pts.shape[0]
    for wrap in (True, False):
        got = call_intersect(pts, radius, traj, ts, wrap)
        _check_intersect(got, ref[wrap])
        wrapped = [v.cpu().numpy() for v in planner_utils.intersect_point(pts, radius, traj, ts, wrap=wrap)]
        hit = got[3] != 0
        for g, w in zip(got, wrapped):
            np.testing.assert_array_equal(g[hit], w[hit])
        np.testing.assert_array_equal(got[3], wrapped[3])
    _check_intersect(call_intersect(pts, radius, traj, None, True), ref[None])      # t_start = NULL: from the first segment
    if N == 200 and B == 500:
        n = pf.case_categories(traj, pts, ts, radius, ref)
        assert all(c >= 40 for name, c in n.items() if closed or name != "wrap_closing"), n
