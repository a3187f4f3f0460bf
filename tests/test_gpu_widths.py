"""The width stage on the GPU (run on the MI355X box with ``-m gpu``): irbfn_knn_d2 through the C ABI against the float64
statement of it (tests/_widths_util.py), then the width rules, ``NormalEquations.rss_of`` and ``select_scale`` end to end.  Every
output buffer is prefilled with a sentinel and carries guard elements past N * p that must come back untouched; the rows and the
centres carry NaN guard rows past N and K that must not be read; the workspace is prefilled with 0x5A and carries a guarded tail.

Bounds (derived in _widths_util): slot j's d2 within gamma relative of the reference's j-th smallest, d2_ref[n, idx[j]] <=
(1 + 3 gamma) times it, gamma = (D + 2) 2^-23; the list ascends in (d2, idx); the indices are distinct, below K and never the
excluded one; the empty slots are exactly the reference's.  Widths within 2 gamma + 2^-24 relative of the float64 rule on the
kernel's own lists / labels.

Largest err / bound over the 19 cases of test_shape_edges_meet_the_float64_statement (printed by the test): slot d2 0.472 (N = 1000,
K = 2, D = 1, p = 3), chosen centre 0.000 (every slot names the float64 statement's centre); the width rules on the kernel's own lists
/ labels: nearest_neighbour 0.043, cluster_spread 0.047.  End to end (s = 0.05 and s = 20 alike): held-out MSE 7.7e-2 / 1.1e-2 / 5.1e-4 /
1.0e-3 / 9.8e-3 at scales 0.5 .. 8 against 0.135 / 0.342 at log_sigs = 0; net.apply on the held-out rows 5.14148e-4 / 5.14151e-4
against 5.14147e-4 from the Gram matrix alone (profiles/widths.txt has the times)."""
import functools

import numpy as np
import pytest
import torch

import _kmeans_util as ku
import _widths_util as wu
from irbfn_amd import _lib, kmeans, linear_fit, widths
from irbfn_amd.model import WCRBFNet, _ptr, _stream_ptr

pytestmark = pytest.mark.gpu
GUARD = 3
SENT_I = -7
SPLITS = (0, 1, 2, 3, 5, 1000)


class Knn:
    """One irbfn_knn_d2 call on guarded, prefilled buffers; the outputs as NumPy arrays."""

    def __init__(self, q, c, p, self0=-1, split=0, want_idx=True, q_offset=0):
        """q_offset: floats by which the rows are moved off their 16-byte aligned allocation (NaN in front of them)."""
        lib = _lib.load()
        q, c = np.ascontiguousarray(q, np.float32), np.ascontiguousarray(c, np.float32)
        N, D = q.shape
        K = c.shape[0]
        flat = np.concatenate([np.full(q_offset, np.nan, np.float32), q.ravel(), np.full(GUARD * D, np.nan, np.float32)])
        qg = torch.from_numpy(flat).cuda()[q_offset:]
        assert qg.data_ptr() % 16 == (4 * q_offset) % 16
        cg = torch.from_numpy(np.vstack([c, np.full((GUARD, D), np.nan, np.float32)])).cuda()
        self.t_d2 = torch.full((N * p + GUARD,), -5.0, dtype=torch.float32, device="cuda")
        self.t_idx = torch.full((N * p + GUARD,), SENT_I, dtype=torch.int32, device="cuda") if want_idx else None
        need = lib.irbfn_knn_workspace_bytes(N, K, D, p, split)
        assert need > 0
        ws = torch.full((need + 8 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda")     # the kernels must not rely on a cleared workspace
        st = lib.irbfn_knn_d2(_ptr(qg), _ptr(cg), N, K, D, p, self0, split, _ptr(self.t_d2), _ptr(self.t_idx) if want_idx else None,
                              _ptr(ws), need, _stream_ptr(torch))
        assert st == 0, st
        torch.cuda.synchronize()
        assert (ws[need:] == 0x5A).all() and (self.t_d2[N * p:] == -5.0).all()
        self.d2 = self.t_d2[:N * p].cpu().numpy().reshape(N, p)
        self.idx = None
        if want_idx:
            assert (self.t_idx[N * p:] == SENT_I).all()
            self.idx = self.t_idx[:N * p].cpu().numpy().reshape(N, p)

    def raw(self):
        """Every output as bytes, for bit-for-bit comparisons."""
        return tuple(t.cpu().numpy().tobytes() for t in (self.t_d2, self.t_idx) if t is not None)


def check_knn(r, d2r, idxr, full, D, self0=-1):
    """Holds one call's lists to the float64 statement; returns the largest (slot d2, chosen centre) error over bound."""
    N, p = d2r.shape
    K = full.shape[1]
    g = ku.gamma(D)
    empty = idxr < 0
    assert np.array_equal(r.idx < 0, empty) and (r.idx[empty] == -1).all() and np.isnan(r.d2[empty]).all()      # exactly the reference's
    assert (r.idx < K).all() and np.isfinite(r.d2[~empty]).all()
    worst = [0.0, 0.0]
    for n in range(N):
        m = int((~empty[n]).sum())
        ks, ds = r.idx[n, :m], r.d2[n, :m].astype(np.float64)
        assert len(set(ks.tolist())) == m and (self0 < 0 or self0 + n not in ks)
        assert all((ds[j], ks[j]) < (ds[j + 1], ks[j + 1]) for j in range(m - 1))      # the kernel's own list ascends in (d2, idx)
        want = d2r[n, :m]
        err = np.abs(ds - want)
        assert (err <= g * want).all(), (n, ds, want)
        chosen = full[n, ks]
        assert (chosen <= want * (1 + 3 * g)).all(), (n, chosen, want)
        pos = want > 0
        if pos.any():
            worst[0] = max(worst[0], float((err[pos] / (g * want[pos])).max()))
            worst[1] = max(worst[1], float(((chosen[pos] / want[pos] - 1) / (3 * g)).max()))
    return worst


@pytest.mark.parametrize("case", wu.KNN_CASES, ids=lambda c: "N%d-K%d-D%d-p%d-self%d" % c)
def test_shape_edges_meet_the_float64_statement(gpu, case):
    N, K, D, p, self0 = case
    q, c, d2r, idxr, full = wu.knn_case(*case)
    r = Knn(q, c, p, self0)
    w = check_knn(r, d2r, idxr, full, D, self0)
    bare = Knn(q, c, p, self0, want_idx=False)                          # idx is optional
    assert bare.raw()[0] == r.raw()[0]
    print(f"knn N={N} K={K} D={D} p={p} self0={self0}: largest err/bound slot d2 {w[0]:.3f} chosen centre {w[1]:.3f}")


@pytest.mark.parametrize("case", ["integer", "ties"])
def test_exact_cases_equal_the_reference(gpu, case):
    x, c = ku.integer_case() if case == "integer" else ku.tie_case()
    c = c.copy()
    c[-1] = c[3]                                                       # a centre duplicated bit for bit: the lower index comes first
    x = x[:700]
    full = ku.d2_ref(x, c)
    for p in (1, 3, 8):
        d2r, idxr = wu.knn_ref(x, c, p, d2=full)
        r = Knn(x, c, p)
        assert np.array_equal(r.idx, idxr)                             # ties included
        assert np.array_equal(r.d2.astype(np.float64), d2r)            # every operation of the chain is exact here
    if case == "ties":
        srt = np.sort(full, axis=1)
        assert ((srt[:, 1:8] == srt[:, :7]).any(axis=1)).sum() > 300


def _kmeans_assign(x, c):
    lab, d2 = kmeans.assign(x, c)
    return lab.cpu().numpy(), d2.cpu().numpy()


def test_p1_is_the_assignment_of_kmeans_step_bit_for_bit(gpu):
    for N, K, D in ((1000, 257, 8), (700, 9, 3), (257, 1025, 7)):
        x, c = ku.uniform_case(N, K, D, seed=31 + D)
        x, c = x.copy(), c.copy()
        x[5, 1] = np.nan
        x[64] = np.inf
        x[200, 0] = -np.inf
        x[N - 1, 2] = np.nan
        x[100] = 3.0e38                                                # finite, but every float32 d2 overflows
        c[2, 1] = np.nan
        c[7] = np.inf
        lab, d2 = _kmeans_assign(x, c)
        for split in (0, 1, 3):
            r = Knn(x, c, 1, split=split)
            assert np.array_equal(r.idx[:, 0], lab) and r.d2[:, 0].tobytes() == d2.tobytes()
        assert (lab[[5, 64, 100, 200, N - 1]] == -1).all() and not np.isin(lab, (2, 7)).any()
        r3 = Knn(x, c, 3)                                              # the non-finite rows and centres leave empty slots and nothing else
        assert (r3.idx[[5, 64, 100, 200, N - 1]] == -1).all() and np.isnan(r3.d2[[5, 64, 100, 200, N - 1]]).all()
        assert not np.isin(r3.idx, (2, 7)).any() and r3.d2[:, 0].tobytes() == d2.tobytes()


@pytest.mark.parametrize("p", (2, 16))
@pytest.mark.parametrize("shape", ((1025, 1025, 0), (65, 1025, -1)))
def test_split_invariance_and_repeats(gpu, shape, p):
    N, K, self0 = shape
    x, c = ku.uniform_case(N, K, 8, seed=41)
    q = c[:N] if self0 >= 0 else x
    first = Knn(q, c, p, self0, split=SPLITS[0]).raw()
    for split in SPLITS:
        assert Knn(q, c, p, self0, split=split).raw() == first, split
        assert Knn(q, c, p, self0, split=split).raw() == first, split
    d2r, idxr = wu.knn_ref(q, c, p, self0)
    check_knn(Knn(q, c, p, self0, split=5), d2r, idxr, ku.d2_ref(q, c), 8, self0)


def test_grid_stride_runs_twice(gpu):
    """The list pass launches at most 2048 blocks of 512 rows: with the 9 tiles of K = 1025 as 9 segments that is 227 row blocks, and
    227 * 512 + 5 rows take the grid-stride loop a second time.  One segment (228 blocks, one trip) must give the same bytes."""
    N, K, D, p = 227 * 512 + 5, 1025, 3, 2
    x, c = ku.uniform_case(N, K, D, seed=11)
    a = Knn(x, c, p, split=1000)
    assert a.raw() == Knn(x, c, p, split=1).raw()
    tail = slice(N - 300, N)
    full = ku.d2_ref(x[tail], c)
    d2r, idxr = wu.knn_ref(x[tail], c, p, d2=full)
    a.d2, a.idx = a.d2[tail], a.idx[tail]
    check_knn(a, d2r, idxr, full, D)


def test_merge_pass_strides_its_grid(gpu):
    """The merge launches at most 2048 blocks of 256 rows; 2048 * 256 + 5 rows in two segments take its loop a second time."""
    N, K, D, p = 2048 * 256 + 5, 129, 1, 2
    x, c = ku.uniform_case(N, K, D, seed=12)
    a = Knn(x, c, p, split=2)
    assert a.raw() == Knn(x, c, p, split=1).raw()
    tail = slice(N - 300, N)
    full = ku.d2_ref(x[tail], c)
    d2r, idxr = wu.knn_ref(x[tail], c, p, d2=full)
    a.d2, a.idx = a.d2[tail], a.idx[tail]
    check_knn(a, d2r, idxr, full, D)


@pytest.mark.parametrize("D", (4, 8, 16))
def test_rows_off_the_16_byte_boundary_take_the_scalar_loads(gpu, D):
    """D a multiple of 4 reads its rows with 16-byte loads only where the table is aligned; one, two and three floats off it the
    same rows must give the same bytes."""
    N, K, p = 300, 257, 3
    x, c = ku.uniform_case(N, K, D, seed=13)
    want = Knn(x, c, p).raw()
    for off in (1, 2, 3):
        assert Knn(x, c, p, q_offset=off).raw() == want, off
    selfwant = Knn(c, c, p, self0=0, split=2).raw()
    assert Knn(c, c, p, self0=0, split=2, q_offset=1).raw() == selfwant


def test_cluster_sums_repeat_bit_for_bit_over_many_tiles(gpu):
    """2^20 rows, far more than one tile of any device scan: the float64 sums themselves, not the rounded widths, must repeat bit for
    bit, and sit within count 2^(e - S - 1) (S = 62 - 21) plus one rounding of the exact sums."""
    N, K = 1 << 20, 1000
    rng = np.random.default_rng(14)
    x = rng.uniform(-3, 3, (N, 8)).astype(np.float32)
    c = x[rng.choice(N, K, replace=False)]
    lab, d2 = kmeans.assign(x, c)
    d64 = d2.to(torch.float64)
    sums, counts = widths.cluster_sums(d64, lab, K)
    for _ in range(4):
        s2, c2 = widths.cluster_sums(d64, lab, K)
        assert torch.equal(s2, sums) and torch.equal(c2, counts)
    perm = torch.randperm(N, device="cuda")                            # another order of the rows: the same integers
    s3, _ = widths.cluster_sums(d64[perm], lab[perm], K)
    assert torch.equal(s3, sums)
    ln, dn = lab.cpu().numpy(), d2.cpu().numpy().astype(np.float64)
    want = np.bincount(ln, weights=dn, minlength=K)
    cn = np.bincount(ln, minlength=K)
    assert np.array_equal(counts.cpu().numpy(), cn)
    e = np.frexp(dn.max())[1]
    assert (np.abs(sums.cpu().numpy() - want) <= cn * 2.0 ** (e - 41 - 1) + cn * 2.0 ** -52 * want).all()
    a = widths.cluster_spread(x, c).sigma
    assert torch.equal(a, widths.cluster_spread(x, c).sigma)


def test_self_exclusion(gpu):
    c = wu.duplicate_case()
    K = len(c)
    d2, idx = widths.knn(c, c, 3, exclude_self=True)
    whole = (d2.cpu().numpy(), idx.cpu().numpy())
    assert not (whole[1] == np.arange(K)[:, None]).any()
    # duplicated centres: slot 0 = (0.0, the other index)
    assert whole[1][[2, 7, 30, 31], 0].tolist() == [7, 2, 31, 30] and (whole[0][[2, 7, 30, 31], 0] == 0).all()
    d2r, idxr = wu.knn_ref(c, c, 3, self0=0)
    assert np.array_equal(whole[1], idxr)
    # a row with three centres at distance 0 takes the lower other index first
    c3 = c.copy()
    c3[20] = c3[2]
    _, i3 = widths.knn(c3, c3, 2, exclude_self=True)
    assert i3.cpu().numpy()[[2, 7, 20]].tolist() == [[7, 20], [2, 20], [2, 7]]
    # two calls over halves of the rows equal one call
    h = K // 2
    cd = torch.from_numpy(c).cuda()
    a = widths.knn(cd[:h], cd, 3, exclude_self=True, row0=0)
    b = widths.knn(cd[h:], cd, 3, exclude_self=True, row0=h)
    assert np.array_equal(np.vstack([a[0].cpu().numpy(), b[0].cpu().numpy()]), whole[0])
    assert np.array_equal(np.vstack([a[1].cpu().numpy(), b[1].cpu().numpy()]), whole[1])
    # self0 + n >= K excludes nothing: every centre finds itself at distance 0
    r = Knn(c, c, 2, self0=K)
    plain = Knn(c, c, 2)
    assert r.raw() == plain.raw() and (r.d2[:, 0] == 0).all()
    first = np.arange(K)
    first[[7, 31]] = (2, 30)                                           # of two centres at distance 0 the lower index comes first
    assert np.array_equal(r.idx[:, 0], first)
    # without exclude_self the wrapper excludes nothing either
    assert np.array_equal(widths.knn(c, c, 2)[1].cpu().numpy(), plain.idx)


def test_scaling_by_a_power_of_two_commutes(gpu):
    _, c = ku.uniform_case(8, 300, 7, seed=5)
    c = c.copy()
    c[17] = c[4]                                                       # one replaced width rides along
    a = widths.nearest_neighbour(c, p=3)
    b = widths.nearest_neighbour(4.0 * c, p=3)
    assert a.replaced == b.replaced == 0                               # a duplicate has other neighbours: its mean is positive
    assert (4.0 * a.sigma).cpu().numpy().tobytes() == b.sigma.cpu().numpy().tobytes()
    a1, b1 = widths.nearest_neighbour(c, p=1), widths.nearest_neighbour(4.0 * c, p=1)
    assert a1.replaced == b1.replaced == 2
    assert (4.0 * a1.sigma).cpu().numpy().tobytes() == b1.sigma.cpu().numpy().tobytes()


def _rel(sigma, ref):
    return float((np.abs(sigma.astype(np.float64) - ref) / ref).max())


def test_width_rules_meet_the_float64_statement(gpu):
    worst = [0.0, 0.0]
    for K, D, p in ((300, 7, 2), (65, 3, 3), (1025, 16, 8), (5, 8, 8)):
        x, c = ku.uniform_case(4000, K, D, seed=51 + D)
        tol = 2 * ku.gamma(D) + 2.0 ** -24
        d2, _ = widths.knn(c, c, p, exclude_self=True)                 # the kernel's own lists
        ref, rep = wu.nn_widths_ref(d2.cpu().numpy(), scale=1.5)
        w = widths.nearest_neighbour(c, p=p, scale=1.5)
        assert w.sigma.dtype == torch.float32 and tuple(w.sigma.shape) == (K,) and w.replaced == rep == 0
        worst[0] = max(worst[0], _rel(w.sigma.cpu().numpy(), ref) / tol)
        # against the reference's lists: the distances' own gamma / 2 on top
        ref64, _ = wu.nn_widths_ref(wu.knn_ref(c, c, p, self0=0)[0], scale=1.5)
        assert _rel(w.sigma.cpu().numpy(), ref64) <= tol
        lab, ad2 = _kmeans_assign(x, c)                                # the kernel's own labels
        ref, rep = wu.spread_widths_ref(ad2, lab, K, scale=0.5)
        s = widths.cluster_spread(x, c, scale=0.5)
        assert s.replaced == rep and tuple(s.sigma.shape) == (K,)
        worst[1] = max(worst[1], _rel(s.sigma.cpu().numpy(), ref) / tol)
        assert s.sigma.cpu().numpy().tobytes() == widths.cluster_spread(x, c, scale=0.5).sigma.cpu().numpy().tobytes()
    print(f"width rules: largest err/bound nearest_neighbour {worst[0]:.3f} cluster_spread {worst[1]:.3f}")
    assert max(worst) <= 1.0


def test_replacement_rule(gpu):
    c = wu.duplicate_case()
    w = widths.nearest_neighbour(c, p=1)                               # two duplicate pairs: four widths of 0
    ref, rep = wu.nn_widths_ref(widths.knn(c, c, 1, exclude_self=True)[0].cpu().numpy())
    assert w.replaced == rep == 4
    s = w.sigma.cpu().numpy()
    assert np.isfinite(s).all() and (s > 0).all() and _rel(s, ref) <= 2.0 ** -23
    assert len(set(s[[2, 7, 30, 31]].tolist())) == 1
    # rows: eight around every centre but 11 (one row) and 12 (none); the duplicates 7 and 31 lose every row to 2 and 30
    rng = np.random.default_rng(3)
    rows = [c[k] + rng.normal(scale=0.01, size=(8, 3)).astype(np.float32) for k in range(40) if k not in (11, 12)]
    x = np.vstack(rows + [c[11:12] + np.float32(0.01)])
    lab, d2 = _kmeans_assign(x, c)
    counts = np.bincount(lab, minlength=40)
    assert counts[11] == 1 and counts[12] == 0 and counts[7] == 0 and counts[31] == 0
    sp = widths.cluster_spread(x, c)
    ref, rep = wu.spread_widths_ref(d2, lab, 40)
    assert sp.replaced == rep == 4 and _rel(sp.sigma.cpu().numpy(), ref) <= 2.0 ** -23
    assert widths.cluster_spread(x, c, min_count=1).replaced == 3
    with pytest.raises(ValueError):
        widths.nearest_neighbour(c[:1])                                # K = 1: no other centre
    with pytest.raises(ValueError):
        widths.cluster_spread(x[:1], c[:1])


@functools.lru_cache(maxsize=None)
def _e2e(s):
    """The end-to-end problem on the device: (x, y, centres, net at log_sigs = 0, widths, search)."""
    x, y = wu.e2e_problem(s)
    res = kmeans.fit(x, k=64, max_iter=10, seed=0)
    net0 = WCRBFNet.from_config(dict(wu.e2e_cfg(), fixed_centers=True, fixed_width=True), centers=res.centers.cpu().numpy())
    w = widths.nearest_neighbour(res.centers, p=2)
    return x, y, res, net0, w, widths.select_scale(net0, w, x, y)


def _holdout_mse(net, x, y, fit=None):
    """(fit on the training rows unless given, its held-out MSE through rss_of)."""
    ho = np.arange(len(x)) % 5 == 0
    p = net.init()
    if fit is None:
        fit = linear_fit.NormalEquations(net).add(p, x[~ho], y[~ho]).solve(ridge=1e-8)
    rss = linear_fit.NormalEquations(net).add(p, x[ho], y[ho]).rss_of(fit)
    return fit, float(rss.sum().item()) / (ho.sum() * y.shape[1])


@pytest.mark.parametrize("s", (0.05, 20.0))
def test_end_to_end_widths_from_the_data_beat_unit_widths(gpu, s):
    x, y, res, net0, w, search = _e2e(s)
    assert w.replaced == 0 and search.scales == wu.SCALES
    held = search.holdout_mse
    _, unit = _holdout_mse(net0, x, y)                                 # the same net at log_sigs = 0, priced through the same rss_of
    print(f"s = {s}: held-out MSE per scale {['%.3e' % h for h in held]}, train {['%.3e' % h for h in search.train_mse]}, "
          f"at log_sigs = 0 {unit:.3e}, best scale {search.best_scale}")
    assert search.best_scale in (2.0, 4.0) and search.best == int(np.argmin(held))
    assert held[search.best] <= unit / 10
    assert held[search.best] <= held[0] / 4 and held[search.best] <= held[4] / 4
    # the forward kernel agrees with the price taken from the Gram matrix alone
    ho = np.arange(len(x)) % 5 == 0
    out = search.net.apply(search.params, x[ho]).astype(np.float64)
    mse = float(((out - y[ho].astype(np.float64)) ** 2).mean())
    print(f"s = {s}: held-out MSE through apply {mse:.6e}, from the Gram matrix {held[search.best]:.6e}")
    assert abs(mse - held[search.best]) <= 0.01 * held[search.best] + 1e-7
    assert search.fit.mse == pytest.approx(search.train_mse[search.best], rel=1e-12)
    assert np.array_equal(search.net.log_sigs.astype(np.float32), w.scaled(search.best_scale).log_sigs(net0))


def test_a_scale_without_a_positive_definite_system_gets_inf(gpu):
    x, y, res, net0, w, _ = _e2e(20.0)
    # at 10^6 times the rule every float32 hidden value is exactly 1: the columns equal the ones column, singular without a ridge
    search = widths.select_scale(net0, w, x, y, scales=(1.0, 1.0e6), ridge=0.0)
    assert search.holdout_mse[1] == float("inf") and search.train_mse[1] == float("inf") and search.best == 0
    with pytest.raises(ValueError):
        widths.select_scale(WCRBFNet.from_config(wu.e2e_cfg()), w, x, y)               # not a fixed-width net
    with pytest.raises(ValueError, match="must have shape"):                           # a wrong table is named, not priced at inf
        widths.select_scale(net0, w, x[:, :2], y)
    with pytest.raises(ValueError, match="must have shape"):
        widths.select_scale(net0, w, x, y[:, :1])


def test_rss_of(gpu):
    x, y, res, net0, w, search = _e2e(20.0)
    net = search.net
    ho = np.arange(len(x)) % 5 == 0
    p = net.init()
    own = linear_fit.NormalEquations(net).add(p, x[~ho], y[~ho])
    fit = own.solve(ridge=1e-8)
    assert torch.equal(own.rss_of(fit), fit.rss)                       # the accumulator the fit was solved on
    flat = own.solve(ridge=1e-8, fit_bias=False)
    assert torch.equal(own.rss_of(flat), flat.rss)
    other = linear_fit.NormalEquations(net).add(p, x[ho], y[ho])
    h = net.hidden(p, x[ho]).astype(np.float64)                        # the kernel's own hidden rows
    y64 = y[ho].astype(np.float64)
    for f in (fit, flat):
        want = ((h @ f.kernel.cpu().numpy() + f.bias.cpu().numpy() - y64) ** 2).sum(0)
        got = other.rss_of(f).cpu().numpy()
        assert (np.abs(got - want) <= 1e-9 * (y64 ** 2).sum(0)).all(), (got, want)
    with pytest.raises(ValueError):
        linear_fit.NormalEquations(net).rss_of(fit)                    # no rows


def test_log_sigs_as_a_constant_and_as_a_leaf(gpu):
    x, y, res, net0, w, search = _e2e(0.05)
    ls = w.scaled(2.0).log_sigs(net0)
    assert ls.shape == (1, 64) and ls.dtype == np.float32
    centers = res.as_centers(net0)
    frozen = WCRBFNet(**wu.e2e_cfg(), centers=centers, fixed_width=True, log_sigs=ls)
    lin = search.params["params"]["linear"]
    a = frozen.apply({"params": {"linear": lin}}, x[:300])
    free = WCRBFNet(**wu.e2e_cfg())
    tree = free.init()
    tree["params"]["rbf_list"]["centers"] = centers[None].copy()
    tree["params"]["rbf_list"]["log_sigs"] = ls
    tree["params"]["linear"] = lin
    b = free.apply(tree, x[:300])
    assert a.tobytes() == b.tobytes() and np.isfinite(a).all()
