"""OLS forward selection on the GPU (run on the MI355X box with ``-m gpu``): irbfn_ols_begin / irbfn_ols_steps through the C ABI
against the float64 statement of it (tests/_ols_util.py: ols_ref) on the kernel's own Gram matrix, then ``ols.select``,
``NormalEquations.subset`` and ``OLSResult.subnet``, and the pipeline pool -> widths -> selection -> fit end to end.

Every buffer is prefilled with a sentinel and carries guard elements behind it; the padding of every row (entries n .. npad - 1),
the rows past the pivots taken and the guards must come back untouched; the workspace is exactly irbfn_ols_workspace_bytes,
prefilled with 0x5A, with a guard pattern behind it.

Bounds.  Indices equal the statement's; every array within TOL (= 16 times the largest difference between the two float64
statements, tests/_ols_util.py) of its largest magnitude.  Index equality rests on the scores of the statement never coming
closer than GAP = 1000 TOL relative, which every test that compares indices asserts of its own design.

Largest err / (TOL max|array|) measured over the cases and the shape edges (printed by the tests): gain 4.5e-4 (M = 65), L 6.4e-3
and d 1.2e-3 (M = 1025), i.e. 1.7e-13 of the largest entry at worst.  Times: profiles/ols.txt."""
import functools

import numpy as np
import pytest
import torch

import _linear_fit_util as lu
import _ols_util as ou
import _widths_util as wu
from irbfn_amd import _lib, kmeans, linear_fit, ols, widths
from irbfn_amd.model import WCRBFNet, _ptr, _stream_ptr

pytestmark = pytest.mark.gpu
GUARD = 3
SENT, SENT_I = -5.0, -7


def device_gram(H, Y):
    """G = Z^T Z of Z = [H | 1 | Y] (float32 values) by irbfn_syrk_f64: the kernel's own Gram matrix, on the device."""
    Z = np.hstack([H, np.ones((len(H), 1)), Y]).astype(np.float32)
    return linear_fit.syrk(torch.from_numpy(Z).cuda())


class Run:
    """One selection through the C ABI on guarded, prefilled buffers: ``plan`` = the steps of each irbfn_ols_steps call."""

    def __init__(self, G, M, O, kmax, fit_bias=True, lam=None, tol=None, plan=None):
        lib = _lib.load()
        Gn = G.cpu().numpy()
        self.lam = ou.lam_of(Gn, M) if lam is None else lam
        self.tol = ou.default_tol(M, fit_bias) if tol is None else tol
        b = 1 if fit_bias else 0
        self.n, self.npad, self.rows = M + b, ou.npad(M), kmax + 1
        f = lambda size, v, dt: torch.full((size + GUARD,), v, dtype=dt, device="cuda")     # noqa: E731
        self.t_l, self.t_d = f(self.rows * self.npad, SENT, torch.float64), f(2 * self.npad, SENT, torch.float64)
        self.t_c, self.t_gain = f(self.npad * O, SENT, torch.float64), f(self.rows * O, SENT, torch.float64)
        self.t_sel, self.t_count = f(self.rows, SENT_I, torch.int32), f(1, SENT_I, torch.int32)
        need = lib.irbfn_ols_workspace_bytes(M, O, kmax)
        assert need > 0
        ws = torch.full((need + 8 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda")        # no reliance on a cleared workspace
        bufs = (_ptr(self.t_l), _ptr(self.t_d), _ptr(self.t_c), _ptr(self.t_sel), _ptr(self.t_gain), _ptr(self.t_count), _ptr(ws), need)
        st = lib.irbfn_ols_begin(_ptr(G), M, O, b, self.lam, self.tol, kmax, *bufs, _stream_ptr(torch))
        assert st == 0, st
        for steps in ([kmax + b] if plan is None else plan):
            st = lib.irbfn_ols_steps(_ptr(G), M, O, b, self.tol, kmax, *bufs, steps, _stream_ptr(torch))
            assert st == 0, st
        torch.cuda.synchronize()
        assert (ws[need:] == 0x5A).all()
        cut = lambda t, size: (t[:size].cpu().numpy(), t[size:].cpu().numpy())               # noqa: E731
        l, g1 = cut(self.t_l, self.rows * self.npad)
        d, g2 = cut(self.t_d, 2 * self.npad)
        c, g3 = cut(self.t_c, self.npad * O)
        gain, g4 = cut(self.t_gain, self.rows * O)
        sel, g5 = cut(self.t_sel, self.rows)
        count, g6 = cut(self.t_count, 1)
        assert all((g == SENT).all() for g in (g1, g2, g3, g4)) and (g5 == SENT_I).all() and (g6 == SENT_I).all()
        self.count = int(count[0])
        l, d, c = l.reshape(self.rows, self.npad), d.reshape(2, self.npad), c.reshape(self.npad, O)
        gain = gain.reshape(self.rows, O)
        # the padding and everything past the pivots taken is untouched
        assert (l[:, self.n:] == SENT).all() and (d[:, self.n:] == SENT).all() and (c[self.n:] == SENT).all()
        assert (l[self.count:] == SENT).all() and (gain[self.count:] == SENT).all() and (sel[self.count:] == SENT_I).all()
        self.L, self.d, self.d0, self.c = l[:self.count, :self.n], d[0, :self.n], d[1, :self.n], c[:self.n]
        self.gain, self.sel = gain[:self.count], sel[:self.count]

    def raw(self):
        """Every output as bytes, for bit-for-bit comparisons."""
        return tuple(t.cpu().numpy().tobytes() for t in (self.t_l, self.t_d, self.t_c, self.t_gain, self.t_sel, self.t_count))


def gap_holds(ref):
    """The statement's own scores never come closer than GAP: index equality may be asked of another order of the sums."""
    with np.errstate(invalid="ignore"):
        g = (ref["best"] - ref["second"]) / ref["best"]
    return bool((g[~np.isnan(g)] > ou.GAP).all())


def check(run, ref, worst=None):
    """Holds one run to the statement; returns the largest error over TOL times the array's largest magnitude."""
    assert run.count == ref["count"] and np.array_equal(run.sel, ref["sel"]), (run.sel, ref["sel"])
    pairs = {"gain": (run.gain, ref["gain"]), "L": (run.L, ref["L"]), "d": (np.stack([run.d, run.d0]), np.stack([ref["d"], ref["d0"]])),
             "c": (run.c, ref["c"])}
    out = {}
    for name, (a, b) in pairs.items():
        scale = np.abs(b).max() if name != "c" else np.abs(ref["d0"]).max() ** 0.5 * np.abs(ref["objective"][0]).max() ** 0.5
        out[name] = float(np.abs(a - b).max() / (ou.TOL * scale)) if b.size and scale > 0 else 0.0
    assert max(out.values()) <= 1.0, out
    if worst is not None:
        for k, v in out.items():
            worst[k] = max(worst.get(k, 0.0), v)
    return out


def check_select(G, M, O, k, fit_bias, ref):
    """``ols.select`` on the same matrix: indices, n_selected, gain and objective of the result."""
    res = ols.select(linear_fit.NormalEquations(lu.Shape(M, O), G=G), k, ridge=ou.RIDGE, fit_bias=fit_bias)
    b = 1 if fit_bias else 0
    assert res.n_selected == ref["count"] - b and res.indices.dtype == torch.int32 and res.indices.is_cuda
    assert np.array_equal(res.indices.cpu().numpy(), ref["sel"][b:])
    want_obj = ref["objective"][b:]
    assert tuple(res.gain.shape) == (res.n_selected, O) and tuple(res.objective.shape) == (res.n_selected + 1, O)
    assert ou.rel(res.gain.cpu().numpy(), ref["gain"][b:]) <= ou.TOL and ou.rel(res.objective.cpu().numpy(), want_obj) <= ou.TOL
    assert res.ridge_abs == pytest.approx(ou.lam_of(G.cpu().numpy(), M), rel=1e-14)
    return res


@pytest.mark.parametrize("fit_bias", (True, False))
@pytest.mark.parametrize("case", ou.CASES, ids=lambda c: "N%d-M%d-O%d-K%d" % c)
def test_cases_meet_the_float64_statement(gpu, case, fit_bias):
    N, M, O, K = case
    H, Y, _ = ou.case(N, M, O)
    G = device_gram(H, Y)
    ref = ou.ols_ref(G.cpu().numpy(), M, O, K, fit_bias=fit_bias)
    assert gap_holds(ref)
    out = check(Run(G, M, O, K, fit_bias), ref)
    check_select(G, M, O, K, fit_bias, ref)
    print(f"ols N={N} M={M} O={O} K={K} fit_bias={fit_bias}: largest err / (TOL max|array|) {out}")


@pytest.mark.parametrize("fit_bias", (True, False))
@pytest.mark.parametrize("M", ou.EDGE_M)
def test_shape_edges_meet_the_float64_statement(gpu, M, fit_bias):
    worst = {}
    for O in ou.EDGE_O:
        H, Y, _, _ = ou.design(ou.edge_rows(M), M, O)
        G = device_gram(H, Y)
        Gn = G.cpu().numpy()
        for kmax in [k for k in ou.EDGE_K if k <= M]:
            ref = ou.ols_ref(Gn, M, O, kmax, fit_bias=fit_bias)
            assert gap_holds(ref), (M, O, kmax)
            check(Run(G, M, O, kmax, fit_bias), ref, worst)
        if M >= 2:
            check_select(G, M, O, min(M, 33), fit_bias, ou.ols_ref(Gn, M, O, min(M, 33), fit_bias=fit_bias))
    print(f"ols edges M={M} fit_bias={fit_bias}: largest err / (TOL max|array|) {worst}")


@pytest.mark.parametrize("case", ou.CASES[:2], ids=lambda c: "N%d-M%d-O%d-K%d" % c)
def test_every_pick_has_the_largest_lstsq_gain_given_its_prefix(gpu, case):
    N, M, O, K = case
    H, Y, _ = ou.case(N, M, O)
    G = device_gram(H, Y)
    run = Run(G, M, O, K)
    lam = ou.lam_of(G.cpu().numpy(), M)
    assert run.count == K + 1 and run.sel[0] == M
    picks = run.sel[1:].tolist()
    for t, j in enumerate(picks):
        g, _ = ou.lstsq_gains(H, Y, lam, True, picks[:t])
        tot = np.where(np.isnan(g.sum(1)), -np.inf, g.sum(1))
        assert int(np.argmax(tot)) == j, (t, j, int(np.argmax(tot)))
        assert abs(run.gain[t + 1].sum() / tot[j] - 1) <= 1000 * ou.TOL          # and the gain is lstsq's, to the margin of the gap


@functools.lru_cache(maxsize=None)
def _degenerate():
    """40 candidates with two bit-for-bit duplicate pairs (wu.duplicate_case: 7 = 2, 31 = 30) and an all-zero column 13."""
    rng = np.random.default_rng(5)
    x = rng.uniform(-3, 3, (300, 3)).astype(np.float32)
    H = wu.hidden32(x, wu.duplicate_case(), np.full(40, 1.5))
    H[:, 13] = 0.0
    Y = (H[:, [2, 30, 20]] @ rng.normal(size=(3, 2)) + 0.1 * rng.normal(size=(300, 2))).astype(np.float32).astype(np.float64)
    return H, Y


def test_duplicates_and_a_zero_column_are_never_selected(gpu):
    H, Y = _degenerate()
    G = device_gram(H, Y)
    ne = linear_fit.NormalEquations(lu.Shape(40, 2), G=G)
    for fit_bias in (True, False):
        res = ols.select(ne, 40, ridge=0.0, fit_bias=fit_bias)                      # the whole pool is asked for
        idx = res.indices.cpu().numpy().tolist()
        assert res.n_selected == 37 == len(set(idx)), idx                           # one of each pair and the zero column are left
        assert 13 not in idx and len({2, 7} & set(idx)) == 1 and len({30, 31} & set(idx)) == 1
        assert tuple(res.objective.shape) == (38, 2) and bool((res.gain >= 0).all())
    some = ols.select(ne, 20, check_every=4, min_gain=0.0)                          # with host reads: the same pivots
    assert np.array_equal(some.indices.cpu().numpy(), ols.select(ne, 20).indices.cpu().numpy())
    early = ols.select(ne, 40, check_every=1, min_gain=1e-3)
    assert 1 <= early.n_selected < 37 and float(early.gain[-1].sum()) < 1e-3 * float(torch.diagonal(G)[41:].sum())
    assert early.n_selected == 1 or float(early.gain[-2].sum()) >= 1e-3 * float(torch.diagonal(G)[41:].sum())


def test_a_pool_of_rank_five_ends_after_five_pivots(gpu):
    """Integer columns of rank 5, no ridge, the caller's tol = 1e-9: five pivots, then every step is a no-op that writes nothing
    (Run holds everything past the count to its sentinels), however the steps are divided over the calls."""
    rng = np.random.default_rng(1)
    Hr = (rng.integers(-3, 4, size=(60, 5)) @ rng.integers(-2, 3, size=(5, 12))).astype(np.float64)
    Yr = rng.integers(-3, 4, size=(60, 2)).astype(np.float64)
    G = device_gram(Hr, Yr)
    assert np.array_equal(G.cpu().numpy(), lu.stacked_gram(Hr, Yr))                  # small integers: exact
    for fit_bias in (True, False):
        b = 1 if fit_bias else 0
        ref = ou.ols_ref(G.cpu().numpy(), 12, 2, 12, fit_bias=fit_bias, lam=0.0, tol=1e-9)
        run = Run(G, 12, 2, 12, fit_bias, lam=0.0, tol=1e-9)
        # no index equality here: with one dimension left every remaining column has the same score but for rounding
        picks = run.sel[b:].tolist()
        assert run.count == ref["count"] == 5 + b and np.linalg.matrix_rank(Hr[:, picks]) == 5 == len(set(picks))
        assert Run(G, 12, 2, 12, fit_bias, lam=0.0, tol=1e-9, plan=[3, 0, 4, 9, 1]).raw() == run.raw()
        res = ols.select(linear_fit.NormalEquations(lu.Shape(12, 2), G=G), 12, ridge=0.0, fit_bias=fit_bias, tol=1e-9)
        assert res.n_selected == 5 and tuple(res.gain.shape) == (5, 2) and tuple(res.objective.shape) == (6, 2)


def test_non_finite_entries_are_refused_with_their_count(gpu):
    H, Y, _ = ou.case(*ou.CASES[0][:3])
    G = device_gram(H, Y)
    G[3, 5] = G[5, 3] = float("nan")
    G[0, 0] = float("inf")
    with pytest.raises(ValueError, match="3 non-finite"):
        ols.select(linear_fit.NormalEquations(lu.Shape(40, 2), G=G), 4)
    with pytest.raises(ValueError, match="no rows"):
        ols.select(linear_fit.NormalEquations(lu.Shape(40, 2)), 4)
    with pytest.raises(ValueError):
        ols.select(linear_fit.NormalEquations(lu.Shape(40, 2), G=device_gram(H, Y)), 41)


def test_equal_scores_go_to_the_lower_index(gpu):
    H, Y = ou.integer_tie_design()
    G = device_gram(H, Y)
    assert np.array_equal(G.cpu().numpy(), lu.stacked_gram(H, Y))                    # exact
    for fit_bias in (True, False):
        ref = ou.ols_ref(G.cpu().numpy(), 6, 2, 6, fit_bias=fit_bias, lam=0.0)
        sel = ref["sel"].tolist()
        assert ref["best"][sel.index(1)] == ref["second"][sel.index(1)] and sel.index(1) < sel.index(4)      # a bit-equal tie, in the statement
        run = Run(G, 6, 2, 6, fit_bias, lam=0.0)
        assert np.array_equal(run.sel, ref["sel"])
        # the same design with the two columns exchanged: the lower index wins again, so the other column does
        P = [0, 4, 2, 3, 1, 5]
        swapped = Run(device_gram(H[:, P], Y), 6, 2, 6, fit_bias, lam=0.0)
        assert np.array_equal(swapped.sel, run.sel)


@pytest.mark.parametrize("shape", ((500, 65, 1, 33), (1225, 1025, 10, 65)), ids=lambda c: "N%d-M%d-O%d-K%d" % c)
def test_repeats_and_divided_steps_are_bit_identical(gpu, shape):
    N, M, O, K = shape
    H, Y, _, _ = ou.design(N, M, O)
    G = device_gram(H, Y)
    first = Run(G, M, O, K).raw()
    assert Run(G, M, O, K).raw() == first
    assert Run(G, M, O, K, plan=[1] * (K + 1)).raw() == first
    assert Run(G, M, O, K, plan=[7, K + 1 - 7]).raw() == first
    assert Run(G, M, O, K, plan=[K + 1, 5]).raw() == first                            # steps past kmax are no-ops
    a, b = (ols.select(linear_fit.NormalEquations(lu.Shape(M, O), G=G), K) for _ in range(2))
    assert torch.equal(a.indices, b.indices) and torch.equal(a.gain, b.gain) and torch.equal(a.objective, b.objective)


# ------------------------------------------------------------------ the Python surface
def _cfg(K, R=1, O=2):
    if R == 1:
        return wu.e2e_cfg(K=K, O=O)
    return dict(in_features=3, out_features=O, num_kernels=K, basis_func="gaussian", num_regions=4, lower_bounds=[[0.0, 2.0]] * 2,
                upper_bounds=[[2.0, 4.0]] * 2, dimension_ranges=[[0, 0], [0, 1], [1, 0], [1, 1]], activation_idx=[0, 1], delta=[5.0, 5.0])


@functools.lru_cache(maxsize=None)
def _pool(R=1, M=48):
    """x in [0, 4]^3 (1024 rows), y of wu.e2e_problem; a pool of M centres on rows of x (other rows per region), sigma ~ U(0.6, 1.2)."""
    x, y = wu.e2e_problem(4.0, seed=3, N=1024)
    rng = np.random.default_rng(11)
    centers = np.stack([x[rng.choice(len(x), M, replace=False)] for _ in range(R)])
    log_sigs = np.log(rng.uniform(0.6, 1.2, size=(R, M)))
    return x, y, centers, log_sigs


def test_subset_solve_is_fit_linear_on_the_hand_sliced_net(gpu):
    x, y, centers, log_sigs = _pool()
    net = WCRBFNet(**_cfg(48), centers=centers, fixed_width=True, log_sigs=log_sigs)
    ne = linear_fit.NormalEquations(net).add(net.init(), x, y)
    res = ols.select(ne, 16)
    idx = res.indices.cpu().numpy()
    assert res.n_selected == 16 and len(set(idx.tolist())) == 16
    yty = torch.diagonal(ne.G)[49:]
    for k in (1, 7, 16):
        hand = WCRBFNet(**_cfg(k), centers=centers[:, idx[:k]], fixed_width=True, log_sigs=log_sigs[:, idx[:k]])
        _, want = linear_fit.fit_linear(hand, hand.init(), x, y)
        sub = ne.subset(res.indices[:k], hand)
        got = sub.solve()
        scale = float(want.kernel.abs().max())
        assert float((got.kernel - want.kernel).abs().max()) <= 1e-9 * scale and float((got.bias - want.bias).abs().max()) <= 1e-9 * scale
        # the path's objective is the fit at the selection's own absolute ridge
        same = sub.solve(ridge=res.ridge_abs * k / float(torch.diagonal(sub.G)[:k].sum()))
        assert same.ridge_abs == pytest.approx(res.ridge_abs, rel=1e-12)
        obj = same.rss + same.ridge_abs * (same.kernel ** 2).sum(0)
        assert bool(((res.objective[k] - obj).abs() <= ou.TOL * yty).all()), (k, res.objective[k], obj)


@pytest.mark.parametrize("R", (1, 4))
def test_subnet_round_trips_frozen_and_free_trees(gpu, R):
    x, y, centers, log_sigs = _pool(R)
    frozen = WCRBFNet(**_cfg(48, R), centers=centers, fixed_width=True, log_sigs=log_sigs)
    free = WCRBFNet(**_cfg(48, R))
    tree = free.init()
    tree["params"]["rbf_list"]["centers"] = centers.astype(np.float32)
    tree["params"]["rbf_list"]["log_sigs"] = log_sigs.astype(np.float32)
    y64 = y.astype(np.float64)
    outs = []
    for net, p in ((frozen, frozen.init()), (free, tree)):
        net_k, p_k, fit, res = ols.fit_ols(net, p, x, y, 12)
        idx = res.indices.cpu().numpy()
        assert net_k.num_kernels == 12 == res.n_selected and net_k.num_regions == R and net_k.frozen == net.frozen
        if net is frozen:                                                # every region keeps the same kernel indices
            assert np.array_equal(net_k.centers, centers[:, idx]) and np.array_equal(net_k.log_sigs, log_sigs[:, idx])
            assert set(p_k["params"]) == {"linear"}
        else:
            assert np.array_equal(p_k["params"]["rbf_list"]["centers"], centers.astype(np.float32)[:, idx])
            assert np.array_equal(p_k["params"]["rbf_list"]["log_sigs"], log_sigs.astype(np.float32)[:, idx])
        assert np.array_equal(p_k["params"]["linear"]["kernel"], fit.kernel.cpu().numpy().astype(np.float32))
        # the sub-net's own hidden layer is the selected columns of the pool's, and reproduces the fit's rss
        assert np.abs(net_k.hidden(p_k, x[:200]) - net.hidden(p, x[:200])[:, idx]).max() <= 2e-6          # values of O(1), float32
        again = linear_fit.NormalEquations(net_k).add(p_k, x, y).rss_of(fit).cpu().numpy()
        assert (np.abs(again - fit.rss.cpu().numpy()) <= 1e-9 * (y64 ** 2).sum(0)).all(), (again, fit.rss)
        out = net_k.apply(p_k, x).astype(np.float64)
        assert (np.abs(((out - y64) ** 2).sum(0) - fit.rss.cpu().numpy()) <= 1e-3 * fit.rss.cpu().numpy() + 1e-6 * (y64 ** 2).sum(0)).all()
        outs.append((idx, out))
    assert np.array_equal(outs[0][0], outs[1][0]) and outs[0][1].tobytes() == outs[1][1].tobytes()


# ------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def _kmeans_best(s):
    """The best held-out MSE of select_scale over wu.SCALES on a 64-centre k-means net (the pipeline before this stage)."""
    x, y = wu.e2e_problem(s)
    res = kmeans.fit(x, k=64, max_iter=10, seed=0)
    net0 = WCRBFNet.from_config(dict(wu.e2e_cfg(), fixed_centers=True, fixed_width=True), centers=res.centers.cpu().numpy())
    search = widths.select_scale(net0, widths.nearest_neighbour(res.centers, p=2), x, y)
    return min(search.holdout_mse)


@pytest.mark.parametrize("s", (0.05, 20.0))
def test_end_to_end_selected_centres_beat_kmeans_centres(gpu, s):
    """64 of a 512-centre k-means pool, widths 4 x the pool's 2-nearest-neighbour rule, selected on the rows with index % 5 != 0 and
    priced on the rest.  Measured (s = 0.05 and s = 20 alike): held-out MSE 1.683e-4 on the device and in the float64 restatement on the
    device's own pool centres and widths (the same column at 64 of 64 steps), against 5.14e-4 for 64 k-means centres at their best
    scale: ratio 3.05 in both, so the divisor stays 1.5."""
    x, y = wu.e2e_problem(s)
    ho = np.arange(len(x)) % 5 == 0
    pool = kmeans.fit(x, k=512, max_iter=10, seed=0)
    w = widths.nearest_neighbour(pool.centers, p=2).scaled(4.0)
    cfg = wu.e2e_cfg(K=512)
    net = WCRBFNet(**cfg, centers=pool.centers.cpu().numpy()[None], fixed_width=True, log_sigs=w.log_sigs(WCRBFNet(**cfg)))
    p = net.init()
    ne = linear_fit.NormalEquations(net).add(p, x[~ho], y[~ho])
    res = ols.select(ne, 64)
    net64, p64, fit = res.subnet(net, p)
    assert res.n_selected == 64
    rss = linear_fit.NormalEquations(net64).add(p64, x[ho], y[ho]).rss_of(fit)
    held = float(rss.sum().item()) / (ho.sum() * y.shape[1])
    # the float64 restatement on the device's own pool centres and widths
    c, sigma = pool.centers.cpu().numpy(), w.sigma.cpu().numpy().astype(np.float64)
    H = wu.hidden32(x, c, sigma)
    y64 = y.astype(np.float64)
    ref = ou.ols_ref(lu.stacked_gram(H[~ho], y64[~ho]), 512, 2, 64)
    sel = ref["sel"][1:]
    sol = wu.solve_ref(H[~ho][:, sel], y64[~ho], 1e-8)
    want = float(((np.hstack([H[ho][:, sel], np.ones((ho.sum(), 1))]) @ sol - y64[ho]) ** 2).mean())
    base = _kmeans_best(s)
    same = int((res.indices.cpu().numpy() == sel).sum())
    print(f"s = {s}: held-out MSE of 64 selected centres {held:.4e} (float64 restatement {want:.4e}; {same} of 64 picks at the same step), "
          f"of 64 k-means centres at their best scale {base:.4e}: ratio {base / held:.2f} (restatement {base / want:.2f})")
    assert abs(held - want) <= 0.01 * want + 1e-7
    assert held <= base / 1.5
