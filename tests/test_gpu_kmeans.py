"""k-means on the GPU (run on the MI355X box with ``-m gpu``): irbfn_kmeans_step through the C ABI against the float64
statement of one Lloyd iteration (tests/_kmeans_util.py), then ``kmeans.fit`` / ``assign``, the labelled ``DeviceTable`` and
``train_epoch`` on a ``ClusterTrainState``.  Every output buffer is prefilled with NaN / a sentinel and carries guard elements
past N and past K * D that must come back untouched; the rows carry NaN guard rows past N that must not be read.

Bounds (derived in _kmeans_util): labels d2_ref[n, label] <= min_k d2_ref[n, k] (1 + 3 gamma), d2 within gamma relative,
gamma = (D + 2) 2^-23; new centres within 2^-23 max_n |x[n, d]| of the float64 mean over the kernel's own labels; counts
and moved exact; inertia within N 2^-53 relative of the float64 sum of the kernel's own d2; shift^2 within 2^-50 relative.

Largest err / bound over the 54 cases of test_step_meets_the_float64_statement (printed by the test): label 0.000 (every row got
its float64 nearest centre), d2 0.479, centre 0.347; the million-row cluster: centre 0.133 (profiles/kmeans.txt has the times)."""
import functools

import numpy as np
import pytest
import torch

import _kmeans_util as ku
from _cluster_util import cluster_case
from irbfn_amd import _lib, configs, kmeans, tables, train
from irbfn_amd.model import ClusterWCRBFNet, _ptr, _stream_ptr

pytestmark = pytest.mark.gpu
BATCHES = (1, 63, 64, 65, 255, 256, 257, 1000)      # around a wave and a block, then several blocks with a ragged last one
NMAX = max(BATCHES)
DIMS = (1, 2, 3, 7, 8, 16)
TILE = 256                                          # centres per LDS tile of the assignment kernel
KS = (1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 1025)
GRID_ROWS = 1024 * 256 * 2                          # rows of one full grid of the assignment kernel: 1024 blocks, two rows per lane
GUARD = 3
SENT_I, SENT_L = -7, -77


class Step:
    """One irbfn_kmeans_step call on guarded, prefilled buffers; the outputs as NumPy arrays."""

    def __init__(self, x, c, prev=None, new=True, counts=True, d2=True):
        lib = _lib.load()
        x, c = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(c, np.float32)
        N, D = x.shape
        K = c.shape[0]
        self.N, self.K, self.D = N, K, D
        xg = torch.from_numpy(np.vstack([x, np.full((GUARD, D), np.nan, np.float32)])).cuda()
        cg = torch.from_numpy(np.vstack([c, np.full((GUARD, D), np.nan, np.float32)])).cuda()
        lab = np.full(N + GUARD, SENT_I, np.int32)
        lab[:N] = -1 if prev is None else prev
        self.t_lab = torch.from_numpy(lab).cuda()
        self.t_d2 = torch.full((N + GUARD,), -5.0, dtype=torch.float32, device="cuda") if d2 else None
        self.t_new = torch.full((K * D + GUARD,), float("nan"), dtype=torch.float32, device="cuda") if new else None
        self.t_cnt = torch.full((K + GUARD,), SENT_L, dtype=torch.int64, device="cuda") if counts else None
        self.t_stats = torch.full((4 + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
        need = lib.irbfn_kmeans_workspace_bytes(N, K, D)
        assert need > 0
        ws = torch.full((need + 8 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda")     # the kernels must not rely on a cleared workspace
        opt = lambda t: _ptr(t) if t is not None else None
        st = lib.irbfn_kmeans_step(_ptr(xg), _ptr(cg), _ptr(self.t_lab), opt(self.t_d2), opt(self.t_new), opt(self.t_cnt),
                                   _ptr(self.t_stats), N, K, D, _ptr(ws), need, _stream_ptr(torch))
        assert st == 0, st
        torch.cuda.synchronize()
        assert (ws[need:] == 0x5A).all()
        assert (self.t_lab[N:] == SENT_I).all() and torch.isnan(self.t_stats[4:]).all()
        self.labels = self.t_lab[:N].cpu().numpy()
        self.stats = self.t_stats[:4].cpu().numpy()
        self.d2 = self.new = self.counts = None
        if d2:
            assert (self.t_d2[N:] == -5.0).all()
            self.d2 = self.t_d2[:N].cpu().numpy()
        if new:
            assert torch.isnan(self.t_new[K * D:]).all()
            self.new = self.t_new[:K * D].cpu().numpy().reshape(K, D)
        if counts:
            assert (self.t_cnt[K:] == SENT_L).all()
            self.counts = self.t_cnt[:K].cpu().numpy()

    def raw(self):
        """Every output as bytes, for bit-for-bit comparisons."""
        return tuple(t.cpu().numpy().tobytes() for t in (self.t_lab, self.t_d2, self.t_new, self.t_cnt, self.t_stats) if t is not None)


def check_step(x, c, s, prev=None, ref=None):
    """Holds the outputs of one step to the float64 statement; returns the largest (label, d2, centre) error over bound."""
    x64, c64 = np.asarray(x, np.float64), np.asarray(c, np.float64)
    N, D = x64.shape
    K = c64.shape[0]
    g = ku.gamma(D)
    d2r = ku.d2_ref(x, c) if ref is None else ref
    want = ku.labels_of(d2r)
    lab = s.labels
    none = want < 0
    assert np.array_equal(lab < 0, none) and (lab[none] == -1).all() and (lab < K).all()
    ok = ~none
    idx = np.flatnonzero(ok)
    chosen = d2r[idx, lab[idx]]
    best = d2r[idx, want[idx]]
    assert np.isfinite(chosen).all()                                   # a non-finite centre is never chosen
    assert (chosen <= best * (1 + 3 * g)).all()                        # every row, none left out
    pos = best > 0
    worst = [float((chosen[pos] / best[pos] - 1).max() / (3 * g)) if pos.any() else 0.0, 0.0, 0.0]
    if s.d2 is not None:
        assert np.isnan(s.d2[none]).all()
        err = np.abs(s.d2[idx].astype(np.float64) - chosen)
        assert (err <= g * chosen).all()
        nzc = chosen > 0
        worst[1] = float((err[nzc] / (g * chosen[nzc])).max()) if nzc.any() else 0.0
    prev = np.full(N, -1, np.int32) if prev is None else np.asarray(prev)
    assert s.stats[0] == ok.sum()
    assert s.stats[2] == (prev[ok] != lab[ok]).sum()                   # moved: exact
    if s.d2 is not None:
        tot = float(s.d2[idx].astype(np.float64).sum())
        assert abs(s.stats[1] - tot) <= N * 2.0 ** -53 * tot           # inertia over the kernel's own d2
    mean, counts = ku.update_of(x, c, lab)                             # over the kernel's own labels
    if s.counts is not None:
        assert np.array_equal(s.counts, counts) and s.counts.sum() == ok.sum()
    if s.new is not None:
        empty = counts == 0
        assert s.new[empty].tobytes() == np.asarray(c, np.float32)[empty].tobytes()      # bit for bit, NaN centres included
        fin = np.isfinite(x64).all(axis=1)                             # max_n |x[n, d]| runs over the rows without a non-finite component
        colmax = np.abs(x64[fin]).max(axis=0) if fin.any() else np.zeros(D)
        err = np.abs(s.new[~empty].astype(np.float64) - mean[~empty])
        assert (err <= 2.0 ** -23 * colmax).all()
        if err.size and (colmax > 0).all():
            worst[2] = float((err / (2.0 ** -23 * colmax)).max())
        sh = ku.shift2_exact(s.new, np.asarray(c, np.float32), counts)
        assert abs(s.stats[3] - sh) <= 2.0 ** -50 * sh
    else:
        assert s.stats[3] == 0.0
    return worst


@functools.lru_cache(maxsize=None)
def _uniform(D):
    """NMAX rows and max(KS) centres of dimension D with their float64 distances, computed once, read-only."""
    x, c = ku.uniform_case(NMAX, max(KS), D, seed=100 + D)
    ref = ku.d2_ref(x, c)
    for a in (x, c, ref):
        a.setflags(write=False)
    return x, c, ref


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("D", DIMS)
def test_step_meets_the_float64_statement(gpu, D, K):
    """Every batch size against K centres (K > N gives empty clusters); a second call on unchanged centres moves nothing."""
    x, c, ref = _uniform(D)
    worst = np.zeros(3)
    for N in BATCHES:
        s = Step(x[:N], c[:K])
        worst = np.maximum(worst, check_step(x[:N], c[:K], s, ref=ref[:N, :K]))
        if N in (65, 1000):
            s2 = Step(x[:N], c[:K], prev=s.labels)
            assert s2.stats[2] == 0 and np.array_equal(s2.labels, s.labels)
            assert s2.raw()[1:4] == s.raw()[1:4]
    print(f"kmeans step D={D} K={K}: largest err/bound label {worst[0]:.3f} d2 {worst[1]:.3f} centre {worst[2]:.3f}")


def test_grid_stride_runs_twice(gpu):
    N = GRID_ROWS + 5
    x, c = ku.uniform_case(N, 5, 3, seed=11)
    s = Step(x, c)
    check_step(x, c, s)
    assert s.stats[0] == N and s.labels[-5:].min() >= 0


@pytest.mark.parametrize("case", ["integer", "ties"])
def test_exact_cases_equal_first_minimum_argmin(gpu, case):
    x, c = ku.integer_case() if case == "integer" else ku.tie_case()
    c = c.copy()
    c[-1] = c[3]                                                       # a centre duplicated bit for bit: the lower index wins
    d2r = ku.d2_ref(x, c)
    s = Step(x, c)
    assert np.array_equal(s.labels, d2r.argmin(axis=1))
    assert (s.labels != len(c) - 1).all() and (s.labels == 3).any()
    assert np.array_equal(s.d2.astype(np.float64), d2r.min(axis=1))    # every operation of the chain is exact here
    check_step(x, c, s, ref=d2r)
    if case == "ties":
        assert ((d2r == d2r.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum() > 300


def test_million_row_cluster_keeps_its_mean(gpu):
    """10^6 rows near 1000 +- 1 in one cluster: float32 partial sums would lose the mean (2^-23 * 1001 = 1.2e-4 is the bound)."""
    rng = np.random.default_rng(21)
    x = (1000.0 + rng.uniform(-1, 1, (1_000_000, 2))).astype(np.float32)
    x[:100] -= 2000.0                                                  # a few rows for the second cluster
    c = np.array([[1000, 1000], [-1000, -1000], [0, 5000]], np.float32)
    s = Step(x, c)
    assert s.counts.tolist() == [999_900, 100, 0]
    w = check_step(x, c, s)
    print(f"million-row cluster: centre err/bound {w[2]:.4f}")


def test_non_finite_rows_and_centres(gpu):
    x, c = ku.uniform_case(700, 9, 3, seed=31)
    x, c = x.copy(), c.copy()
    x[5, 1] = np.nan
    x[64] = np.inf
    x[300, 0] = -np.inf
    x[699, 2] = np.nan
    x[400] = 3.0e38                                                    # finite, but every float32 d2 overflows
    c[2, 1] = np.nan
    c[7] = np.inf
    s = Step(x, c, prev=np.zeros(700, np.int32))
    bad = [5, 64, 300, 400, 699]
    assert (s.labels[bad] == -1).all() and np.isnan(s.d2[bad]).all()
    assert s.stats[0] == 695 and s.counts.sum() == 695
    assert not np.isin(s.labels, (2, 7)).any() and s.counts[2] == 0 and s.counts[7] == 0
    assert np.isfinite(s.new[[0, 1, 3, 4, 5, 6, 8]]).all()
    ref = ku.d2_ref(x, c)
    ref[400] = np.inf                                                  # the float64 statement of "no finite float32 distance"
    check_step(x, c, s, prev=np.zeros(700, np.int32), ref=ref)
    # all rows non-finite: nothing is counted anywhere, every centre stays
    xn = np.full((70, 3), np.nan, np.float32)
    sn = Step(xn, c)
    assert (sn.labels == -1).all() and sn.stats.tolist() == [0.0, 0.0, 0.0, 0.0] and (sn.counts == 0).all()
    assert sn.new.tobytes() == c.tobytes()


@pytest.mark.parametrize("K,D", [(65, 8), (1025, 3)])
def test_two_runs_are_bit_identical(gpu, K, D):
    x, c = ku.uniform_case(40_000, K, D, seed=41)
    a, b = Step(x, c), Step(x, c)
    assert a.raw() == b.raw()


def test_assign_only(gpu):
    x, c, ref = _uniform(8)
    for N, K in ((1000, 65), (257, 1025)):
        full = Step(x[:N], c[:K])
        s = Step(x[:N], c[:K], new=False)                              # counts and statistics without new centres
        check_step(x[:N], c[:K], s, ref=ref[:N, :K])
        assert np.array_equal(s.counts, full.counts) and s.raw()[:2] == full.raw()[:2]
        assert s.stats[:3].tolist() == full.stats[:3].tolist() and s.stats[3] == 0.0
        bare = Step(x[:N], c[:K], new=False, counts=False, d2=False)
        assert np.array_equal(bare.labels, full.labels) and bare.stats.tolist() == s.stats.tolist()
        lab, d2 = kmeans.assign(x[:N], c[:K])
        assert lab.dtype == torch.int32 and d2.dtype == torch.float32
        assert np.array_equal(lab.cpu().numpy(), full.labels) and d2.cpu().numpy().tobytes() == full.d2.tobytes()


def test_fit_on_the_blobs(gpu):
    x, ids, init = ku.blobs()
    res = kmeans.fit(x, 5, max_iter=6, init=init)
    assert res.n_iter == 6 and tuple(res.history.shape) == (6, 4)
    assert np.array_equal(res.labels.cpu().numpy(), ids)
    c = init.astype(np.float64)
    for _ in range(6):
        c = ku.lloyd_step(x, c)["centers"].astype(np.float32).astype(np.float64)
    colmax = np.abs(x.astype(np.float64)).max(axis=0)
    assert (np.abs(res.centers.cpu().numpy() - c) <= 2.0 ** -23 * colmax).all()
    assert res.counts.cpu().numpy().tolist() == [400] * 5
    h = res.history.cpu().numpy()
    assert (h[:, 0] == 2000).all() and h[0, 2] == 2000 and (h[1:, 2] == 0).all()
    assert (h[1:, 1] <= h[:-1, 1] * (1 + ku.gamma(2))).all()           # the inertia does not increase, up to gamma
    assert res.inertia == h[-1, 1]
    early = kmeans.fit(x, 5, max_iter=6, init=init, check_every=1)
    assert early.n_iter == 2 and early.history[-1, 2].item() == 0      # the second iteration moved no row
    assert early.centers.cpu().numpy().tobytes() == res.centers.cpu().numpy().tobytes()
    assert np.array_equal(early.labels.cpu().numpy(), ids) and early.counts.cpu().numpy().tolist() == [400] * 5

    class Net:
        num_kernels, in_features = 5, 2
    assert res.as_centers(Net()).tobytes() == res.centers.cpu().numpy().tobytes()
    Net.in_features = 3
    with pytest.raises(ValueError):
        res.as_centers(Net())


@pytest.mark.parametrize("init", ["kmeans++", "random"])
def test_initialisations(gpu, init):
    rng = np.random.default_rng(51)
    x = rng.normal(size=(3000, 4)).astype(np.float32)
    x[::7, 2] = np.nan                                                 # every seventh row is not finite
    x[5::11] = np.inf
    rows = {r.tobytes() for r in x[np.isfinite(x).all(axis=1)]}
    a = kmeans.fit(x, 40, max_iter=0, init=init, seed=3)
    b = kmeans.fit(x, 40, max_iter=0, init=init, seed=3)
    c = kmeans.fit(x, 40, max_iter=0, init=init, seed=4)
    ca = a.centers.cpu().numpy()
    assert a.n_iter == 0 and ca.shape == (40, 4) and np.isfinite(ca).all()
    assert all(r.tobytes() in rows for r in ca) and len({r.tobytes() for r in ca}) == 40      # distinct finite rows of x
    assert ca.tobytes() == b.centers.cpu().numpy().tobytes()           # repeatable for a seed
    assert ca.tobytes() != c.centers.cpu().numpy().tobytes()
    with pytest.raises(ValueError):
        kmeans.fit(x[:14], 13, init=init)                              # fewer finite rows than centres


def test_kmeanspp_takes_no_duplicate_while_a_distant_row_remains(gpu):
    """Six distinct points, each repeated 50 times, and NaN rows: six centres must be the six points whatever the seed."""
    pts = np.array([[0, 0], [1, 0], [0, 1], [5, 5], [-3, 2], [2, -4]], np.float32)
    x = np.vstack([np.repeat(pts, 50, axis=0), np.full((20, 2), np.nan, np.float32)])
    x = x[np.random.default_rng(0).permutation(len(x))]
    for seed in range(5):
        c = kmeans.fit(x, 6, max_iter=0, init="kmeans++", seed=seed).centers.cpu().numpy()
        assert sorted(map(tuple, c.tolist())) == sorted(map(tuple, pts.tolist()))
    # more centres than distinct points: the rest repeat a finite row, never a NaN one
    c = kmeans.fit(x, 9, max_iter=0, init="kmeans++", seed=1).centers.cpu().numpy()
    assert np.isfinite(c).all() and {tuple(r) for r in c.tolist()} == {tuple(r) for r in pts.tolist()}


def test_labelled_device_table(gpu):
    rng = np.random.default_rng(61)
    xin, yout = rng.normal(size=(40, 8)).astype(np.float32), rng.normal(size=(40, 10)).astype(np.float32)
    xin[:, 0] = np.arange(40)                                          # the row number rides along
    lab = rng.integers(-1, 4, 40).astype(np.int32)
    lab[:3] = (-1, 0, 3)
    t = tables.DeviceTable(xin, yout, seed=1, labels=torch.from_numpy(lab).cuda(), num_classes=4)
    seen = 0
    for bx, by, ids in t.epoch(16):
        assert tuple(ids.shape) == (16, 4) and ids.dtype == torch.float32 and ids.is_contiguous()
        rows = bx[:, 0].cpu().numpy().astype(int)
        want = np.zeros((16, 4), np.float32)
        for i, r in enumerate(rows):
            if lab[r] >= 0:
                want[i, lab[r]] = 1.0
        assert np.array_equal(ids.cpu().numpy(), want)
        assert np.array_equal(by.cpu().numpy(), yout[rows])
        seen += 1
    assert seen == 2
    plain = tables.DeviceTable(xin, yout, seed=1)
    batches = list(plain.epoch(16))
    assert len(batches) == 2 and all(len(b) == 2 for b in batches)
    same = list(tables.DeviceTable(xin, yout, seed=1, labels=lab, num_classes=4).epoch(16))
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(batches, same))    # the same permutation stream
    for bad in (dict(labels=lab), dict(labels=lab[:5], num_classes=4), dict(labels=lab + 3, num_classes=4),
                dict(labels=lab.astype(np.float32), num_classes=4)):
        with pytest.raises(ValueError):
            tables.DeviceTable(xin, yout, **bad)


def test_train_epoch_with_a_cluster_state(gpu):
    R, K, B, T = 4, 3, 16, 5
    rng, cfg, params, xin = cluster_case(71, R=R, K=K, O=2 * T, B=2 * B)
    xin[:, 7] = rng.normal(size=2 * B).astype(np.float32) * 0.05       # a Frenet state the low-speed model integrates
    xin[:, 0] = rng.normal(size=2 * B).astype(np.float32) * 0.2
    xin[:, 2] = rng.uniform(1.0, 6.0, size=2 * B).astype(np.float32)
    yout = np.hstack([rng.normal(size=(2 * B, T)) * 2, rng.normal(size=(2 * B, T)) * 0.5]).astype(np.float32)
    lab = rng.integers(-1, R, 2 * B).astype(np.int32)
    net = ClusterWCRBFNet(**cfg)
    dp = configs.DYN_PARAMS

    def table():
        return tables.DeviceTable(xin, yout, seed=5, labels=lab, num_classes=R)
    state = train.ClusterTrainState.create(net, params)
    state, losses = train.train_epoch(state, table(), B, dyn_params=dp)
    assert tuple(losses.shape) == (2,) and torch.isfinite(losses).all()
    hand = train.ClusterTrainState.create(ClusterWCRBFNet(**cfg), params)
    by_hand = []
    for bx, by, ids in table().epoch(B):
        hand, loss = train.train_step_fullint_withcluster(hand, bx, by, ids, dp)
        by_hand.append(loss)
    assert torch.cat(by_hand).cpu().numpy().tobytes() == losses.cpu().numpy().tobytes()
    assert torch.equal(hand.flat, state.flat)
    with pytest.raises(ValueError):
        train.train_epoch(state, tables.DeviceTable(xin, yout), B, dyn_params=dp)        # unlabelled table
    with pytest.raises(ValueError):
        train.train_epoch(state, table(), B)                                             # no dyn_params
