"""Table evaluation on the GPU (run on the MI355X box with ``-m gpu``): the per-row roll-out error metrics of
irbfn_eval_rollout_errors against their float64 statement, its statistics against NumPy over the kernel's own per-row output,
accumulation across calls, determinism, non-finite rows, ties of the maximum, ``evaluate_table`` on the three net classes and
the merge of two ranks.  Output buffers are prefilled with NaN / -7 and carry guard rows; inputs carry NaN guard rows past B.

Largest err / bound over all cases of test_per_row_metrics_meet_the_float64_statement, per mode (printed by the test):
ST_SELECT 0.250 (state components and position) / 0.103 (controls), ST_KS 0.118 / 0.165, FULLINT 0.243 / 0.058,
FRENET_LS 0.064 / 0.140 (profiles/evaluate.txt)."""
import ctypes as C
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _evaluate_util as eu
from _evaluate_util import FRENET, FULLINT, KS, MODES, NUM_BINS, NUM_METRICS, SELECT
from _rollout_util import frenet_inputs, frenet_inputs_long, st_inputs
from irbfn_amd import _lib, configs, evaluate
from irbfn_amd import dynamics as dyn
from irbfn_amd.model import ClusterWCRBFNet, DeeperWCRBFNet, WCRBFNet, _stream_ptr

pytestmark = pytest.mark.gpu
DP = np.array(configs.DYN_PARAMS)
BATCHES = (1, 63, 64, 65, 255, 256, 257, 1000)     # around a wave and a block of 256, then several blocks with a ragged last one
NMAX = max(BATCHES)
S0 = {SELECT: 7, KS: 7, FULLINT: 1, FRENET: 8}
GUARD = 3
WORST = {}                                          # (mode, "state" / "controls") -> largest err / bound seen


def _params(mode):
    return None if mode == FULLINT else DP


def _rows(mode, B, T, seed, fast=True):
    """(state0 [B, S0], y [B, 2T], y_pred [B, 2T]) float32: seeded rows of a mode, y_pred = y + noise of a tenth of each control
    stream's rms."""
    rng = np.random.default_rng(seed + 1000)
    if mode in (SELECT, KS):
        x = st_inputs(B, T, seed, fast)
    elif mode == FULLINT:
        x = np.hstack([rng.uniform(-1, 8, (B, 1)), rng.normal(size=(B, T)) * 5, rng.normal(size=(B, T)) * 2])
    elif T <= 10:
        x = frenet_inputs(B, T, np.random.default_rng(seed))
    else:
        x = frenet_inputs_long(B, T, seed, DP)
    s0, y = x[:, :S0[mode]], x[:, S0[mode]:]
    rms = np.sqrt((y.reshape(B, 2, T) ** 2).mean(axis=(0, 2)))
    y_pred = y + rng.normal(size=(B, 2, T)).reshape(B, 2 * T) * np.repeat(0.1 * rms, T)
    return s0.astype(np.float32), y.astype(np.float32), y_pred.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(mode, T, fast=True):
    """NMAX rows of a mode with their float64 metrics and bounds, computed once and shared (read-only) by the batch sizes."""
    s0, y, yp = _rows(mode, NMAX, T, seed=17 * T + mode, fast=fast)
    err, bound = eu.metrics64(mode, s0, yp, y, DP)
    for a in (s0, y, yp, err, bound):
        a.setflags(write=False)
    return s0, y, yp, err, bound


def _dev(a, guard=GUARD):
    """Device copy of the rows `a` followed by `guard` rows of NaN that the kernel must not read."""
    a = np.ascontiguousarray(a, np.float32)
    return torch.from_numpy(np.vstack([a, np.full((guard, a.shape[1]), np.nan, np.float32)])).cuda()


class Out:
    """Output buffers of one evaluation, prefilled with NaN / -7, with a guard row each."""

    def __init__(self, mode, B, per_row=True):
        self.mode, self.M, self.B = mode, NUM_METRICS[mode], B
        M = self.M
        self.err = torch.full((B + GUARD, M), float("nan"), dtype=torch.float32, device="cuda") if per_row else None
        self.stats = torch.full((M + 1, 4), float("nan"), dtype=torch.float64, device="cuda")
        self.argmax = torch.full((M + 1,), -7, dtype=torch.int64, device="cuda")
        self.hist = torch.full((M + 1, NUM_BINS), -7, dtype=torch.int64, device="cuda")
        nb = _lib.load().irbfn_eval_workspace_bytes(mode)
        self.ws = torch.full((nb // 8 + 1,), float("nan"), dtype=torch.float64, device="cuda")

    def call(self, s0, yp, y, B, T, row0=0, accumulate=0):
        lib = _lib.load()
        keep, pp = dyn._dyn(_params(self.mode))
        p = lambda t: C.c_void_p(t.data_ptr() if t is not None else None)
        st = lib.irbfn_eval_rollout_errors(self.mode, p(s0), p(yp), p(y), pp, B, T, row0, accumulate, p(self.err), p(self.stats),
                                           p(self.argmax), p(self.hist), p(self.ws), (self.ws.numel() - 1) * 8, _stream_ptr(torch))
        _lib.check(st, "irbfn_eval_rollout_errors")
        return self

    def host(self):
        """(err [B, M] or None, stats [M, 4], argmax [M], hist [M, 512]) as NumPy after the guards were checked."""
        torch.cuda.synchronize()
        M, B = self.M, self.B
        assert torch.isnan(self.stats[M]).all() and (self.argmax[M] == -7) and (self.hist[M] == -7).all(), "store past the M metrics"
        assert torch.isnan(self.ws[-1]), "store past the workspace"
        err = None
        if self.err is not None:
            assert torch.isnan(self.err[B:]).all(), "store past row B"
            err = self.err[:B].cpu().numpy()
        return err, self.stats[:M].cpu().numpy(), self.argmax[:M].cpu().numpy(), self.hist[:M].cpu().numpy()


def _evaluate(mode, s0, y, yp, B, T, row0=0):
    out = Out(mode, B).call(_dev(s0[:B]), _dev(yp[:B]), _dev(y[:B]), B, T, row0)
    return out.host()


def _assert_stats_match(err, stats, argmax, hist, rows, row0=0):
    """The kernel's statistics against NumPy over a per-row table: n, max, argmax and every bin exactly, the two sums within
    rows * 2^-52 * sum |terms| of math.fsum."""
    rs, ra, rh, terms = eu.table_stats(err, row0)
    assert np.array_equal(stats[:, 0], rs[:, 0]), (stats[:, 0], rs[:, 0])
    assert np.array_equal(stats[:, 3], rs[:, 3])
    assert np.array_equal(argmax, ra), (argmax, ra)
    assert np.array_equal(hist, rh)
    assert (hist.sum(axis=1) == stats[:, 0]).all()
    for j in (1, 2):
        assert (np.abs(stats[:, j] - rs[:, j]) <= eu.sum_bound(rows, terms[:, j - 1])).all(), (j, stats[:, j], rs[:, j])


CASES = ([(m, T, f) for m in (SELECT, KS) for T in (1, 5, 16) for f in (True, False)]
         + [(FULLINT, T, True) for T in (1, 5, 16, 64)] + [(FRENET, T, True) for T in (1, 5, 16)])


@pytest.mark.parametrize("mode,T,fast", CASES)
def test_per_row_metrics_meet_the_float64_statement(mode, T, fast):
    s0, y, yp, ref, bound = _case(mode, T, fast)
    S = eu.STATE_DIM[mode]
    for B in BATCHES:
        err, stats, argmax, hist = _evaluate(mode, s0, y, yp, B, T)
        assert np.isfinite(err).all()
        ratio = np.abs(err.astype(np.float64) - ref[:B]) / bound[:B]
        for key, r in (("state", ratio[:, :S + 1].max()), ("controls", ratio[:, S + 1].max())):
            WORST[(mode, key)] = max(WORST.get((mode, key), 0.0), float(r))
        print(f"evaluate mode={mode} T={T} fast={fast} B={B}: largest err/bound state+position {ratio[:, :S + 1].max():.3f} "
              f"controls {ratio[:, S + 1].max():.3f}; per mode so far {WORST[(mode, 'state')]:.3f} / {WORST[(mode, 'controls')]:.3f}")
        bad = ratio > 1.0
        assert not bad.any(), (B, int(bad.sum()), np.argwhere(bad)[:4].tolist(), float(ratio.max()))
        _assert_stats_match(err, stats, argmax, hist, B)


@pytest.mark.parametrize("mode", MODES)
def test_statistics_match_numpy_over_the_kernels_own_rows(mode):
    """Rows drawn wide enough that some roll-outs differ a lot: the statistics are checked against the kernel's own per-row
    output, whatever the values; row0 offsets argmax."""
    T = 5
    s0, y, yp = _rows(mode, NMAX, T, seed=5 + mode)
    yp = (yp + np.random.default_rng(mode).normal(size=yp.shape) * 3).astype(np.float32)
    for B in BATCHES:
        err, stats, argmax, hist = _evaluate(mode, s0, y, yp, B, T, row0=10 ** 10)
        _assert_stats_match(err, stats, argmax, hist, B, row0=10 ** 10)
        assert (argmax >= 10 ** 10).all()


def test_statistics_past_the_grid_stride():
    """262 401 rows: 1024 blocks of 256 cover 262 144, the rest is a second pass of the first blocks' threads."""
    B, T = 262401, 5
    s0, y, yp = _rows(FULLINT, B, T, seed=3)
    err, stats, argmax, hist = _evaluate(FULLINT, s0, y, yp, B, T)
    assert np.isfinite(err).all() and (stats[:, 0] == B).all()
    _assert_stats_match(err, stats, argmax, hist, B)
    # the rows of the second pass are the same function of their inputs as those of the first
    tail, _, _, _ = _evaluate(FULLINT, s0[262144:], y[262144:], yp[262144:], B - 262144, T)
    assert np.array_equal(tail, err[262144:])


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype.itemsize == 8 else np.int32)


def test_accumulation_reset_and_determinism():
    T, N = 5, 1557
    s0, y, yp = _rows(SELECT, N, T, seed=41)
    whole = _evaluate(SELECT, s0, y, yp, N, T)
    again = _evaluate(SELECT, s0, y, yp, N, T)
    for a, b in zip(whole, again):
        assert np.array_equal(_bits(a), _bits(b)), "two identical runs differ"
    out = Out(SELECT, N, per_row=False)
    for i, (lo, n) in enumerate(((0, 1000), (1000, 257), (1257, 300))):
        out.call(_dev(s0[lo:lo + n]), _dev(yp[lo:lo + n]), _dev(y[lo:lo + n]), n, T, row0=lo, accumulate=int(i > 0))
    _, stats, argmax, hist = out.host()
    err, wstats, wargmax, whist = whole
    assert np.array_equal(stats[:, 0], wstats[:, 0]) and np.array_equal(stats[:, 3], wstats[:, 3])
    assert np.array_equal(argmax, wargmax) and np.array_equal(hist, whist)
    _assert_stats_match(err, stats, argmax, hist, N)
    # an empty batch that accumulates changes nothing
    before = [t.clone() for t in (out.stats, out.argmax, out.hist)]
    out.call(None, None, None, 0, T, accumulate=1)
    torch.cuda.synchronize()
    for a, b in zip(before, (out.stats, out.argmax, out.hist)):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    # accumulate = 0 afterwards starts again: the same buffers now hold the statistics of the 257 rows alone
    out.call(_dev(s0[1000:1257]), _dev(yp[1000:1257]), _dev(y[1000:1257]), 257, T, row0=1000, accumulate=0)
    _, stats, argmax, hist = out.host()
    _assert_stats_match(err[1000:1257], stats, argmax, hist, 257, row0=1000)
    # and an empty batch under accumulate = 0 leaves the empty statistics
    out.call(None, None, None, 0, T, accumulate=0)
    _, stats, argmax, hist = out.host()
    M = NUM_METRICS[SELECT]
    assert np.array_equal(stats, np.tile([0.0, 0.0, 0.0, -np.inf], (M, 1))) and (argmax == -1).all() and (hist == 0).all()


def test_non_finite_rows_are_counted_out():
    B, T = 300, 5
    s0, y, yp = _rows(FULLINT, B, T, seed=9)
    clean, _, _, _ = _evaluate(FULLINT, s0, y, yp, B, T)
    bad = yp.copy()
    bad[10, 2] = np.nan                   # an acceleration: reaches v, then x, y and the yaw, and the controls' mean
    bad[20, T + 1] = np.inf               # a steering rate: the steering angle is clipped, so it reaches the controls' mean only
    err, stats, argmax, hist = _evaluate(FULLINT, s0, y, bad, B, T)
    fin = np.isfinite(err)
    others = np.ones(B, bool)
    others[[10, 20]] = False
    assert np.array_equal(err[others], clean[others]) and fin[others].all()
    assert not fin[10, [0, 1, 3, 4, 5, 6]].any() and err[10, 2] == clean[10, 2]
    assert np.isinf(err[20, 6]) and fin[20, :6].all()
    assert np.array_equal(stats[:, 0], [B - 1, B - 1, B, B - 1, B - 1, B - 1, B - 2])
    _assert_stats_match(err, stats, argmax, hist, B)
    # the two rows move nothing of the controls' metric: it has the statistics of the clean rows without them
    masked = clean.copy()
    masked[[10, 20], 6] = np.nan
    rs, ra, rh, terms = eu.table_stats(masked)
    assert stats[6, 3] == rs[6, 3] and argmax[6] == ra[6] and np.array_equal(hist[6], rh[6])
    assert (np.abs(stats[6, 1:3] - rs[6, 1:3]) <= eu.sum_bound(B, terms[6])).all()
    # a batch of NaN predictions
    err, stats, argmax, hist = _evaluate(FULLINT, s0, y, np.full_like(yp, np.nan), B, T)
    assert np.isnan(err).all()
    assert (stats[:, :3] == 0).all() and np.isneginf(stats[:, 3]).all() and (argmax == -1).all() and (hist == 0).all()


def test_ties_report_the_lowest_row():
    B, T = 600, 5
    s0, y, yp = _rows(FRENET, B, T, seed=23)
    s0, y, yp = s0.copy(), y.copy(), yp.copy()
    src = 599                                        # rows 41, 300 and 599 (three blocks) share one input row with large errors
    yp[src] = y[src] + np.float32(1.5) * np.sign(y[src] + np.float32(0.01))
    for r in (300, 41):
        s0[r], y[r], yp[r] = s0[src], y[src], yp[src]
    err, stats, argmax, hist = _evaluate(FRENET, s0, y, yp, B, T, row0=7)
    assert np.array_equal(err[41], err[300]) and np.array_equal(err[41], err[599])
    M = NUM_METRICS[FRENET]
    assert err[41, M - 1] == err[:, M - 1].max() and argmax[M - 1] == 7 + 41
    # wherever exactly the three shared rows attain a metric's maximum, the lowest of them is reported (a metric that is 0 in
    # every row, such as the Frenet vy, is attained by row 0: _assert_stats_match covers it)
    top = [m for m in range(M) if np.flatnonzero(err[:, m] == err[:, m].max()).tolist() == [41, 300, 599]]
    print("ties: only the shared rows attain the maximum of metrics", top)
    assert M - 1 in top and len(top) >= 2 and all(argmax[m] == 7 + 41 for m in top)
    _assert_stats_match(err, stats, argmax, hist, B, row0=7)


# ------------------------------------------------------------------ evaluate_table
_card = eu.net_card


def _net_case(cls, kind, N=1000, T=5):
    """(net, params, x [N, D], y [N, 2T], dyn_params): a synthetic net of `cls` at the size of BASELINE config 1 (256 centres)
    with table rows inside its bounds.  Frenet rows: [ey, delta, vx_car, vy_car, vx_goal, wz, epsi, curv]."""
    rng = np.random.default_rng(len(cls.__name__) * 7 + len(kind))
    D, O = (8, 2 * T) if kind == "frenet" else (7, 2 * T)
    f = lambda *s, scale=1.0: (rng.normal(size=s) * scale).astype(np.float32)
    if kind == "frenet":
        x = (rng.normal(size=(N, 8)) * [.2, .2, 1, .1, 1, .1, .15, .08] + [0, 0, 4, 0, 4, 0, 0, 0]).astype(np.float32)
        lo, hi = x.min(0), x.max(0)
    else:
        card, lo, hi = _card(D, O)
        x = rng.uniform(lo, hi, size=(N, D)).astype(np.float32)
    y = np.hstack([f(N, T, scale=2.0), f(N, T, scale=0.5)])
    rbf = lambda R, K: {"centers": rng.uniform(lo, hi, size=(R, K, D)).astype(np.float32),
                        "log_sigs": rng.uniform(0.5, 1.5, size=(R, K)).astype(np.float32)}
    if cls is ClusterWCRBFNet:
        R, K = 11, 24
        net = cls(in_features=D, out_features=O, num_kernels=K, basis_func="gaussian", num_regions=R)
        params = {"params": {"rbf_list": rbf(R, K), "linear": {"kernel": f(K, O, scale=0.3), "bias": f(O, scale=0.1)},
                             "cluster": {"kernel": f(D, R), "bias": f(R)}}}
    else:
        card = _card(D, O)[0]
        if kind == "frenet":
            card["lower_bounds"], card["upper_bounds"] = [[float(v)] for v in lo], [[float(v)] for v in hi]
        net = cls.from_config(card)
        if cls is DeeperWCRBFNet:
            params = {"params": {"rbf_list": rbf(1, 256), "linear_pre1": {"kernel": f(256, 64, scale=0.1), "bias": f(64, scale=0.1)},
                                 "linear_pre2": {"kernel": f(64, 64, scale=0.2), "bias": f(64, scale=0.1)},
                                 "linear": {"kernel": f(64, O, scale=0.3), "bias": f(O, scale=0.1)}}}
        else:
            params = {"params": {"rbf_list": rbf(1, 256), "linear": {"kernel": f(256, O, scale=0.1), "bias": f(O, scale=0.1)}}}
    return net, params, x, y, (None if kind == "cartesian" else DP)


def _state0(kind, x):
    if kind == "cartesian":
        return x[:, :1]
    if kind == "cartesian_st":
        return configs.initial_state_from_query(x)
    return x[:, [0, 0, 1, 2, 3, 5, 6, 7]]


@pytest.mark.parametrize("cls,kind", [(WCRBFNet, "cartesian"), (WCRBFNet, "cartesian_st"), (WCRBFNet, "frenet"),
                                      (DeeperWCRBFNet, "cartesian"), (DeeperWCRBFNet, "frenet"),
                                      (ClusterWCRBFNet, "cartesian"), (ClusterWCRBFNet, "frenet")])
def test_evaluate_table_equals_rollout_errors_on_the_apply_outputs(cls, kind):
    net, params, x, y, dp = _net_case(cls, kind)
    N, bs = x.shape[0], 300                           # 300 does not divide 1000: the last batch has 100 rows
    xd = torch.from_numpy(x).cuda()
    outs = [net.apply(params, xd[i:i + bs]) for i in range(0, N, bs)]
    y_pred = torch.cat([o[0] if cls is ClusterWCRBFNet else o for o in outs])
    mode = evaluate.KINDS[kind][0]
    ref, ref_err = evaluate.rollout_errors(mode, _state0(kind, x), y_pred, y, dp, per_row=True)
    stats, err = evaluate.evaluate_table(net, params, x, y, kind, dp, batch_size=bs, per_row=True)
    assert tuple(err.shape) == (N, NUM_METRICS[mode]) and torch.equal(err, ref_err)
    a, b = stats.to_host(), ref.to_host()
    assert a[3] == b[3] == N
    assert np.array_equal(a[0][:, [0, 3]], b[0][:, [0, 3]]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    _assert_stats_match(err.cpu().numpy(), a[0], a[1], a[2], N)
    # without per-row output, from a DeviceTable-like pair of device tensors, in one batch
    one = evaluate.evaluate_table(net, params, xd, torch.from_numpy(y).cuda(), kind, dp, batch_size=80000)
    c = one.to_host()                                  # (the net's kernels may round a row differently in a batch of another size)
    assert c[3] == N and np.array_equal(c[0][:, 0], a[0][:, 0]) and (c[2].sum(axis=1) == c[0][:, 0]).all()
    # the summary brackets the exact quantiles of the per-row values
    summ = stats.summary()
    e = err.cpu().numpy()
    assert list(summ) == list(evaluate.METRIC_NAMES[mode])
    for m, name in enumerate(summ):
        s = summ[name]
        col = e[:, m][np.isfinite(e[:, m])].astype(np.float64)
        assert s["n"] == col.size and s["nonfinite"] == N - col.size and s["max"] == col.max() and s["argmax"] == a[1][m]
        assert abs(s["mean"] - col.mean()) <= 1e-12 * col.mean() and abs(s["rms"] - np.sqrt((col * col).mean())) <= 1e-12 * s["rms"]
        for q, (lo, hi) in s["quantiles"].items():
            exact = np.sort(col)[max(1, math.ceil(q * col.size)) - 1]          # the ceil(q n)-th smallest value
            assert lo <= exact <= hi and (lo == 0.0 or hi <= lo * 9.0 / 8.0), (name, q, lo, exact, hi)


def test_evaluate_table_kinematic_mode_and_refusals():
    net, params, x, y, dp = _net_case(WCRBFNet, "cartesian_st", N=200)
    ks = evaluate.evaluate_table(net, params, x, y, "cartesian_st", dp, mode=KS)
    ref = evaluate.rollout_errors(KS, _state0("cartesian_st", x), net.apply(params, x), y, dp)
    assert ks.mode == KS and np.array_equal(ks.to_host()[2], ref.to_host()[2])
    with pytest.raises(ValueError):
        evaluate.evaluate_table(net, params, x, y[:, :8], "cartesian_st", dp)         # out_features is not the width of y
    with pytest.raises(ValueError):
        evaluate.evaluate_table(net, params, x, y, "cartesian_st", None)              # the single-track model needs parameters
    with pytest.raises(ValueError):
        evaluate.rollout_errors(_lib.ROLLOUT_SPIRAL, x[:, :5], y, y)


def test_two_ranks_merge_to_the_one_process_result(tmp_path):
    net, params, x, y, dp = _net_case(WCRBFNet, "cartesian_st", N=1001)
    p = params["params"]
    inp, out = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(inp, x=x, y=y, centers=p["rbf_list"]["centers"], log_sigs=p["rbf_list"]["log_sigs"], kernel=p["linear"]["kernel"],
             bias=p["linear"]["bias"])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", "29561", os.path.join(root, "tests", "_evaluate_two_ranks.py"), inp, out],
                       cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    two = np.load(out)
    assert tuple(two["shards"]) == (0, 501, 501, 1001)
    # batches of 501 rows are the two ranks' shards: the net sees the same batches in both runs
    one, err = evaluate.evaluate_table(net, params, x, y, "cartesian_st", dp, batch_size=501, per_row=True)
    stats, argmax, hist, rows = one.to_host()
    assert int(two["rows"]) == rows == 1001
    assert np.array_equal(two["stats"][:, [0, 3]], stats[:, [0, 3]]) and np.array_equal(two["argmax"], argmax)
    assert np.array_equal(two["hist"], hist)
    _assert_stats_match(err.cpu().numpy(), two["stats"], two["argmax"], two["hist"], 1001)
