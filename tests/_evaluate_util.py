"""Helpers of test_evaluate_cpu.py and test_gpu_evaluate.py: the float64 NumPy statement of the roll-out error metrics of
irbfn_eval_rollout_errors (include/irbfn_hip.h) on the oracle's roll-outs, the bound a float32 evaluation of them is held to,
the histogram's bin function on float32 bit patterns with its edges, and the statistics of a [B, M] table of metrics.  A plain
module (no fixtures, no hooks)."""
import math

import numpy as np

from _rollout_util import RTOL
from oracle import c_oracle as co
from oracle import irbfn_oracle as orc

SELECT, KS, FULLINT, FRENET, SPIRAL = 0, 1, 2, 3, 4
MODES = (SELECT, KS, FULLINT, FRENET)
STATE_DIM = {SELECT: 7, KS: 7, FULLINT: 5, FRENET: 8}
NUM_METRICS = {m: s + 2 for m, s in STATE_DIM.items()}
NUM_BINS, BIN_BIAS = 512, 696
U32 = 2.0 ** -23


def f32(a):
    """float32-rounded values as a float64 array: what both the kernel and the float64 statement start from."""
    return np.asarray(a, np.float32).astype(np.float64)


def rollouts(mode, state0, u, dp):
    """(float64 oracle, float32 restatement) states [B, T, S] of controls u [B, 2T] from state0 [B, S0] (FULLINT: v0 [B, 1])."""
    T = u.shape[1] // 2
    if mode == FULLINT:
        return (orc.rollout_fullint(state0[:, 0], u),
                co.rollout_fullint(state0[:, 0].astype(np.float32), u.astype(np.float32), T, np.float32))
    xu = np.hstack([state0, u])
    x32, dp32 = xu.astype(np.float32), np.asarray(dp, np.float32)
    if mode == SELECT:
        return orc.integrate_st_mult(xu, dp), co.integrate_st_mult(x32, dp32, T, np.float32)
    if mode == KS:
        return orc.integrate_st_ks_mult(xu, dp), co.integrate_st_mult(x32, dp32, T, np.float32, True)
    return orc.integrate_frenet_mult(xu, dp), co.integrate_frenet_mult(x32, dp32, T, np.float32)


def final_state_bound(ref, ref32, rtol=RTOL, floor=1e-3, k32=4.0):
    """What _rollout_util.assert_states_close grants the FINAL state of a roll-out, [B, S]: rtol of |ref| + scale (scale = the
    component's largest magnitude along the trajectory), or k32 x the error of the float32 restatement on that trajectory
    component, whichever is larger."""
    scale = np.maximum(np.abs(ref).max(axis=1), floor)
    e32 = np.abs(np.asarray(ref32, np.float64) - ref).max(axis=1)
    return np.maximum(rtol * (np.abs(ref[:, -1]) + scale), k32 * e32 + 1e-7 * scale)


def metrics64(mode, state0, y_pred, y, dp):
    """The M = S + 2 metrics of every row in float64 and the bound of a float32 evaluation, both [B, M].  Inputs are taken at
    their float32 values.  Bounds: a component gets the sum of final_state_bound of the prediction's and the label's
    roll-out; `position` (hypot of components 0 and 1) the sum of those two components' bounds; `controls` 4 * 2^-23 *
    mean(|y_pred| + |y|) (one rounding per difference, one of the mean, with room for the summation)."""
    state0, y_pred, y = f32(state0), f32(y_pred), f32(y)
    S = STATE_DIM[mode]
    p, p32 = rollouts(mode, state0, y_pred, dp)
    a, a32 = rollouts(mode, state0, y, dp)
    d = p[:, -1] - a[:, -1]
    err = np.empty((y.shape[0], S + 2))
    err[:, :S] = np.abs(d)
    err[:, S] = np.hypot(d[:, 0], d[:, 1])
    err[:, S + 1] = np.abs(y_pred - y).mean(axis=1)
    bound = np.empty_like(err)
    bound[:, :S] = final_state_bound(p, p32) + final_state_bound(a, a32)
    bound[:, S] = bound[:, 0] + bound[:, 1]
    bound[:, S + 1] = 4.0 * U32 * (np.abs(y_pred) + np.abs(y)).mean(axis=1)
    return err, bound


def bin_of(e):
    """The histogram bin of float32 values, from their bit patterns: clamp((bits >> 20) - 696, 0, 511)."""
    bits = np.ascontiguousarray(e, dtype=np.float32).view(np.uint32).astype(np.int64)
    return np.clip((bits >> 20) - BIN_BIAS, 0, NUM_BINS - 1)


def edge(k):
    """Lower edge of bin k: 2^(-40 + k // 8) * (1 + (k mod 8) / 8)."""
    k = int(k)
    return math.ldexp(1.0 + (k % 8) / 8.0, -40 + k // 8)


def table_stats(err, row0=0):
    """The statistics of a [B, M] float32 table of metrics as the kernel defines them: stats [M, 4] = (n, fsum, fsum of squares,
    max) over the finite values (max = -inf without one), argmax [M] = row0 + the first row that attains max (-1 without one),
    hist [M, 512], and abs_terms [M, 2] = (sum |e|, sum e^2), the scale of the summation bound."""
    err = np.asarray(err, np.float32)
    M = err.shape[1]
    stats = np.zeros((M, 4))
    argmax = np.full(M, -1, np.int64)
    hist = np.zeros((M, NUM_BINS), np.int64)
    terms = np.zeros((M, 2))
    for m in range(M):
        col = err[:, m]
        fin = np.isfinite(col)
        v = col[fin].astype(np.float64)
        stats[m] = (v.size, math.fsum(v), math.fsum(v * v), v.max() if v.size else -np.inf)
        if v.size:
            argmax[m] = row0 + int(np.flatnonzero(fin & (col == col[fin].max()))[0])
        hist[m] = np.bincount(bin_of(col[fin]), minlength=NUM_BINS)
        terms[m] = (math.fsum(np.abs(v)), math.fsum(v * v))
    return stats, argmax, hist, terms


def sum_bound(rows, terms):
    """|sum - fsum| of `rows` float64 terms added in any order: rows * 2^-52 * sum |terms| (each partial sum is at most
    sum |terms| and rounds once, to half an ulp of 2^-52)."""
    return rows * 2.0 ** -52 * terms


def net_card(D, O, K=256):
    """(model card, lower bounds, upper bounds) of a one-region gaussian net at the size of BASELINE config 1 (256 centres)."""
    lo, hi = ([0.0, 0.0, 0.0, -3.1, 0.0, -0.6, -3.0, -1.0][:D], [7.0, 3.6, 3.6, 3.2, 7.0, 0.4, 2.5, 1.0][:D])
    return {"in_features": D, "out_features": O, "num_kernels": K, "basis_func": "gaussian", "num_regions": 1,
            "lower_bounds": [[v] for v in lo], "upper_bounds": [[v] for v in hi], "dimension_ranges": [[0] * D],
            "activation_idx": list(range(D)), "delta": [100.0] * D}, np.array(lo), np.array(hi)
