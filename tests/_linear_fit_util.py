"""Shared cases and float64 statements of the closed-form output-layer fit (irbfn_amd/linear_fit.py): used by
tests/test_linear_fit_cpu.py (here) and tests/test_gpu_linear_fit.py (on the MI355X).

Gram matrix: every float32 x float32 product is exact in float64, so any summation order of `rows` of them is within
rows 2^-53 sum_n |z_ni z_nj| of the real sum (``gram_bound``); integer rows with |z| <= 1024 keep every partial sum below
2^53 up to 2^33 rows, so there the float64 result is the int64 one bit for bit.

Hidden layer: |h - h64| <= 1e-5 |h64| + 3e-6 sum_r gamma64[b,r] max(1, |phi64[b,r,k]|) per entry (``hidden_ref``): the project's
forward tolerance read with W = I.  It has no absolute gate term, so the synthetic nets keep their queries inside the gate's
box, at least 1 / delta from its faces."""
import functools

import numpy as np

from oracle import irbfn_oracle as orc

BASES = ("gaussian", "gaussian_wide", "gaussian_wider", "inverse_quadratic", "linear", "quadratic", "multiquadric",
         "inverse_multiquadric", "spline", "poisson_one", "poisson_two", "matern32", "matern52")
SYN_DIMS = (1, 3, 7, 8)
SYN_KS = (1, 17, 64)
SYN_B = 96                      # a full tile of 64 queries and a ragged one
BOX, DELTA = 4.0, 5.0           # the synthetic nets' gate: [0, BOX]^D, queries in [1 / DELTA + margin, BOX - ...]


# ------------------------------------------------------------------ Gram matrix
def integer_rows(rows, M, seed):
    """Integer-valued float32 rows, |z| <= 1024, another (asymmetric) range per column."""
    rng = np.random.default_rng(seed)
    lo = -rng.integers(0, 1025, size=M)
    hi = rng.integers(0, 1025, size=M)
    return rng.integers(lo, hi + 1, size=(rows, M)).astype(np.float32)


def gram_int(z, block=128):
    """z^T z in int64 (NumPy's integer product runs without BLAS: the lower block triangle only, mirrored), as float64."""
    zi = z.astype(np.int64)
    M = zi.shape[1]
    if M <= 2 * block:
        return (zi.T @ zi).astype(np.float64)
    G = np.zeros((M, M), np.int64)
    for c0 in range(0, M, block):
        c1 = min(c0 + block, M)
        blk = zi[:, c0:c1].T @ zi[:, :c1]
        G[c0:c1, :c1] = blk
        G[:c1, c0:c1] = blk.T
    return G.astype(np.float64)


def float_rows(rows, M, seed):
    """z ~ N(0,1) 2^U(-8,8) per column."""
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(rows, M)) * 2.0 ** rng.uniform(-8, 8, size=M)).astype(np.float32)


def gram_ref(z):
    z64 = z.astype(np.float64)
    return z64.T @ z64


def gram_bound(z):
    """rows 2^-53 sum_n |z_ni z_nj| per entry: the bound of any summation order over exact products."""
    a = np.abs(z.astype(np.float64))
    return z.shape[0] * 2.0 ** -53 * (a.T @ a)


# ------------------------------------------------------------------ hidden layer
def hidden_ref(cfg, params, x32):
    """(h64 [B,K], bound [B,K]) of float32 queries from the float64 oracle."""
    p64 = orc.cast_params(params, np.float64)
    x64 = np.asarray(x32, np.float32).astype(np.float64)
    _, h64, g64 = orc.wcrbfnet_apply(cfg, p64, x64, return_aux=True)
    pp = p64["params"] if "params" in p64 else p64
    phi = orc.rbf_layer(x64, pp["rbf_list"]["centers"], pp["rbf_list"]["log_sigs"], cfg["basis_func"])
    bound = 1e-5 * np.abs(h64) + 3e-6 * np.einsum("br,brk->bk", g64, np.maximum(1.0, np.abs(phi)))
    return h64, bound


def hidden_restated32(cfg, params, x32):
    """The reference's own arithmetic in float32 (NumPy): what a float32 evaluation may differ from the float64 one by."""
    _, h32, _ = orc.wcrbfnet_apply(cfg, orc.cast_params(params, np.float32), np.asarray(x32, np.float32), return_aux=True)
    return np.asarray(h32, np.float64)


def ratio(h, h64, bound):
    """max err / bound (0 / 0 counts as inside)."""
    err = np.abs(np.asarray(h, np.float64) - h64)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err <= bound, np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0), np.inf)
    return float(r.max())


def synthetic_cfg(D, K, basis, O=2):
    return dict(in_features=D, out_features=O, num_kernels=K, basis_func=basis, num_regions=1, lower_bounds=[[0.0]] * D,
                upper_bounds=[[BOX]] * D, dimension_ranges=[[0] * D], activation_idx=list(range(D)), delta=[DELTA] * D)


@functools.lru_cache(maxsize=None)
def synthetic_case(D, K, basis):
    """(cfg, params, x32, h64, bound) of a one-region net with every dimension gated, computed once, read-only."""
    seed = 1000 * D + 10 * K + BASES.index(basis)
    rng = np.random.default_rng(seed)
    cfg = synthetic_cfg(D, K, basis)
    params = {"params": {"rbf_list": {"centers": rng.uniform(0.0, BOX, size=(1, K, D)).astype(np.float32),
                                      "log_sigs": rng.uniform(0.0, 1.5, size=(1, K)).astype(np.float32)},
                         "linear": {"kernel": rng.normal(size=(K, 2)).astype(np.float32), "bias": np.zeros(2, np.float32)}}}
    x = rng.uniform(1.0 / DELTA + 0.05, BOX - 1.0 / DELTA - 0.05, size=(SYN_B, D)).astype(np.float32)
    h64, bound = hidden_ref(cfg, params, x)
    for a in (x, h64, bound):
        a.setflags(write=False)
    return cfg, params, x, h64, bound


# ------------------------------------------------------------------ the solve
def lstsq_ref(Zh, Y, lam, fit_bias):
    """numpy.linalg.lstsq of the stacked system [Z_h 1; sqrt(lam) I 0] [W; b] = [Y; 0] in float64 -> (W, b, rss)."""
    n, K = Zh.shape
    A = np.hstack([Zh, np.ones((n, 1))]) if fit_bias else Zh
    top = A
    if lam > 0:
        reg = np.hstack([np.sqrt(lam) * np.eye(K), np.zeros((K, A.shape[1] - K))])
        top = np.vstack([A, reg])
    rhs = np.vstack([Y, np.zeros((top.shape[0] - n, Y.shape[1]))])
    sol = np.linalg.lstsq(top, rhs, rcond=None)[0]
    rss = ((A @ sol - Y) ** 2).sum(0)
    return sol[:K], (sol[K] if fit_bias else np.zeros(Y.shape[1])), rss


def stacked_gram(Zh, Y):
    Z = np.hstack([Zh, np.ones((Zh.shape[0], 1)), Y])
    return Z.T @ Z


class Shape:
    """What NormalEquations reads of a net."""
    use_float64 = False

    def __init__(self, K, O):
        self.num_kernels, self.out_features = K, O


# ------------------------------------------------------------------ the end-to-end case
@functools.lru_cache(maxsize=None)
def fit_case():
    """D = 3, K = 48: a jittered 4 x 4 x 3 grid of centres in [0.5, 3.5]^3, sigma ~ U(0.45, 0.7), gaussian, one region on
    [0, 4]^3 with delta = 15, O = 3; 1500 queries in [0.2, 3.8]^3; y = net(x; W*, b*) + N(0, 0.05).
    -> (cfg, centers [K,3], log_sigs [K], x32, y32, h64, bound_terms) with bound_terms = (|h64|, sum_r gamma) for the tolerance."""
    rng = np.random.default_rng(7)
    gx, gy, gz = np.meshgrid(np.linspace(0.5, 3.5, 4), np.linspace(0.5, 3.5, 4), np.linspace(0.5, 3.5, 3), indexing="ij")
    centers = (np.stack([gx, gy, gz], -1).reshape(-1, 3) + rng.uniform(-0.15, 0.15, size=(48, 3))).astype(np.float32)
    log_sigs = np.log(rng.uniform(0.45, 0.7, size=48)).astype(np.float32)
    cfg = dict(in_features=3, out_features=3, num_kernels=48, basis_func="gaussian", num_regions=1, lower_bounds=[[0.0]] * 3,
               upper_bounds=[[4.0]] * 3, dimension_ranges=[[0, 0, 0]], activation_idx=[0, 1, 2], delta=[15.0] * 3)
    x = rng.uniform(0.2, 3.8, size=(1500, 3)).astype(np.float32)
    Wt, bt = rng.normal(size=(48, 3)), rng.normal(size=3)
    p = {"params": {"rbf_list": {"centers": centers[None].astype(np.float64), "log_sigs": log_sigs[None].astype(np.float64)},
                    "linear": {"kernel": Wt, "bias": bt}}}
    out, h64, g64 = orc.wcrbfnet_apply(cfg, p, x.astype(np.float64), return_aux=True)
    y = (out + rng.normal(scale=0.05, size=out.shape)).astype(np.float32)
    for a in (centers, log_sigs, x, y, h64, g64):
        a.setflags(write=False)
    return cfg, centers, log_sigs, x, y, h64, g64.sum(1)
