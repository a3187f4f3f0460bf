"""NumPy float64 statements of the width stage (irbfn_amd/widths.py, irbfn_knn_d2 in include/irbfn_hip.h) and the cases the CPU
and GPU tests share: the p nearest centres of every row, the two width rules with their replacement rule, and the search for
the multiplier on held-out rows.

Bounds.  gamma(D) = (D + 2) 2^-23 bounds the relative error of the float32 chain (tests/_kmeans_util.py).  Every entry of a row of
d2 moves by at most gamma relative, so its j-th smallest moves by at most that: slot j of the kernel is within gamma relative of
the reference's j-th smallest, and the centre it names is within (1 + 3 gamma) of it in float64 (both candidates' errors plus the
comparison).  A width is the square root of a mean of such d2: gamma / 2 relative from the distances, and the tests allow 2 gamma
plus one float32 rounding (2^-24) for the result."""
import functools

import numpy as np

import _kmeans_util as ku

SCALES = (0.5, 1.0, 2.0, 4.0, 8.0)


def knn_ref(q, c, p, self0=-1, d2=None):
    """(d2 [N,p] float64, idx [N,p] int32): per row the p smallest finite squared distances in ascending order of (d2, k),
    without centre self0 + n if self0 >= 0; the rest NaN / -1.  d2: the [N,K] matrix if it is already there."""
    d2 = ku.d2_ref(q, c) if d2 is None else d2
    N, K = d2.shape
    out = np.full((N, p), np.nan)
    idx = np.full((N, p), -1, np.int32)
    for n in range(N):
        ok = np.isfinite(d2[n])
        if self0 >= 0 and self0 + n < K:
            ok[self0 + n] = False
        ks = np.flatnonzero(ok)
        ks = ks[np.argsort(d2[n, ks], kind="stable")][:p]           # stable: equal d2 keeps the lower k first
        out[n, :len(ks)] = d2[n, ks]
        idx[n, :len(ks)] = ks
    return out, idx


def replace_ref(sigma):
    """The replacement rule: a sigma that is 0 or non-finite becomes the median of the finite positive ones -> (sigma, replaced)."""
    sigma = np.asarray(sigma, np.float64).copy()
    good = np.isfinite(sigma) & (sigma > 0)
    if not good.any():
        raise ValueError("no finite positive width")
    sigma[~good] = np.median(sigma[good])
    return sigma, int((~good).sum())


def nn_widths_ref(nd2, scale=1.0):
    """nd2 [K,p]: squared distances to the p nearest other centres (NaN = empty slot) -> (sigma float64 [K], replaced)."""
    nd2 = np.asarray(nd2, np.float64)
    filled = np.isfinite(nd2)
    with np.errstate(invalid="ignore", divide="ignore"):
        sigma = np.sqrt(np.where(filled, nd2, 0.0).sum(1) / filled.sum(1))
    sigma, rep = replace_ref(sigma)
    return scale * sigma, rep


def spread_widths_ref(d2, labels, K, scale=1.0, min_count=2):
    """d2 [N], labels [N] (-1 = none) -> (sigma float64 [K], replaced): the RMS distance of each cluster's rows."""
    d2, labels = np.asarray(d2, np.float64), np.asarray(labels)
    ok = labels >= 0
    counts = np.bincount(labels[ok], minlength=K)
    sums = np.bincount(labels[ok], weights=d2[ok], minlength=K)
    with np.errstate(invalid="ignore", divide="ignore"):
        sigma = np.where(counts >= min_count, np.sqrt(sums / counts), np.nan)
    sigma, rep = replace_ref(sigma)
    return scale * sigma, rep


# ------------------------------------------------------------------ the scale search
def hidden32(x, c, sigma):
    """The gaussian hidden layer exp(-|x - c|^2 / sigma^2) of an ungated one-region net, rounded to float32, as float64."""
    return np.exp(-ku.d2_ref(x, c) / np.asarray(sigma, np.float64)[None] ** 2).astype(np.float32).astype(np.float64)


def solve_ref(h, y, ridge):
    """NormalEquations.solve in NumPy: lambda = ridge trace(H^T H) / K on the weights, none on the bias, Jacobi scaling, Cholesky, the
    pivot test -> sol [K+1,O], or None where the system is not positive definite."""
    K = h.shape[1]
    A1 = np.hstack([h, np.ones((len(h), 1))])
    A = A1.T @ A1
    A[np.arange(K), np.arange(K)] += ridge * np.trace(h.T @ h) / K
    d = np.diagonal(A)
    s = np.where(d > 0, 1.0 / np.sqrt(np.where(d > 0, d, 1.0)), 1.0)
    try:
        L = np.linalg.cholesky(A * s[:, None] * s[None, :])
    except np.linalg.LinAlgError:
        return None
    if not (np.diagonal(L) ** 2 > (K + 1) * 2.0 ** -52).all():
        return None
    t = np.linalg.solve(L, (A1.T @ y) * s[:, None])
    return np.linalg.solve(L.T, t) * s[:, None]


def price_ref(x, y, c, sigma, holdout_every=5, ridge=1e-8):
    """(train MSE, held-out MSE) of the closed-form fit at widths sigma: fitted on the rows with index % holdout_every != 0, priced on
    the rest; inf where the system is not positive definite."""
    ho = np.arange(len(x)) % holdout_every == 0
    h = hidden32(x, c, sigma)
    y = np.asarray(y, np.float64)
    sol = solve_ref(h[~ho], y[~ho], ridge)
    if sol is None:
        return np.inf, np.inf
    res = np.hstack([h, np.ones((len(h), 1))]) @ sol - y
    return float((res[~ho] ** 2).mean()), float((res[ho] ** 2).mean())


def scale_search_ref(x, y, c, sigma, scales=SCALES, holdout_every=5, ridge=1e-8):
    """-> (train MSE per scale, held-out MSE per scale, best index)."""
    both = [price_ref(x, y, c, s * np.asarray(sigma, np.float64), holdout_every, ridge) for s in scales]
    held = [b[1] for b in both]
    return [b[0] for b in both], held, int(np.argmin(held))


def e2e_problem(s, seed=0, N=4096):
    """x float32 uniform in [0, s]^3, y float32 = (sin 6 u0 + u2 cos 5 u1, u0 u1 - u2^2) with u = x / s."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(0.0, 1.0, (N, 3))
    x = (u * s).astype(np.float32)
    u = x.astype(np.float64) / s
    y = np.stack([np.sin(6 * u[:, 0]) + u[:, 2] * np.cos(5 * u[:, 1]), u[:, 0] * u[:, 1] - u[:, 2] ** 2], 1).astype(np.float32)
    return x, y


def e2e_cfg(K=64, D=3, O=2):
    """The model card of an ungated one-region gaussian net."""
    return dict(in_features=D, out_features=O, num_kernels=K, basis_func="gaussian", num_regions=1, lower_bounds=[], upper_bounds=[],
                dimension_ranges=[[]], activation_idx=[], delta=[])


def lloyd_centers(x, K=64, iters=10, seed=0):
    """K random rows, then `iters` Lloyd iterations in float64, rounded to float32 after each (as the device holds them)."""
    rng = np.random.default_rng(seed)
    c = x[rng.choice(len(x), K, replace=False)].astype(np.float64)
    for _ in range(iters):
        c = ku.lloyd_step(x, c)["centers"].astype(np.float32).astype(np.float64)
    return c.astype(np.float32)


# ------------------------------------------------------------------ shared cases of the kernel
# (N, K, D, p, self0): every N of {1, 63, 64, 65, 257, 1000}, K of {1, 2, p, p + 1, 255, 256, 257, 1025}, D of {1, 3, 7, 8, 16} and
# p of {1, 2, 3, 8, 16}; p > K, p = K and the self case p = K - 1 among them.  self0 = 0: the rows are the first N centres.
KNN_CASES = (
    (1, 1, 1, 1, -1), (63, 2, 3, 2, -1), (64, 3, 7, 2, -1), (65, 255, 8, 3, -1), (257, 256, 16, 8, -1), (1000, 257, 3, 16, -1),
    (1000, 1025, 8, 1, -1), (257, 1025, 7, 16, 0), (65, 8, 1, 16, -1), (64, 16, 16, 16, -1), (63, 17, 3, 16, -1), (9, 9, 8, 8, 0),
    (1000, 2, 1, 3, -1), (1, 1025, 16, 8, -1), (257, 4, 7, 3, -1), (64, 3, 8, 3, -1), (257, 257, 3, 2, 0), (65, 1025, 1, 2, -1),
    (1, 1, 3, 2, 0),
)


@functools.lru_cache(maxsize=None)
def knn_case(N, K, D, p, self0):
    """(q, c, d2 [N,p], idx [N,p], full d2 [N,K]) of one case, computed once, read-only."""
    x, c = ku.uniform_case(max(N, 4), K, D, seed=1000 * D + K + p)
    q = c[:N].copy() if self0 >= 0 else x[:N]
    full = ku.d2_ref(q, c)
    d2, idx = knn_ref(q, c, p, self0, d2=full)
    for a in (q, c, d2, idx, full):
        a.setflags(write=False)
    return q, c, d2, idx, full


def duplicate_case():
    """40 centres at D = 3, uniform in +-3, with two bit-for-bit duplicate pairs (7 = 2, 31 = 30)."""
    rng = np.random.default_rng(17)
    c = rng.uniform(-3, 3, (40, 3)).astype(np.float32)
    c[7] = c[2]
    c[31] = c[30]
    return c
