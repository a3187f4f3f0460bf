"""Float64 statements and bounds of the leave-one-out pass (irbfn_amd/loo.py, irbfn_rows_quad_f64): used by tests/test_loo_cpu.py
(here) and tests/test_gpu_loo.py (on the MI355X).

Statement: with z_n = [h_n | 1], A = Z^T Z + lam diag(1, .., 1, 0), s = 1 / sqrt(diag A) and L L^T = diag(s) A diag(s), the leverage
is l_n = |L^-1 diag(s) z_n|^2 (a triangular solve), the leave-one-out residual e_n / (1 - l_n), PRESS and trace their sums.
``brute_loo`` refits without the row at the same absolute lam: what the identity is held against (tests/test_loo_cpu.py).

Kernel bounds (any order of the sums; u = 2^-53): every product z_k p_kj of a float32 and a float64 value is rounded once, each
sum of m terms adds at most m - 1 roundings: |v - exact| <= (m + 1) u sum_k |z_k p_ko|.  With U_j = sum_k |z_k p_kj| the square of
a sum carries 2 (m + 1) u U_j^2 + u U_j^2, and the sum over j another (m - 1) u: |q - exact| <= (4 m + 8) u sum_j U_j^2 with room
to spare (3 m + 2 would do)."""
import numpy as np

SOLVE_RTOL = 1e-9        # tests/test_gpu_linear_fit.py: the device's solve against the float64 solve, relative to the largest weight
U53 = 2.0 ** -53


# ------------------------------------------------------------------ the kernel
def integer_case(rows, m, nd, seed):
    """Integer z [rows, m] float32 and p [m, m + nd] float64 in [-8, 8]; the strict lower triangle of p[:, :m] is NaN."""
    rng = np.random.default_rng(seed)
    z = rng.integers(-8, 9, size=(rows, m)).astype(np.float32)
    p = rng.integers(-8, 9, size=(m, m + nd)).astype(np.float64)
    p[:, :m][np.tril_indices(m, -1)] = np.nan
    return z, p


def float_case(rows, m, nd, seed):
    """Normal z and p; the strict lower triangle of p[:, :m] is NaN."""
    rng = np.random.default_rng(seed)
    z = rng.normal(size=(rows, m)).astype(np.float32)
    p = rng.normal(size=(m, m + nd))
    p[:, :m][np.tril_indices(m, -1)] = np.nan
    return z, p


def _split(p, m):
    tri = np.triu(np.where(np.isnan(p[:, :m]), 0.0, p[:, :m]))          # the strict lower triangle is not part of the statement
    return tri, p[:, m:]


def quad_int(z, p):
    """(q, v) in int64, as float64: exact while every sum is below 2^53."""
    m = z.shape[1]
    tri, dense = _split(p, m)
    zi = z.astype(np.int64)
    u = zi @ tri.astype(np.int64)
    return (u * u).sum(1).astype(np.float64), (zi @ dense.astype(np.int64)).astype(np.float64)


def quad_ref(z, p, dtype=np.longdouble):
    """(q, v, q_bound, v_bound): the statement in ``dtype`` and the any-order bounds of the float64 kernel."""
    m = z.shape[1]
    tri, dense = _split(p, m)
    zl = z.astype(dtype)
    u = zl @ tri.astype(dtype)
    q, v = (u * u).sum(1), zl @ dense.astype(dtype)
    za = np.abs(z.astype(np.float64))
    qb = (4 * m + 8) * U53 * ((za @ np.abs(tri)) ** 2).sum(1)
    vb = (m + 1) * U53 * (za @ np.abs(dense))
    return q, v, qb, vb


# ------------------------------------------------------------------ the statement
def _solve_lower(L, B):
    """L^-1 B for a lower triangular L by forward substitution (float64)."""
    X = np.array(B, dtype=np.float64, copy=True)
    for i in range(L.shape[0]):
        X[i] = (X[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def design(Zh, fit_bias=True):
    return np.hstack([Zh, np.ones((Zh.shape[0], 1))]) if fit_bias else np.asarray(Zh, np.float64)


def system(Zh, lam, fit_bias=True):
    """(Z, A0, A, s): the design matrix, Z^T Z, Z^T Z + lam diag(1, .., 1, 0) and the Jacobi scaling."""
    Z = design(Zh, fit_bias)
    K = Zh.shape[1]
    A0 = Z.T @ Z
    A = A0.copy()
    A[np.arange(K), np.arange(K)] += lam
    d = np.diag(A)
    return Z, A0, A, np.where(d > 0, 1.0 / np.sqrt(np.where(d > 0, d, 1.0)), 1.0)


def statement(Zh, Y, lam, fit_bias=True):
    """-> dict: sol [m,O], leverage [n], residual [n,O], loo_residual [n,O], rss [O], press [O], trace, gcv [O], cond (of the
    scaled matrix), all float64."""
    Z, A0, A, s = system(Zh, lam, fit_bias)
    As = A * s[:, None] * s[None, :]
    L = np.linalg.cholesky(As)
    T = _solve_lower(L, np.diag(s))                     # L^-1 diag(s)
    lev = ((Z @ T.T) ** 2).sum(1)
    sol = T.T @ (T @ (Z.T @ Y))
    e = Y - Z @ sol
    le = e / (1.0 - lev)[:, None]
    n = Z.shape[0]
    rss, tr = (e ** 2).sum(0), lev.sum()
    return dict(sol=sol, leverage=lev, residual=e, loo_residual=le, rss=rss, press=(le ** 2).sum(0), trace=tr,
                gcv=n * rss / (n - tr) ** 2, cond=np.linalg.cond(As))


def brute_loo(Zh, Y, lam, rows, fit_bias=True):
    """The residual of each row of ``rows`` under the fit of all other rows at the same absolute lam: [len(rows), O]."""
    Z, A0, A, _ = system(Zh, lam, fit_bias)
    B = Z.T @ Y
    out = []
    for i in rows:
        zi, yi = Z[i], Y[i]
        sol = np.linalg.solve(A - np.outer(zi, zi), B - np.outer(zi, yi))
        out.append(yi - zi @ sol)
    return np.array(out)


def trace_from_gram(G, K, lam, fit_bias=True):
    """trace(A_lam^-1 A_0) from the stacked Gram matrix G of [h | 1 | y] alone."""
    m = K + 1 if fit_bias else K
    A0 = np.array(G[:m, :m], dtype=np.float64)
    A = A0.copy()
    A[np.arange(K), np.arange(K)] += lam
    return float(np.trace(np.linalg.solve(A, A0)))


def leverage_bound(Z, T):
    """The kernel's bound of q for the rows Z [n,m] (float32 values) against T = L^-1 diag(s) [m,m]."""
    m = Z.shape[1]
    return (4 * m + 8) * U53 * ((np.abs(Z) @ np.abs(np.tril(T)).T) ** 2).sum(1)
