"""NumPy float64 statements of OLS forward selection (irbfn_amd/ols.py, irbfn_ols_begin / irbfn_ols_steps in include/irbfn_hip.h)
and the cases the CPU and GPU tests share.

``ols_ref`` is the Gram form the kernel computes: a Cholesky factorisation of A = H^T H + lambda I (+ the ones column) whose pivot
is the column with the largest (sum_o c[i,o]^2) / d[i].  ``lstsq_gains`` is the independent statement: numpy.linalg.lstsq on the
ridge-augmented columns themselves, never on their Gram matrix.

TOL.  The two statements were compared on CASES (tests/test_ols_cpu.py prints the figures): the same index at every step, and the
largest relative difference of a step's gain (summed over the outputs) or of an entry of the objective was MEASURED.  Nearly all of
it is the lstsq statement's own error: its gain is the difference of two objectives, which cancels where a step explains little
(against the largest entry of each array the two agree to 4.3e-15).  TOL is 16 times MEASURED: the factor covers another order of
the sums (the kernel splits the sum over the factor into 16 x 4 partial sums).  The GPU tests hold every array to TOL times its
largest magnitude."""
import functools

import numpy as np

import _kmeans_util as ku
import _linear_fit_util as lu
import _widths_util as wu

MEASURED = 1.65e-12                      # largest reference-against-reference difference over CASES: a step's gain of (2000, 257, 10, 20);
                                         # 1.5e-13 and 4.2e-13 on the other two, objectives 5.5e-14
TOL = 16 * MEASURED
GAP = 1000 * TOL                         # every step of every case: (best score - second best) / best > GAP (asserted on the CPU)
RIDGE = 1e-8
CASES = ((300, 40, 2, 12), (500, 65, 1, 33), (2000, 257, 10, 20))           # (N, M, O, K)
EDGE_M = (1, 2, 63, 64, 65, 257, 1025)
EDGE_K = (1, 33, 65)
EDGE_O = (1, 2, 10)


def npad(M):
    return (M + 1 + 63) // 64 * 64


def lam_of(G, M, ridge=RIDGE):
    return ridge * np.trace(G[:M, :M]) / M


def default_tol(M, fit_bias):
    return (M + (1 if fit_bias else 0)) * 2.0 ** -52


def ols_ref(G, M, O, kmax, fit_bias=True, lam=None, tol=None):
    """The statement.  -> dict: sel [count] (the ones column M included), count, gain [count,O], objective [count + 1,O] (row 0 =
    diag G_yy), L [count,n], d [n], d0 [n], c [n,O], and per step the two best scores (``best``, ``second``; nan where the pivot was
    the ones column or there was no second candidate)."""
    G = np.asarray(G, np.float64)
    n = M + 1 if fit_bias else M
    lam = lam_of(G, M) if lam is None else lam
    tol = default_tol(M, fit_bias) if tol is None else tol
    A = G[:n, :n].copy()
    A[np.arange(M), np.arange(M)] += lam
    d = np.diagonal(A).copy()
    d0 = d.copy()
    c = G[:n, M + 1:].copy()
    avail = np.ones(n, bool)
    L, sel, gain, best, second = [], [], [], [], []
    for t in range(kmax + (1 if fit_bias else 0)):
        if fit_bias and t == 0:
            if not d[M] > 0:
                break
            j, b1, b2 = M, np.nan, np.nan
        else:
            ok = avail[:M] & (d[:M] > tol * d0[:M])
            score = np.zeros(M)
            with np.errstate(invalid="ignore", divide="ignore"):
                score[ok] = (c[:M][ok] ** 2).sum(1) / d[:M][ok]
            score[~(score > 0)] = 0.0                              # a NaN or a non-positive score never wins
            j = int(np.argmax(score))                              # the first of equal maxima
            if not score[j] > 0:
                break
            rest = np.delete(score, j)
            b1, b2 = score[j], (rest.max() if rest.size else np.nan)
        sq = np.sqrt(d[j])
        col = np.zeros(n)
        dot = np.zeros(n)
        for s in range(t):
            dot += L[s] * L[s][j]
        col[avail] = (A[avail, j] - dot[avail]) / sq
        col[j] = sq
        ly = c[j] / sq
        L.append(col)
        gain.append(ly ** 2)
        d[avail] -= col[avail] ** 2
        c[avail] -= col[avail, None] * ly[None]
        avail[j] = False
        sel.append(j)
        best.append(b1)
        second.append(b2)
    gain = np.array(gain).reshape(len(sel), O)
    yty = np.diagonal(G)[M + 1:]
    return dict(sel=np.array(sel, np.int32), count=len(sel), gain=gain, objective=np.vstack([yty[None], yty[None] - np.cumsum(gain, 0)]),
                L=np.array(L).reshape(len(sel), n), d=d, d0=d0, c=c, best=np.array(best), second=np.array(second))


def lstsq_gains(H, Y, lam, fit_bias, prefix):
    """The independent statement: with the candidates ``prefix`` (and the ones column) in, the drop of min_w rss + lam |w|^2 per
    output that each further candidate would bring -> (gains [M,O], nan for the members; objective [O] of the prefix).  One
    numpy.linalg.lstsq on the augmented columns [h_i; sqrt(lam) e_i]: the residual of the augmented candidate column against the
    prefix, r_i, gives the drop (r_i . r_y)^2 / (r_i . r_i)."""
    N, M = H.shape
    Ha = np.vstack([H, np.sqrt(lam) * np.eye(M)])
    Ya = np.vstack([Y, np.zeros((M, Y.shape[1]))])
    cols = [Ha[:, i] for i in prefix]
    if fit_bias:
        cols.append(np.concatenate([np.ones(N), np.zeros(M)]))
    rhs = np.hstack([Ya, Ha])
    if cols:
        P = np.stack(cols, 1)
        rhs = rhs - P @ np.linalg.lstsq(P, rhs, rcond=None)[0]
    ry, rh = rhs[:, :Y.shape[1]], rhs[:, Y.shape[1]:]
    with np.errstate(invalid="ignore", divide="ignore"):
        gains = (rh.T @ ry) ** 2 / (rh * rh).sum(0)[:, None]
    gains[list(prefix)] = np.nan
    return gains, (ry * ry).sum(0)


def lstsq_path(H, Y, lam, fit_bias, K):
    """Forward selection by lstsq alone, prefix by prefix -> (sel [K], gain [K,O], objective [K + 1,O] (row 0: the ones column
    alone, or y^T y), best and second-best summed gains per step).  The candidates are ranked by ``lstsq_gains``; the objective of
    every prefix is the residual of its own lstsq, and a gain is the drop from one prefix to the next."""
    sel, obj, best, second = [], [], [], []
    for _ in range(K):
        g, o = lstsq_gains(H, Y, lam, fit_bias, sel)
        tot = np.where(np.isnan(g.sum(1)), -np.inf, g.sum(1))
        srt = np.sort(tot)
        obj.append(o)
        sel.append(int(np.argmax(tot)))
        best.append(srt[-1])
        second.append(srt[-2] if len(srt) > 1 else np.nan)
    obj.append(lstsq_gains(H, Y, lam, fit_bias, sel)[1])
    obj = np.array(obj)
    return np.array(sel, np.int32), obj[:-1] - obj[1:], obj, np.array(best), np.array(second)


def design(N, M, O, seed=None, D=3, sigma=1.5):
    """(H [N,M] = the float32 gaussian hidden layer of ku.uniform_case centres at sigma, as float64; Y [N,O] float32 values = five
    of its columns mixed per output plus N(0, 0.1) noise; x, c)."""
    seed = 7000 + 10 * M + O if seed is None else seed
    x, c = ku.uniform_case(N, M, D, seed=seed)
    H = wu.hidden32(x, c, np.full(M, sigma))
    rng = np.random.default_rng(seed + 1)
    five = rng.choice(M, min(5, M), replace=False)
    Y = H[:, five] @ rng.normal(size=(len(five), O)) + 0.1 * rng.normal(size=(N, O))
    return H, Y.astype(np.float32).astype(np.float64), x, c


@functools.lru_cache(maxsize=None)
def case(N, M, O):
    """(H, Y, G) of one design, computed once, read-only."""
    H, Y, _, _ = design(N, M, O)
    G = lu.stacked_gram(H, Y)
    for a in (H, Y, G):
        a.setflags(write=False)
    return H, Y, G


def edge_rows(M):
    """Rows of the shape-edge designs: enough for M independent columns, and few."""
    return max(2 * M, 64) if M <= 257 else M + 200


def rel_entries(a, b):
    """max |a / b - 1| over the entries."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a / b - 1).max())


def rel(a, b):
    """max |a - b| / max |b| (0 for two empty arrays)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / np.abs(b).max()) if b.size else 0.0


def integer_tie_design():
    """An exact integer design [N,6] | Y [N,2]: columns 1 and 4 are the same multiset of values against y (column 4 is column 1
    with rows permuted among rows where every other column and y agree), so their Gram rows agree entry for entry except for
    each other's position, and every score of theirs is bit-equal.  Small integers: every product and sum is exact."""
    rng = np.random.default_rng(23)
    base = rng.integers(-3, 4, size=(40, 5)).astype(np.float64)       # columns 0, 1, 2, 3, 5 of one half
    v = rng.integers(1, 4, size=40).astype(np.float64)
    yb = rng.integers(-1, 2, size=(40, 2)).astype(np.float64)
    yb[:, 0] += 2 * v                                                 # y leans on columns 1 and 4 alike
    # rows come in pairs (r, r') that agree in every column but 1 and 4, where they hold (v, 0) and (0, v)
    top = np.column_stack([base[:, 0], v, base[:, 2], base[:, 3], 0 * v, base[:, 4]])
    bot = np.column_stack([base[:, 0], 0 * v, base[:, 2], base[:, 3], v, base[:, 4]])
    return np.vstack([top, bot]), np.vstack([yb, yb])
