"""NumPy float64 statement of one Lloyd iteration as irbfn_kmeans_step defines it (include/irbfn_hip.h), the bounds the
float32 kernel is held to, and the cases the CPU and GPU tests share.

Bounds.  gamma(D) = (D + 2) 2^-23 bounds the relative error of the float32 chain d2 = fmaf(t, t, d2), t = x - c, for O(1)
data: rounding t costs 2^-24 of t, so t^2 carries about 2 * 2^-24; each of the D fused adds costs 2^-24 of a running sum
of positive terms; in total <= (D + 2) 2^-24, and gamma doubles it.  A label is right when the float64 distance to the
chosen centre is within (1 + 3 gamma) of the smallest one (both candidates' errors plus the comparison).  A new centre is
within 2^-23 max_n |x[n,d]| of the float64 mean over the kernel's own labels: 2^-24 for the float32 rounding of the result
and as much again for the accumulation."""
import numpy as np


def gamma(D):
    return (D + 2) * 2.0 ** -23


def d2_ref(x, c):
    """[N,K] float64 squared distances, brute force; non-finite entries stay non-finite."""
    x = np.asarray(x, np.float64)
    c = np.asarray(c, np.float64)
    out = np.empty((x.shape[0], c.shape[0]))
    with np.errstate(invalid="ignore", over="ignore"):
        for k0 in range(0, c.shape[0], 256):
            t = x[:, None, :] - c[None, k0:k0 + 256, :]
            out[:, k0:k0 + 256] = (t * t).sum(axis=2)
    return out


def labels_of(d2):
    """First-minimum argmin over the finite entries of each row of d2 [N,K]; -1 for a row without one."""
    d = np.where(np.isfinite(d2), d2, np.inf)
    lab = d.argmin(axis=1).astype(np.int32)
    lab[~np.isfinite(d.min(axis=1))] = -1
    return lab


def update_of(x, c, lab):
    """(new centres float64 [K,D], counts int64 [K]) from labels: the mean of the rows labelled k; an empty cluster keeps c[k]."""
    x = np.asarray(x, np.float64)
    new = np.asarray(c, np.float64).copy()
    K = new.shape[0]
    ok = lab >= 0
    counts = np.bincount(lab[ok], minlength=K).astype(np.int64)
    sums = np.zeros_like(new)
    np.add.at(sums, lab[ok], x[ok])
    nz = counts > 0
    new[nz] = sums[nz] / counts[nz, None]
    return new, counts


def lloyd_step(x, c, prev=None):
    """One iteration in float64 -> dict(labels, d2, centers, counts, finite, inertia, moved, shift2).  prev: the labels on entry
    (None = all -1).  Rows without a finite distance get -1 / NaN and enter nothing."""
    d2 = d2_ref(x, c)
    lab = labels_of(d2)
    ok = lab >= 0
    best = np.full(len(lab), np.nan)
    best[ok] = d2[ok, lab[ok]]
    new, counts = update_of(x, c, lab)
    prev = np.full(len(lab), -1, np.int32) if prev is None else np.asarray(prev)
    moved_c = new[counts > 0] - np.asarray(c, np.float64)[counts > 0]
    return dict(labels=lab, d2=best, centers=new, counts=counts, finite=int(ok.sum()), inertia=float(best[ok].sum()),
                moved=int((prev[ok] != lab[ok]).sum()),
                shift2=float((moved_c ** 2).sum(axis=1).max()) if moved_c.size else 0.0)


def shift2_exact(new32, old32, counts):
    """max_k ||new_k - old_k||^2 over the non-empty clusters from float32 centres, in extended precision."""
    nz = np.asarray(counts) > 0
    if not nz.any():
        return 0.0
    t = np.asarray(new32)[nz].astype(np.longdouble) - np.asarray(old32)[nz].astype(np.longdouble)
    return float((t * t).sum(axis=1).max())


def d2_chain32(x, c):
    """The kernel's float32 chain with separate multiply and add: equal to the fused chain wherever every product and sum is
    exact in float32 (integer grids below 2^24)."""
    x = np.asarray(x, np.float32)
    c = np.asarray(c, np.float32)
    d2 = np.zeros((x.shape[0], c.shape[0]), np.float32)
    for d in range(x.shape[1]):
        t = x[:, d, None] - c[None, :, d]
        d2 = t * t + d2
    return d2


BLOB_MEANS = np.array([(0, 0), (100, 0), (0, 100), (100, 100), (50, 250)], np.float64)


def blobs(seed=3):
    """Five blobs of 400 rows, sigma = 1 -> (x float32 [2000,2] shuffled, blob id per row, init [5,2] = one seed row per blob)."""
    rng = np.random.default_rng(seed)
    ids = np.repeat(np.arange(5), 400)
    x = (BLOB_MEANS[ids] + rng.normal(size=(2000, 2))).astype(np.float32)
    p = rng.permutation(2000)
    x, ids = x[p], ids[p].astype(np.int32)
    init = np.stack([x[np.flatnonzero(ids == b)[0]] for b in range(5)])
    return x, ids, init


def uniform_case(N, K, D, seed):
    """x [N,D], c [K,D] float32 uniform in +-3; the first centres sit on rows of x (zero distances)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-3, 3, (N, D)).astype(np.float32)
    c = rng.uniform(-3, 3, (K, D)).astype(np.float32)
    m = min(K, N, 4)
    c[:m] = x[:m]
    return x, c


def integer_case(N=2000, K=97, D=16, lim=256, seed=5):
    """Integer coordinates in [-lim, lim]: every float32 operation of the chain is exact (largest d2 = D (2 lim)^2 < 2^24)."""
    rng = np.random.default_rng(seed)
    return (rng.integers(-lim, lim + 1, (N, D)).astype(np.float32), rng.integers(-lim, lim + 1, (K, D)).astype(np.float32))


def tie_case(N=3000, K=40, seed=7):
    """A small grid, coordinates in [-4, 4] at D = 3: many rows have two or more nearest centres at exactly equal distance."""
    return integer_case(N, K, 3, 4, seed)
