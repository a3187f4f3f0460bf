"""k-means on the device: centres and cluster labels from a table (``irbfn_kmeans_step``, include/irbfn_hip.h).

The reference derives the centres of its warm-start / fixed-centre / fixed-width nets ("constraint clustering -> centre
files") and the ``cluster_ids`` of ``train_step_fullint_withcluster`` in notebooks; neither the
notebooks nor the centre files are in its snapshot (VERDICT, missing #3), so parity with its clustering is unpinned.  What
is pinned is one Lloyd iteration against a float64 statement of it (tests/_kmeans_util.py).

    res = kmeans.fit(table_inputs, k=1000)                       # plain Lloyd, k-means++ start
    net = WCRBFNet(..., centers=res.as_centers(net0), fixed_centers=True)
    w = widths.nearest_neighbour(res.centers, p=2)               # the widths from the centres: w.log_sigs(net) is the log_sigs leaf
    table = tables.DeviceTable(inputs, outputs, labels=res.labels, num_classes=500)   # -> train_epoch(ClusterTrainState)

One iteration is one library call that reads the rows once (nearest centre, the per-cluster sums and counts, the step
statistics); nothing synchronises with the host inside ``fit`` unless ``check_every > 0``.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .model import _ptr, _stream_ptr, to_device_f32

STATS = ("finite", "inertia", "moved", "max_shift2")      # the four float64 values of one iteration


def _step(lib, torch, x, centers, labels, d2, new_centers, counts, stats, ws):
    N, D = x.shape
    st = lib.irbfn_kmeans_step(_ptr(x), _ptr(centers), _ptr(labels), _ptr(d2) if d2 is not None else None,
                               _ptr(new_centers) if new_centers is not None else None,
                               _ptr(counts) if counts is not None else None, _ptr(stats), N, centers.shape[0], D,
                               _ptr(ws), ws.numel(), _stream_ptr(torch))
    _lib.check(st, "irbfn_kmeans_step")


def _workspace(torch, N, K, D, device):
    return torch.empty(max(_lib.workspace_bytes("irbfn_kmeans_workspace_bytes", N, K, D), 8), dtype=torch.uint8, device=device)


def _rows_and_centers(x, centers, torch):
    xd = to_device_f32(x, torch)
    cd = to_device_f32(centers, torch, device=xd.device)
    if xd.dim() != 2 or cd.dim() != 2 or cd.shape[1] != xd.shape[1] or cd.shape[0] < 1:
        raise ValueError(f"k-means needs x [N,D] and centers [K,D], got {tuple(xd.shape)} / {tuple(cd.shape)}")
    return xd, cd


def assign(x, centers):
    """-> (labels int32 [N], d2 float32 [N]) on the device: the nearest centre of every row (ties to the lowest index) and the
    squared distance to it; a row without a finite distance gets -1 / NaN."""
    torch = _lib.require_gpu()
    lib = _lib.load()
    xd, cd = _rows_and_centers(x, centers, torch)
    N, D = xd.shape
    labels = torch.full((N,), -1, dtype=torch.int32, device=xd.device)
    d2 = torch.empty(N, dtype=torch.float32, device=xd.device)
    if N:
        stats = torch.empty(4, dtype=torch.float64, device=xd.device)
        _step(lib, torch, xd, cd, labels, d2, None, None, stats, _workspace(torch, N, cd.shape[0], D, xd.device))
    return labels, d2


class KMeansResult:
    """``centers`` [k,D] float32, ``labels`` [N] int32, ``counts`` [k] int64, ``history`` [n_iter,4] float64 (per iteration:
    ``STATS``), all on the device; ``n_iter``.  Labels, counts and inertia are those of the last iteration's assignment;
    ``centers`` are the means of exactly those labels (an empty cluster keeps its previous centre).  Once an iteration
    moved no row, both describe the same fixed point."""

    def __init__(self, centers, labels, counts, history, n_iter):
        self.centers, self.labels, self.counts, self.history, self.n_iter = centers, labels, counts, history, int(n_iter)

    @property
    def inertia(self) -> float:
        """Sum of the squared distances of the last assignment (one host read)."""
        return float(self.history[self.n_iter - 1, 1].item()) if self.n_iter else float("nan")

    def as_centers(self, net) -> np.ndarray:
        """[K,D] float32 as ``WCRBFNet(centers=...)`` takes it (the same centres in every region)."""
        k, D = self.centers.shape
        if k != net.num_kernels or D != net.in_features:
            raise ValueError(f"{k} centres of {D} columns do not fit a net of num_kernels={net.num_kernels}, "
                             f"in_features={net.in_features}")
        return self.centers.detach().cpu().numpy().copy()


def _finite_first(xd, gen, torch):
    """A random permutation of the row indices with the finite rows first, and their number (a device scalar)."""
    fin = torch.isfinite(xd).all(dim=1)
    perm = torch.randperm(xd.shape[0], device=xd.device, generator=gen)
    order = perm[torch.sort((~fin[perm]).to(torch.int8), stable=True).indices]
    return order, fin.sum()


def init_random(xd, k, gen):
    """k distinct finite rows, drawn with ``torch.randperm``."""
    torch = _lib.require_gpu()
    order, _ = _finite_first(xd, gen, torch)
    return xd.index_select(0, order[:k])


def init_kmeanspp(xd, k, gen):
    """D^2 sampling (Arthur & Vassilvitskii 2007) on the device, no host synchronisation per centre: ``assign`` against the
    newest centre -> running minimum -> float64 cumulative sum -> ``searchsorted`` of one uniform draw (``torch.multinomial``
    stops at 2^24 categories).  A row at distance 0 from a chosen centre, and a non-finite row, has weight 0 and is never
    drawn while any weight is positive; with none left the first centre is repeated."""
    torch = _lib.require_gpu()
    lib = _lib.load()
    N, D = xd.shape
    order, _ = _finite_first(xd, gen, torch)
    first = order[:1]
    centers = torch.empty((k, D), dtype=torch.float32, device=xd.device)
    centers[0:1] = xd.index_select(0, first)
    ws = _workspace(torch, N, 1, D, xd.device)
    labels = torch.full((N,), -1, dtype=torch.int32, device=xd.device)
    d2 = torch.empty(N, dtype=torch.float32, device=xd.device)
    stats = torch.empty(4, dtype=torch.float64, device=xd.device)
    mind = torch.full((N,), float("inf"), dtype=torch.float32, device=xd.device)
    u = torch.rand(max(k - 1, 1), dtype=torch.float64, device=xd.device, generator=gen)
    zero = torch.zeros((), dtype=torch.float64, device=xd.device)
    for i in range(1, k):
        _step(lib, torch, xd, centers[i - 1:i], labels, d2, None, None, stats, ws)
        mind = torch.minimum(mind, torch.nan_to_num(d2, nan=0.0, posinf=0.0))          # a row without a finite distance: weight 0
        cs = torch.cumsum(mind.to(torch.float64), 0)
        total = cs[-1]
        t = torch.minimum(u[i - 1] * total, torch.nextafter(total, zero))              # stay below the total: an index < N
        idx = torch.searchsorted(cs, t.reshape(1), right=True).clamp_(max=N - 1)
        idx = torch.where(total > 0, idx, first)
        centers[i:i + 1] = xd.index_select(0, idx)
    return centers


def fit(x, k: int, max_iter: int = 100, init="kmeans++", seed: int = 0, tol: float = 0.0, check_every: int = 0) -> KMeansResult:
    """Lloyd's algorithm on x [N,D] (1 <= D <= 16, 1 <= k <= 65536).  init: "kmeans++", "random" or an array [k,D].
    check_every = m > 0: every m-th iteration reads its statistics and the loop stops when no row moved or the largest
    squared shift of a centre is <= tol; with 0 the loop runs max_iter iterations without touching the host."""
    torch = _lib.require_gpu()
    lib = _lib.load()
    xd = to_device_f32(x, torch)
    if xd.dim() != 2:
        raise ValueError(f"fit needs x [N,D], got {tuple(xd.shape)}")
    N, D = xd.shape
    k = int(k)
    if k < 1 or N < 1 or max_iter < 0:
        raise ValueError("fit needs k >= 1, at least one row and max_iter >= 0")
    gen = torch.Generator(device=xd.device)
    gen.manual_seed(int(seed))
    if isinstance(init, str):
        if init not in ("kmeans++", "random"):
            raise ValueError('init must be "kmeans++", "random" or an array [k,D]')
        n_fin = int(torch.isfinite(xd).all(dim=1).sum().item())          # the one host read of the initialisation
        if n_fin < k:
            raise ValueError(f"{n_fin} finite rows cannot seed {k} centres")
        cur = (init_kmeanspp if init == "kmeans++" else init_random)(xd, k, gen)
    else:
        cur = to_device_f32(init, torch, device=xd.device).clone()
        if tuple(cur.shape) != (k, D):
            raise ValueError(f"init has shape {tuple(cur.shape)}, expected ({k}, {D})")
    ws = _workspace(torch, N, k, D, xd.device)
    nxt = torch.empty_like(cur)
    labels = torch.full((N,), -1, dtype=torch.int32, device=xd.device)
    counts = torch.zeros(k, dtype=torch.int64, device=xd.device)
    history = torch.zeros((max(max_iter, 1), 4), dtype=torch.float64, device=xd.device)
    n_iter = 0
    for i in range(max_iter):
        _step(lib, torch, xd, cur, labels, None, nxt, counts, history[i], ws)
        cur, nxt = nxt, cur
        n_iter = i + 1
        if check_every > 0 and n_iter % check_every == 0:
            _, _, moved, shift2 = history[i].tolist()
            if moved == 0 or shift2 <= tol:
                break
    return KMeansResult(cur, labels, counts, history[:n_iter], n_iter)
