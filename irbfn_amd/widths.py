"""RBF widths from the data: the p nearest centres of every row on the device (``irbfn_knn_d2``, include/irbfn_hip.h), the two
classical width rules on top of it, and the search for their one multiplier on held-out rows.

The stage between ``kmeans.fit`` (the centres) and ``linear_fit.fit_linear`` (the output layer).  The reference leaves the widths
to Adam from ``log_sigs = 0`` and has no width rule, so parity is unpinned; what is pinned is each stage against a float64
statement of it (tests/_widths_util.py).  ``log_sigs = 0`` is sigma = 1 in the units of the table's columns, whatever the centres.

    res = kmeans.fit(table.x, k=1000)
    w = widths.nearest_neighbour(res.centers, p=2)                # sigma_k from the 2 nearest other centres
    net = WCRBFNet(..., centers=res.as_centers(net0), fixed_centers=True, fixed_width=True)
    search = widths.select_scale(net, w, table.x, table.y)        # -> search.net, search.params, search.fit, search.best

Convention: the layer computes phi(|x - c| / sigma) with sigma = exp(log_sig), so for ``gaussian`` phi = exp(-|x - c|^2 / sigma^2)
(no factor 2): a centre's nearest neighbour at distance sigma sees phi = 1 / e.
"""
from __future__ import annotations

import numpy as np

from . import _lib, kmeans
from .linear_fit import NormalEquations, with_fit
from .model import _grown_ws, _ptr, _stream_ptr, to_device_f32

_KNN_WS: dict = {}


def knn(q, c, p: int, exclude_self: bool = False, row0: int = 0, split: int = 0):
    """q [N,D], c [K,D] -> (d2 [N,p] float32, idx [N,p] int32) on the device: per row the p smallest squared distances in
    ascending order of (d2, index) and their centres; slots without a candidate hold NaN / -1 (``irbfn_knn_d2``).
    ``exclude_self``: q is rows ``row0 .. row0 + N - 1`` of c and row n never takes centre ``row0 + n``.  ``split``: 0 = the
    library cuts the centres into segments as it sees fit, s >= 1 = s segments; the result does not depend on it."""
    torch = _lib.require_gpu()
    lib = _lib.load()
    qd = to_device_f32(q, torch)
    cd = to_device_f32(c, torch, device=qd.device)
    if qd.dim() != 2 or cd.dim() != 2 or cd.shape[1] != qd.shape[1] or cd.shape[0] < 1:
        raise ValueError(f"knn needs q [N,D] and c [K,D], got {tuple(qd.shape)} / {tuple(cd.shape)}")
    p, row0, split = int(p), int(row0), int(split)
    if row0 < 0:
        raise ValueError("row0 must be >= 0")
    N, D = qd.shape
    K = cd.shape[0]
    need = _lib.workspace_bytes("irbfn_knn_workspace_bytes", N, K, D, p, split)
    d2 = torch.empty((N, p), dtype=torch.float32, device=qd.device)
    idx = torch.empty((N, p), dtype=torch.int32, device=qd.device)
    ws = _grown_ws(_KNN_WS, qd.device.index, need, torch, qd.device)
    st = lib.irbfn_knn_d2(_ptr(qd), _ptr(cd), N, K, D, p, row0 if exclude_self else -1, split, _ptr(d2), _ptr(idx), _ptr(ws),
                          ws.numel(), _stream_ptr(torch))
    _lib.check(st, "irbfn_knn_d2")
    return d2, idx


class Widths:
    """``sigma`` [K] float32 on the device, all finite and positive; ``replaced`` = how many of them the rule could not give (0 or
    non-finite) and the median of the others stands in for."""

    def __init__(self, sigma, replaced: int = 0):
        self.sigma, self.replaced = sigma, int(replaced)

    def scaled(self, s: float) -> "Widths":
        """The widths times s."""
        return Widths(self.sigma * float(s), self.replaced)

    def log_sigs(self, net) -> np.ndarray:
        """[R,K] float32 (the same widths in every region, as ``KMeansResult.as_centers``): what
        ``WCRBFNet(centers=..., fixed_width=True, log_sigs=...)`` takes, and the ``rbf_list/log_sigs`` leaf of a trainable tree.
        The layer computes phi(|x - c| / sigma) with sigma = exp(log_sig); for ``gaussian`` phi = exp(-|x - c|^2 / sigma^2)."""
        K = self.sigma.shape[0]
        if self.sigma.dim() != 1 or K != net.num_kernels:
            raise ValueError(f"{K} widths do not fit a net of num_kernels={net.num_kernels}")
        ls = np.log(self.sigma.detach().cpu().numpy().astype(np.float64)).astype(np.float32)
        return np.ascontiguousarray(np.broadcast_to(ls, (net.num_regions, K)))


def _finish(sigma64, scale, what) -> Widths:
    """float64 sigma [K] before the scale -> Widths: a sigma that is 0 or non-finite becomes the median of the finite positive
    ones (the mean of the two middle ones for an even number).  One host read: the number of good ones."""
    torch = _lib.require_gpu()
    K = sigma64.shape[0]
    good = torch.isfinite(sigma64) & (sigma64 > 0)
    n = int(good.sum().item())
    if n == 0:
        raise ValueError(f"{what}: no centre has a finite positive width (duplicate centres, one-row clusters or K = 1)")
    v = torch.sort(torch.where(good, sigma64, torch.full_like(sigma64, float("inf")))).values
    med = 0.5 * (v[(n - 1) // 2] + v[n // 2])
    sigma = torch.where(good, sigma64, med) * float(scale)
    return Widths(sigma.to(torch.float32), K - n)


def nearest_neighbour(centers, p: int = 2, scale: float = 1.0) -> Widths:
    """sigma_k = scale * sqrt(mean of the filled slots of the squared distances to the p nearest *other* centres): the
    p-nearest-neighbour heuristic of Moody & Darken (1989).  The distances are the kernel's float32 chain; the mean is taken in
    float64 on the device.  A centre with a bit-for-bit duplicate has a neighbour at distance 0 like any other; a sigma of 0 or
    without a filled slot is degenerate (``Widths``)."""
    torch = _lib.require_gpu()
    cd = to_device_f32(centers, torch)
    if cd.dim() != 2:
        raise ValueError(f"nearest_neighbour needs centers [K,D], got {tuple(cd.shape)}")
    d2, _ = knn(cd, cd, p, exclude_self=True)
    filled = torch.isfinite(d2)
    total = torch.where(filled, d2.to(torch.float64), torch.zeros((), dtype=torch.float64, device=cd.device)).sum(dim=1)
    return _finish(torch.sqrt(total / filled.sum(dim=1)), scale, "nearest_neighbour")        # no filled slot: 0 / 0 = NaN


def cluster_sums(values64, labels, K: int):
    """(sums float64 [K], counts int64 [K]) of the non-negative values64 [N] by labels [N] (-1 = in no cluster), bit-identical
    across repeats because every sum is an exact integer sum, as the cells of ``irbfn_kmeans_step``: with max v < 2^e and
    N < 2^L a row adds q = rint(v 2^(S - e)), S = 62 - L, so no sum leaves int64 in any order and integer addition has no
    order.  The rows are sorted by label, the q summed by one int64 running sum and the clusters taken as differences at
    their ends (a floating-point ``torch.cumsum`` combines its tiles in an order that depends on timing; an integer one
    cannot differ).  |sum - exact| <= count 2^(e - S - 1) <= count 2^-S max v, then one float64 rounding: 2^-42 of the largest
    value per row at N = 2^20.  No host read; torch operations only, on the tensors' device."""
    import torch
    lab = labels.to(torch.int64)
    N = lab.shape[0]
    if N == 0:
        return torch.zeros(K, dtype=torch.float64, device=lab.device), torch.zeros(K, dtype=torch.int64, device=lab.device)
    valid = lab >= 0
    v = torch.where(valid, values64, torch.zeros_like(values64))
    S = 62 - int(N).bit_length()                                       # N < 2^L with L = bit_length(N)
    e = torch.frexp(v.max())[1].to(torch.int64)                        # max v = m 2^e with m in [0.5, 1): max v < 2^e (0 for 0)
    pow2 = lambda p: ((p + 1023) << 52).view(torch.float64)            # 2^p exactly, from its bits (|p| < 1023 for float32 values)
    q = torch.round(v * pow2(S - e)).to(torch.int64)
    key = torch.where(valid, lab, torch.full_like(lab, K))
    order = torch.sort(key, stable=True).indices
    run = torch.cumsum(q[order], 0)
    counts = torch.bincount(key, minlength=K + 1)[:K]
    ends = torch.cumsum(counts, 0)
    run0 = torch.cat([torch.zeros(1, dtype=run.dtype, device=run.device), run])      # run0[i] = the sum of the first i sorted rows
    return (run0[ends] - run0[ends - counts]).to(torch.float64) * pow2(e - S), counts


def cluster_spread(x, centers, scale: float = 1.0, min_count: int = 2) -> Widths:
    """sigma_k = scale * the RMS distance of the rows that ``kmeans.assign`` gives to centre k (exact integer sums of the
    kernel's float32 d2 on a fixed-point grid, ``cluster_sums``: bit-identical across repeats).  A cluster with fewer than ``min_count`` rows is degenerate (``Widths``)."""
    torch = _lib.require_gpu()
    labels, d2 = kmeans.assign(x, centers)
    K = to_device_f32(centers, torch).shape[0]
    sums, counts = cluster_sums(d2.to(torch.float64), labels, K)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=sums.device)
    return _finish(torch.where(counts >= int(min_count), torch.sqrt(sums / counts), nan), scale, "cluster_spread")


class ScaleSearch:
    """``scales``; ``train_mse`` / ``holdout_mse`` per scale (``inf`` where the system was not positive definite); ``best`` = the
    index of the smallest held-out MSE; ``net``, ``params``, ``fit`` = the best scale's net, its tree and its ``LinearFit``."""

    def __init__(self, scales, train_mse, holdout_mse, best, net, params, fit):
        self.scales, self.train_mse, self.holdout_mse = tuple(scales), list(train_mse), list(holdout_mse)
        self.best, self.net, self.params, self.fit = int(best), net, params, fit

    @property
    def best_scale(self) -> float:
        return self.scales[self.best]


def finite_lists(t):
    """A device tensor of errors as nested host lists, NaN and +inf both as ``inf`` (one host read)."""
    import torch
    return torch.nan_to_num(t, nan=float("inf"), posinf=float("inf")).tolist()


def search_scales(net, widths: Widths, x, y, scales, batch_size: int, price, what: str) -> ScaleSearch:
    """The search of this module's ``select_scale`` and of ``loo.select_scale``.  x [n,D], y [n,O]: the rows every scale is fitted
    on, float32 on the device.  Per scale s: net_s, its ``init()`` tree p, ``ne = NormalEquations(net_s).add(p, x, y)`` (a wrong
    shape of x or y raises there) and ``price(net_s, p, ne) -> (LinearFit, second error)``, the error a float64 device scalar;
    a ``ValueError`` from ``price`` (a system ``solve`` refuses) puts the scale out with ``inf`` for both errors.  ``train_mse`` =
    rss / (n O) of the fit, ``holdout_mse`` = the second error, which ``what`` names where no scale has a finite one.  Host
    reads: those of ``price``, the widths once before the first scale (``log_sigs`` is a host array; the scales are applied to
    the host copy) and one read of both paths at the end."""
    torch = _lib.require_gpu()
    if not (net.fixed_width and net.centers is not None):
        raise ValueError("select_scale needs a fixed-width net: WCRBFNet(..., centers=C, fixed_width=True)")
    scales = tuple(float(s) for s in scales)
    if not scales:
        raise ValueError("select_scale needs at least one scale")
    inf = torch.full((), float("inf"), dtype=torch.float64, device=x.device)
    tried, mse_t, mse_x = [], [], []
    host = Widths(widths.sigma.detach().cpu(), widths.replaced)      # the one read of the widths
    for s in scales:
        net_s = type(net).from_config(dict(net.config(), log_sigs=host.scaled(s).log_sigs(net)), centers=net.centers)
        p = net_s.init()
        ne = NormalEquations(net_s).add(p, x, y, batch_size=batch_size)
        try:
            fit, second = price(net_s, p, ne)
        except ValueError:             # not positive definite, or non-finite entries: this scale is out
            fit, second = None, inf
        tried.append((net_s, fit))
        mse_t.append(inf if fit is None else fit.rss.sum() / (x.shape[0] * net.out_features))
        mse_x.append(second)
    both = finite_lists(torch.stack([torch.stack(mse_t), torch.stack(mse_x)]))
    best = int(np.argmin(both[1]))
    net_b, fit_b = tried[best]
    if fit_b is None or not np.isfinite(both[1][best]):
        raise ValueError(f"select_scale: no scale gave a positive definite system with a finite {what}")
    return ScaleSearch(scales, both[0], both[1], best, net_b, with_fit(net_b.init(), fit_b), fit_b)


def select_scale(net, widths: Widths, x, y, scales=(0.5, 1, 2, 4, 8), holdout_every: int = 5, ridge: float = 1e-8,
                 batch_size: int = 65536) -> ScaleSearch:
    """The multiplier of a width rule from held-out rows.  net: a fixed-width ``WCRBFNet`` with ``centers=``.  For every scale s
    the same net with ``log_sigs = widths.scaled(s).log_sigs(net)``, one ``NormalEquations`` over the rows with
    index % holdout_every != 0 and one over the rest; the first is solved, and the solution is priced on the second from its Gram
    matrix alone (``NormalEquations.rss_of``): no second pass over the held-out rows.  The search, its host reads (here those of
    ``solve`` per scale) and its refusals are ``search_scales``'."""
    torch = _lib.require_gpu()
    holdout_every = int(holdout_every)
    if holdout_every < 2:
        raise ValueError("select_scale needs holdout_every >= 2")
    xd = to_device_f32(x, torch)
    yd = to_device_f32(y, torch, device=xd.device)
    N = xd.shape[0]
    rows = np.arange(N)
    tr = torch.from_numpy(rows[rows % holdout_every != 0]).to(xd.device)
    ho = torch.from_numpy(rows[rows % holdout_every == 0]).to(xd.device)
    if tr.numel() == 0 or ho.numel() == 0:
        raise ValueError(f"{N} rows leave nothing to fit on or to hold out at holdout_every={holdout_every}")
    xh, yh = xd[ho], yd[ho]

    def held_out(net_s, p, train):
        fit = train.solve(ridge=ridge)               # a refused scale ends here: no pass over its held-out rows
        held = NormalEquations(net_s).add(p, xh, yh, batch_size=batch_size)
        return fit, held.rss_of(fit).sum() / (ho.numel() * net.out_features)
    return search_scales(net, widths, xd[tr], yd[tr], scales, batch_size, held_out, "held-out error")
