"""The output layer in closed form: float64 normal equations on the device (``irbfn_net_hidden``, ``irbfn_syrk_f64``).

With the centres and widths held fixed a ``WCRBFNet`` is linear in ``linear/kernel`` and ``linear/bias``, so the classical RBF
construction -- centres from clustering, then the output layer from linear least squares -- needs one pass over the table
where Adam needs thousands of epochs.  The reference has no counterpart (it trains these weights by Adam alone), so parity is
unpinned; what is pinned is each stage against a float64 statement of it (tests/_linear_fit_util.py).

    res = kmeans.fit(table.x, k=1000)
    w = widths.nearest_neighbour(res.centers, p=2).scaled(2.0)                     # or widths.select_scale for the multiplier
    net = WCRBFNet(..., centers=res.as_centers(net0), fixed_centers=True, fixed_width=True, log_sigs=w.log_sigs(net0))
    params, fit = linear_fit.fit_linear(net, net.init(), table.x, table.y)         # -> evaluate_table(net, params, table)

Without ``log_sigs=`` a fixed-width net runs at sigma = 1 in the units of the table's columns, whatever the centres.

One chunk of rows is one hidden-layer launch into Z = [h | 1 | y] and one float64 Gram launch G += Z^T Z; nothing synchronises
with the host until ``solve``.  G is accumulated in float64 because RBF design matrices are ill-conditioned and the normal
equations square the condition number; the products of float32 values are exact in float64, so G is the Gram matrix of the
kernel's own float32 hidden layer up to rows * 2^-53 relative per entry.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .model import NO_F64_HIDDEN, _grown_ws, _inner, _ptr, _stream_ptr, to_device_f32

_SYRK_WS: dict = {}


def _rows_f32(z, what: str, torch):
    """-> (z, ld): the float32 matrix argument ``what`` of a kernel that reads rows of any stride, and its leading dimension; a
    float32 cuda matrix with unit column stride is read in place, anything else goes through ``to_device_f32``."""
    if not isinstance(z, torch.Tensor) or not z.is_cuda or z.dtype != torch.float32 or z.dim() != 2 or (z.shape[0] > 1 and z.stride(1) != 1):
        z = to_device_f32(z, torch)
        if z.dim() != 2:
            raise ValueError(f"{what}, got {tuple(z.shape)}")
    rows, cols = z.shape
    return z, (z.stride(0) if rows > 1 else max(z.stride(0), cols))


def syrk(z, out=None, accumulate: bool = False):
    """z [rows, M] float32 on the device (rows may be strided: ``z.stride(0) >= M``) -> G = z^T z [M, M] float64, both
    triangles (``irbfn_syrk_f64``).  ``out``: a contiguous float64 [M, M] cuda tensor to write, or with ``accumulate`` to add onto."""
    torch = _lib.require_gpu()
    lib = _lib.load()
    z, ldz = _rows_f32(z, "syrk needs z [rows, M]", torch)
    rows, M = z.shape
    if out is None:
        if accumulate:
            raise ValueError("syrk: accumulate=True needs out=")
        out = torch.empty((M, M), dtype=torch.float64, device=z.device)
    elif tuple(out.shape) != (M, M) or out.dtype != torch.float64 or not out.is_cuda or not out.is_contiguous():
        raise ValueError(f"syrk: out must be a contiguous float64 cuda tensor of shape ({M}, {M})")
    ws = _grown_ws(_SYRK_WS, z.device.index, _lib.workspace_bytes("irbfn_syrk_f64_workspace_bytes", rows, M), torch, z.device)
    st = lib.irbfn_syrk_f64(_ptr(z), ldz, rows, M, _ptr(out), 1 if accumulate else 0, _ptr(ws), ws.numel(), _stream_ptr(torch))
    _lib.check(st, "irbfn_syrk_f64")
    return out


def _rows_of(net, x) -> int:
    """N of x [N, in_features]; any other shape raises."""
    xs = tuple(x.shape)
    if len(xs) != 2 or xs[1] != net.in_features:
        raise ValueError(f"x must have shape (N, {net.in_features}), got {xs}")
    return xs[0]


def hidden_rows(net, params, x, width: int, ones_col, batch_size: int, what: str, buf=None):
    """The one pass over the rows of x [N,D] that every closed-form stage makes -> (xd, Z, chunks).  ``chunks`` yields (i, n, Z[:n])
    per chunk of ``batch_size`` rows: ``irbfn_net_hidden`` of x[i:i + n] under ``params`` in the first K columns of the reused
    float32 buffer Z [chunk, width], 1 in column ``ones_col`` (None: no column is written); every other column is the caller's.
    ``xd`` = x on the device, where y can follow it; Z = ``buf`` where that has the rows and the device, else a new buffer.
    ``what`` names the caller where a float64 net is refused.  No host read."""
    torch = _lib.require_gpu()
    if getattr(net, "use_float64", False):
        raise ValueError(f"{what}: {NO_F64_HIDDEN}")
    N = _rows_of(net, x)
    if int(batch_size) < 1:
        raise ValueError("batch_size must be >= 1")
    net._warn_if_float64(params)
    net.bind(params)
    xd = to_device_f32(x, torch)
    chunk = min(int(batch_size), max(N, 1))
    if buf is None or buf.shape[0] < chunk or buf.device != xd.device:
        buf = torch.empty((chunk, int(width)), dtype=torch.float32, device=xd.device)

    def chunks():
        for i in range(0, N, chunk):
            n = min(chunk, N - i)
            Z = buf[:n]
            net._hidden_into(xd[i:i + n], Z, torch)
            if ones_col is not None:
                Z[:, ones_col] = 1.0
            yield i, n, Z
    return xd, buf, chunks()


class LinearFit:
    """The solution of ``NormalEquations.solve``: ``kernel`` [K,O] and ``bias`` [O] in float64 (on G's device), the number of
    rows ``n``, ``rss`` [O] = the residual sum of squares per output computed from G alone, ``mse`` = sum(rss) / (n O), and
    ``ridge_abs`` = the absolute ridge lambda that was added to the diagonal of H^T H; ``fit_bias`` as ``solve`` was called.
    ``sol`` = the stacked solution [W; b] ([W] without the ones column), the very tensor ``solve`` took ``rss`` from.  ``rss_of``
    prices it where it is there, so that for a fit made by ``solve`` ``rss_of`` on the solving accumulator equals ``rss`` bit for
    bit.  A ``LinearFit`` built by hand (``sol=None``) is stacked from ``kernel`` and ``bias``; the matrix product may then take
    another path and agree only to rounding."""

    def __init__(self, kernel, bias, n, rss, ridge_abs, fit_bias: bool = True, sol=None):
        self.kernel, self.bias, self.n, self.rss, self.ridge_abs = kernel, bias, n, rss, float(ridge_abs)
        self.fit_bias, self.sol = bool(fit_bias), sol

    @property
    def mse(self) -> float:
        return float(self.rss.sum().item()) / (max(self.n, 1) * max(self.rss.numel(), 1))


class NormalEquations:
    """G = Z^T Z in float64, Z = [h_0 .. h_{K-1}, 1, y_0 .. y_{O-1}] (M = K + 1 + O columns): H^T H, the column sums H^T 1, H^T Y,
    n = G[K,K], 1^T Y and Y^T Y at once.  ``add`` accumulates rows on the device; ``merge`` / ``all_reduce`` combine
    accumulators; ``solve`` returns the ridge-regularised least-squares output layer."""

    def __init__(self, net, G=None):
        if getattr(net, "use_float64", False):
            raise ValueError(f"NormalEquations: {NO_F64_HIDDEN}")
        self.net = net
        self.K, self.O = int(net.num_kernels), int(net.out_features)
        self.M = self.K + 1 + self.O
        if G is not None and (tuple(G.shape) != (self.M, self.M) or str(G.dtype) != "torch.float64"):
            raise ValueError(f"G must be a float64 tensor of shape ({self.M}, {self.M})")
        self.G = G
        self._Z = None

    def add(self, params: dict, x, y, batch_size: int = 65536) -> "NormalEquations":
        """Adds the rows (x [N,D], y [N,O]) under ``params``: per chunk of ``batch_size`` rows one ``irbfn_net_hidden`` into the
        reused buffer Z [chunk, M], the ones column and y by two slice assignments, then ``irbfn_syrk_f64(accumulate=1)``."""
        torch = _lib.require_gpu()
        K, O, M = self.K, self.O, self.M
        N, ys = _rows_of(self.net, x), tuple(y.shape)
        if len(ys) != 2 or ys[1] != O:
            raise ValueError(f"y must have shape (N, {O}), got {ys}")
        if N != ys[0]:
            raise ValueError(f"x has {N} rows, y has {ys[0]}")
        xd, self._Z, chunks = hidden_rows(self.net, params, x, M, K, batch_size, "NormalEquations", buf=self._Z)
        yd = to_device_f32(y, torch, device=xd.device)
        if self.G is None:
            self.G = torch.zeros((M, M), dtype=torch.float64, device=xd.device)
        for i, n, Z in chunks:
            Z[:, K + 1:] = yd[i:i + n]
            syrk(Z, out=self.G, accumulate=True)
        return self

    def merge(self, other: "NormalEquations") -> "NormalEquations":
        """Adds another accumulator of the same net shape (e.g. of another part of the table)."""
        if (other.K, other.O) != (self.K, self.O):
            raise ValueError(f"merge: accumulators of K={other.K}, O={other.O} and K={self.K}, O={self.O}")
        if other.G is not None:
            self.G = other.G.clone() if self.G is None else self.G + other.G.to(self.G.device)
        return self

    def subset(self, indices, net_k) -> "NormalEquations":
        """The accumulator of the sub-net ``net_k`` that keeps the kernels ``indices`` (in that order) of this one: the rows and
        columns [indices, K, K + 1 ...] of G, so that ``solve`` / ``rss_of`` give and price the fit of any selection without
        another pass over the rows (``ols.select``).  indices: an integer array or tensor of ``net_k.num_kernels`` entries."""
        import torch
        if self.G is None:
            raise ValueError("subset: no rows were added")
        idx = torch.as_tensor(indices).to(device=self.G.device, dtype=torch.long).reshape(-1)
        out = NormalEquations(net_k)
        if out.K != idx.numel() or out.O != self.O:
            raise ValueError(f"subset: {idx.numel()} indices and O={self.O} for a net of num_kernels={out.K}, out_features={out.O}")
        if idx.numel() and not bool(((idx >= 0) & (idx < self.K)).all().item()):
            raise ValueError(f"subset: indices outside [0, {self.K})")
        full = torch.cat([idx, torch.arange(self.K, self.M, device=idx.device)])
        out.G = self.G.index_select(0, full).index_select(1, full).contiguous()
        return out

    def all_reduce(self) -> "NormalEquations":
        """Sums G over the ranks when ``torch.distributed`` is initialised (identity otherwise), as ``ErrorStats.all_reduce``."""
        from . import distributed
        if distributed.is_dist() and self.G is not None:
            import torch.distributed as dist
            dist.all_reduce(self.G, op=dist.ReduceOp.SUM)
        return self

    def solve(self, ridge: float = 1e-8, fit_bias: bool = True) -> LinearFit:
        """(A + lambda diag(1, .., 1, 0)) [W; b] = [H^T Y; 1^T Y] with A = [[H^T H, H^T 1], [1^T H, n]] and
        lambda = ridge * trace(H^T H) / K (none on the bias), in float64 on G's device: symmetric Jacobi scaling by
        1 / sqrt(diag) (a zero diagonal entry is scaled by 1), ``torch.linalg.cholesky_ex``, two triangular solves.
        ``fit_bias=False`` drops the ones column and returns bias = 0.  O(K^3), once per fit."""
        return self._factorise(ridge, fit_bias)[2]

    def finite_G(self, what: str):
        """G, after the two refusals every consumer of it shares: no rows were added, or an entry is not finite (one host read)."""
        import torch
        if self.G is None:
            raise ValueError(f"{what}: no rows were added")
        bad = int((~torch.isfinite(self.G)).sum().item())
        if bad:
            raise ValueError(f"normal equations hold {bad} non-finite entries of {self.G.numel()} (non-finite rows in x or y?)")
        return self.G

    def ridge_abs(self, ridge: float) -> float:
        """The absolute ridge lambda = ridge * trace(H^T H) / K (one host read)."""
        import torch
        return float(ridge) * float(torch.diagonal(self.G)[:self.K].sum().item()) / self.K

    def _system(self, fit_bias: bool):
        """(A0 [m,m], rhs [m,O]) of G: [[H^T H, H^T 1], [1^T H, n]] and [H^T Y; 1^T Y], without the ones column m = K."""
        import torch
        G, K = self.G, self.K
        if fit_bias:
            return G[:K + 1, :K + 1], torch.cat([G[:K, K + 1:], G[K:K + 1, K + 1:]])
        return G[:K, :K], G[:K, K + 1:]

    def _factorise(self, ridge: float, fit_bias: bool):
        """``solve``, keeping what ``loo.factor`` builds on -> (L [m,m] the lower Cholesky factor of the scaled matrix
        diag(s) (A0 + Lambda) diag(s), s [m] the scaling, the ``LinearFit``)."""
        import torch
        G, K, O = self.finite_G("solve"), self.K, self.O
        n = int(round(float(G[K, K].item())))
        A0, rhs = self._system(fit_bias)
        m = A0.shape[0]
        lam = self.ridge_abs(ridge)
        A = A0.clone()
        torch.diagonal(A)[:K] += lam
        d = torch.diagonal(A)
        s = torch.where(d > 0, torch.rsqrt(torch.where(d > 0, d, torch.ones_like(d))), torch.ones_like(d))
        As = A * s[:, None] * s[None, :]
        try:
            L, info = torch.linalg.cholesky_ex(As)
        except RuntimeError:           # a torch build without the device factorisation: the O(K^3) step on the host
            L, info = (t.to(As.device) for t in torch.linalg.cholesky_ex(As.cpu()))
        # the scaled matrix has a unit diagonal: a pivot below m 2^-52 is rounding noise of a singular system
        if int(info.item()) != 0 or not bool((torch.diagonal(L) ** 2 > m * 2.0 ** -52).all().item()):
            raise ValueError(f"normal equations not positive definite at ridge={ridge:g}; raise ridge")
        t = torch.linalg.solve_triangular(L, rhs * s[:, None], upper=False)
        sol = torch.linalg.solve_triangular(L.mT, t, upper=True) * s[:, None]
        W = sol[:K].contiguous()
        b = sol[K].contiguous() if fit_bias else torch.zeros(O, dtype=G.dtype, device=G.device)
        return L, s, LinearFit(W, b, n, self._rss(sol, fit_bias), lam, fit_bias, sol)

    def _rss(self, sol, fit_bias: bool):
        """y^T y - 2 sol^T rhs + sol^T A0 sol per output, clamped at 0: the residual sum of squares of sol = [W; b] ([W] without
        the ones column) on this accumulator's rows, from G alone."""
        import torch
        A0, rhs = self._system(fit_bias)
        yty = torch.diagonal(self.G)[self.K + 1:]
        return (yty - 2.0 * (sol * rhs).sum(0) + (sol * (A0 @ sol)).sum(0)).clamp_min(0.0)

    def rss_of(self, fit: LinearFit):
        """The residual sum of squares per output [O] of a given ``LinearFit`` on this accumulator's rows, from G alone (no pass
        over the rows): how a fit solved on one part of a table is priced on another.  On the accumulator the fit was solved on
        it is ``fit.rss``."""
        import torch
        if self.G is None:
            raise ValueError("rss_of: no rows were added")
        if tuple(fit.kernel.shape) != (self.K, self.O):
            raise ValueError(f"rss_of: a fit of shape {tuple(fit.kernel.shape)} on an accumulator of K={self.K}, O={self.O}")
        if fit.sol is not None:            # the very tensor solve priced: the matrix product then takes the same path, bit for bit
            return self._rss(fit.sol.to(device=self.G.device, dtype=self.G.dtype), fit.fit_bias)
        W = fit.kernel.to(device=self.G.device, dtype=self.G.dtype)
        b = fit.bias.to(device=self.G.device, dtype=self.G.dtype)
        return self._rss(torch.cat([W, b[None]]) if fit.fit_bias else W, fit.fit_bias)


def _like_leaf(t64, old):
    """The float32 leaf that replaces ``old``: a torch tensor on old's device, else a NumPy array."""
    import torch
    if isinstance(old, torch.Tensor):
        return t64.to(device=old.device, dtype=torch.float32)
    return t64.detach().cpu().numpy().astype(np.float32)


def with_fit(params: dict, fit: LinearFit) -> dict:
    """The tree of ``params`` (with its ``{"params": ...}`` wrapper or without) with ``linear/kernel`` and ``linear/bias`` from the
    fit, cast to float32 in the flavour of the leaves they replace; every other leaf is the input's own, the groups are new dicts
    and ``params`` is left as it was."""
    p = _inner(params)
    new = {g: dict(v) for g, v in p.items()}
    new["linear"]["kernel"] = _like_leaf(fit.kernel, p["linear"]["kernel"])
    new["linear"]["bias"] = _like_leaf(fit.bias, p["linear"]["bias"])
    return {"params": new} if "params" in params else new


def fit_linear(net, params: dict, x, y, ridge: float = 1e-8, fit_bias: bool = True, batch_size: int = 65536):
    """-> (new_params, LinearFit): ``linear/kernel`` and ``linear/bias`` of ``params`` replaced by the ridge least-squares fit
    of y [N,O] on the net's hidden layer of x [N,D] (centres, widths and gate as in ``params`` / the net), cast to float32;
    every other leaf and the tree's shape are the input's, so a fixed-centre or fixed-width net gets its reduced tree back.
    x, y: arrays or tensors on any device (a ``DeviceTable``'s ``.x``, ``.y``)."""
    fit = NormalEquations(net).add(params, x, y, batch_size=batch_size).solve(ridge=ridge, fit_bias=fit_bias)
    return with_fit(params, fit), fit
