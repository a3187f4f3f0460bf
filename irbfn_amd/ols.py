"""Centres chosen by what they explain: orthogonal least squares forward selection on the device (``irbfn_ols_begin`` /
``irbfn_ols_steps``, include/irbfn_hip.h).

k-means puts centres where the rows are dense, not where the target is hard.  Forward selection (Chen, Cowan & Grant 1991) takes,
from a pool of M candidate centres, again and again the one whose hidden-layer column removes the most of what is still unexplained
in y.  It needs nothing but the Gram matrix a ``NormalEquations`` of the pool net already holds: it is a Cholesky factorisation of
H^T H + lambda I whose pivot is the largest drop of the residual.  The reference has no counterpart: parity is unpinned; the
arithmetic is pinned against a float64 statement of it (tests/_ols_util.py).

    pool = kmeans.fit(table.x, k=512)
    w = widths.nearest_neighbour(pool.centers, p=2).scaled(4.0)
    net = WCRBFNet(..., num_kernels=512, centers=pool.as_centers(net0), fixed_width=True, log_sigs=w.log_sigs(net0))
    net64, params64, fit, res = ols.fit_ols(net, net.init(), table.x, table.y, k=64)      # res.objective: the whole path

Selection is by kernel index: ``linear/kernel`` is shared over the regions of a gated net, so the k-th centres of all regions enter
or leave together.  ``k`` pivots are two launches each and no host read, unless ``check_every > 0``.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .linear_fit import NormalEquations, with_fit
from .model import NO_F64_HIDDEN, WCRBFNet, _inner, _ptr, _stream_ptr


def npad(M: int) -> int:
    """The row length of the factor and the state vectors: M + 1 rounded up to a multiple of 64."""
    return (int(M) + 1 + 63) // 64 * 64


def default_tol(M: int, fit_bias: bool = True) -> float:
    """n 2^-52 with n = the number of columns: the pivot test of ``NormalEquations.solve`` (d / d0 is the pivot of the
    unit-diagonal matrix)."""
    return (int(M) + (1 if fit_bias else 0)) * 2.0 ** -52


class OLSResult:
    """What ``select`` found.  ``indices`` int32 [n_selected] on the device, in the order of selection (the ones column excluded);
    ``n_selected`` (< k when the pool ran out of independent columns, or ``min_gain`` stopped the run); ``gain`` [n_selected, O] =
    the drop of the objective per output at each pivot; ``objective`` [n_selected + 1, O] = the least of rss + ridge_abs |w|^2 over
    the weights of the first t centres (row 0: after the ones column alone, or y^T y without ``fit_bias``); ``ridge_abs`` = the
    absolute lambda on the diagonal of H^T H; ``ridge`` / ``fit_bias`` as ``select`` was called."""

    def __init__(self, ne, indices, gain, objective, ridge, ridge_abs, fit_bias):
        self.ne, self.indices, self.gain, self.objective = ne, indices, gain, objective
        self.n_selected = int(indices.numel())
        self.ridge, self.ridge_abs, self.fit_bias = float(ridge), float(ridge_abs), bool(fit_bias)

    def subnet(self, net, params: dict, k: int | None = None):
        """-> (net_k, params_k, LinearFit): the ``WCRBFNet`` of ``num_kernels = k`` that keeps the kernel indices
        ``indices[:k]`` in every region, its tree (``centers[:, idx]``, ``log_sigs[:, idx]``, ``kernel[idx]`` sliced; the constants
        of a fixed-centre or fixed-width net are sliced in the net and its reduced tree is returned) with the linear leaves
        from ``ne.subset(idx, net_k).solve(ridge, fit_bias)``, and that fit."""
        k = self.n_selected if k is None else int(k)
        if not 1 <= k <= self.n_selected:
            raise ValueError(f"subnet: k = {k} of {self.n_selected} selected centres")
        idx = self.indices[:k]
        net_k, new = slice_net(net, params, idx.cpu().numpy())
        fit = self.ne.subset(idx, net_k).solve(ridge=self.ridge, fit_bias=self.fit_bias)
        return net_k, with_fit({"params": new} if "params" in params else new, fit), fit      # slice_net keeps the leaves' flavour


def _take(leaf, idx: np.ndarray, axis: int):
    """Entries ``idx`` of a NumPy or torch leaf along ``axis``."""
    if hasattr(leaf, "index_select"):
        import torch
        return leaf.index_select(axis, torch.as_tensor(idx, dtype=torch.long, device=leaf.device)).contiguous()
    return np.ascontiguousarray(np.take(np.asarray(leaf), idx, axis=axis))


def slice_net(net, params: dict, idx):
    """-> (net_k, tree_k): the net that keeps the kernel indices ``idx`` (in that order) of every region, and the inner tree of
    ``params`` sliced alike (``linear/bias`` as it is).  One-region and tanh-gated multi-region ``WCRBFNet`` only."""
    if type(net) is not WCRBFNet:
        raise ValueError(f"selection of centres is built for WCRBFNet, not {type(net).__name__}")
    if net.use_float64:
        raise ValueError(f"NormalEquations: {NO_F64_HIDDEN}")
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    if idx.size < 1 or idx.min() < 0 or idx.max() >= net.num_kernels:
        raise ValueError(f"kernel indices must be a non-empty subset of [0, {net.num_kernels})")
    p = _inner(params)
    net._check_shapes(p)
    cfg = dict(net.config(), num_kernels=int(idx.size))
    if net.log_sigs is not None:
        cfg["log_sigs"] = net.log_sigs[:, idx]
    net_k = WCRBFNet.from_config(cfg, centers=None if net.centers is None else net.centers[:, idx])
    new = {g: dict(v) for g, v in p.items()}
    for name in ("centers", "log_sigs"):
        if name in new.get("rbf_list", {}):
            new["rbf_list"][name] = _take(new["rbf_list"][name], idx, 1)
    new["linear"]["kernel"] = _take(new["linear"]["kernel"], idx, 0)
    return net_k, new


class _State:
    """The device buffers of one selection (the layout of include/irbfn_hip.h) and the two library calls."""

    def __init__(self, G, M, O, fit_bias, ridge_abs, tol, kmax, torch, lib):
        dev = G.device
        self.args = (M, O, 1 if fit_bias else 0)
        self.G, self.tol, self.kmax, self.lib, self.torch = G, float(tol), int(kmax), lib, torch
        n = npad(M)
        self.L = torch.zeros((kmax + 1, n), dtype=torch.float64, device=dev)
        self.d = torch.zeros((2, n), dtype=torch.float64, device=dev)
        self.c = torch.zeros((n, O), dtype=torch.float64, device=dev)
        self.sel = torch.full((kmax + 1,), -1, dtype=torch.int32, device=dev)
        self.gain = torch.zeros((kmax + 1, O), dtype=torch.float64, device=dev)
        self.count = torch.zeros(1, dtype=torch.int32, device=dev)
        self.ws = torch.empty(_lib.workspace_bytes("irbfn_ols_workspace_bytes", M, O, kmax), dtype=torch.uint8, device=dev)
        st = lib.irbfn_ols_begin(_ptr(G), M, O, self.args[2], float(ridge_abs), self.tol, self.kmax, *self._bufs(), _stream_ptr(torch))
        _lib.check(st, "irbfn_ols_begin")

    def _bufs(self):
        return (_ptr(self.L), _ptr(self.d), _ptr(self.c), _ptr(self.sel), _ptr(self.gain), _ptr(self.count), _ptr(self.ws),
                self.ws.numel())

    def steps(self, steps: int):
        M, O, fb = self.args
        st = self.lib.irbfn_ols_steps(_ptr(self.G), M, O, fb, self.tol, self.kmax, *self._bufs(), int(steps), _stream_ptr(self.torch))
        _lib.check(st, "irbfn_ols_steps")


def select(ne: NormalEquations, k: int, ridge: float = 1e-8, fit_bias: bool = True, tol: float | None = None, check_every: int = 0,
           min_gain: float = 0.0) -> OLSResult:
    """Forward selection of ``k`` of the ``ne.K`` candidate kernels on an accumulator whose rows were already added.
    lambda = ridge trace(H^T H) / K as in ``solve`` (none on the ones column, which with ``fit_bias`` is taken first: the same as
    centring).  tol: a candidate whose remaining diagonal d is not above tol times its first value is numerically dependent on those
    taken and never selected (default: ``default_tol``).  check_every = m > 0: every m steps one host read; the run stops once the
    last step's gain, summed over the outputs, is below ``min_gain`` trace(Y^T Y), or the pool is exhausted.  With 0 nothing is
    read until the result is built.  Raises ``ValueError`` where ``solve`` does: no rows, non-finite entries in G."""
    torch = _lib.require_gpu()
    lib = _lib.load()
    G, M, O = ne.finite_G("select").contiguous(), ne.K, ne.O
    k = int(k)
    if not 1 <= k <= M:
        raise ValueError(f"select: k = {k} of a pool of {M}")
    if not float(ridge) >= 0.0 or int(check_every) < 0:
        raise ValueError("select needs ridge >= 0 and check_every >= 0")
    diag = torch.diagonal(G)
    lam = ne.ridge_abs(ridge)
    tol = default_tol(M, fit_bias) if tol is None else float(tol)
    b = 1 if fit_bias else 0
    with torch.cuda.device(G.device):
        st = _State(G, M, O, fit_bias, lam, tol, k, torch, lib)
        total = k + b
        if check_every > 0:
            floor = float(min_gain) * float(diag[M + 1:].sum().item())
            done = 0
            while done < total:
                m = min(int(check_every), total - done)
                st.steps(m)
                done += m
                cnt = int(st.count.item())
                if cnt < done or (cnt > b and float(st.gain[cnt - 1].sum().item()) < floor):
                    break
        else:
            st.steps(total)
        cnt = int(st.count.item())
    gain = st.gain[:cnt]
    yty = diag[M + 1:]
    path = yty[None] - torch.cumsum(gain, 0)
    objective = path[b - 1:] if b else torch.cat([yty[None], path])
    return OLSResult(ne, st.sel[b:cnt], gain[b:], objective, ridge, lam, fit_bias)


def fit_ols(net, params: dict, x, y, k: int, ridge: float = 1e-8, fit_bias: bool = True, tol: float | None = None,
            check_every: int = 0, min_gain: float = 0.0, batch_size: int = 65536):
    """-> (net_k, params_k, LinearFit, OLSResult): ``NormalEquations(net).add`` -> ``select`` -> ``subnet`` in one call: the ``k``
    kernels of the pool net that explain y [N,O] on x [N,D] best, and the closed-form output layer of the net that keeps them."""
    slice_net(net, params, [0])                    # the class and tree checks, before the pass over the rows
    ne = NormalEquations(net).add(params, x, y, batch_size=batch_size)
    res = select(ne, k, ridge=ridge, fit_bias=fit_bias, tol=tol, check_every=check_every, min_gain=min_gain)
    if res.n_selected < 1:
        raise ValueError("fit_ols: no candidate explains anything of y")
    return (*res.subnet(net, params), res)
