"""How good is a trained net on a whole table: roll-out error statistics on device.

The reference answers this on the host: ``scripts/eval_irbfn_dnmpc.py`` pushes a table through ``pred_step``, rolls the label
controls and the predicted controls out side by side (:95-159) and reports position, heading and velocity errors (:162-167);
``deprecated/evaluate.py:265-283`` reports trajectory end-point errors the same way.  Here the two roll-outs, the per-row
metrics and their statistics run in one kernel (``irbfn_eval_rollout_errors``, include/irbfn_hip.h), batch after batch with
no host synchronisation, so a table of tens of millions of rows never leaves the device.  The metric definitions are this
project's own (those lines of the reference are not in the snapshot this library was written from: parity unpinned):

* per state component ``|p_i - a_i|`` of the final states (prediction ``p``, label ``a``; no angle wrapping),
* ``position`` = ``hypot(p_0 - a_0, p_1 - a_1)`` (x, y; Frenet: s, e_y),
* ``controls`` = ``mean_j |y_pred_j - y_j|`` over the 2T controls.

Statistics per metric: count of finite values, mean, rms, maximum and the row that attains it, and a histogram with eight
bins per octave (``bin_edge``) from which ``summary()`` brackets quantiles.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib, distributed
from .dynamics import _dyn
from .model import ClusterWCRBFNet, DeeperWCRBFNet, WCRBFNet, _ptr, _stream_ptr, to_device_f32

NUM_BINS = 512
QUANTILES = (0.5, 0.95, 0.99)
_INT64_MAX = (1 << 63) - 1

# names of the M = S + 2 metrics, per roll-out mode (state order of include/irbfn_hip.h: dynamics.py:9-91, train_nmpc.py:329-347,
# dynamics.py:190-281)
_ST_NAMES = ("x", "y", "delta", "v", "yaw", "yaw_rate", "slip_angle", "position", "controls")
METRIC_NAMES = {
    _lib.ROLLOUT_ST_SELECT: _ST_NAMES,
    _lib.ROLLOUT_ST_KS: _ST_NAMES,
    _lib.ROLLOUT_FULLINT: ("x", "y", "delta", "v", "yaw", "position", "controls"),
    _lib.ROLLOUT_FRENET_LS: ("s", "ey", "delta", "vx", "vy", "wz", "epsi", "cur", "position", "controls"),
}
# leading columns of a state0 row, per mode (FULLINT: v0 only)
_STATE0_COLS = {_lib.ROLLOUT_ST_SELECT: 7, _lib.ROLLOUT_ST_KS: 7, _lib.ROLLOUT_FULLINT: 1, _lib.ROLLOUT_FRENET_LS: 8}

# kind -> (default mode, allowed modes, columns of x the initial state reads)
KINDS = {
    "cartesian": (_lib.ROLLOUT_FULLINT, (_lib.ROLLOUT_FULLINT,), 1),                                   # train_nmpc.py:319
    "cartesian_st": (_lib.ROLLOUT_ST_SELECT, (_lib.ROLLOUT_ST_SELECT, _lib.ROLLOUT_ST_KS), 7),         # train_nmpc.py:260-266
    "frenet": (_lib.ROLLOUT_FRENET_LS, (_lib.ROLLOUT_FRENET_LS,), 8),                                  # train_nmpc_frenet.py:398
}
_FRENET_STATE_COLS = (0, 0, 1, 2, 3, 5, 6, 7)


def bin_edge(k: int) -> float:
    """Lower edge of histogram bin k: 2^(-40 + k // 8) * (1 + (k % 8) / 8).  Bin k holds [edge(k), edge(k + 1)); bin 0 also takes
    everything below its edge, bin 511 everything finite from edge(511) up."""
    k = int(k)
    return math.ldexp(1.0 + (k % 8) / 8.0, -40 + k // 8)


def bin_of(e) -> np.ndarray:
    """The bin of float32 values e >= 0, as the kernel computes it: clamp((bits >> 20) - 696, 0, 511)."""
    bits = np.ascontiguousarray(e, dtype=np.float32).view(np.uint32).astype(np.int64)
    return np.clip((bits >> 20) - 696, 0, NUM_BINS - 1)


class ErrorStats:
    """Running statistics of the M metrics of one roll-out mode, on the device: ``stats`` [M,4] float64 = (n, sum, sum_sq, max),
    ``argmax`` [M] int64, ``hist`` [M,512] int64, ``rows`` [1] int64 (rows seen, finite or not).  ``rollout_errors`` and
    ``evaluate_table`` add to it; ``summary()`` reads it back."""

    def __init__(self, mode: int, device=None):
        torch = _lib.require_gpu()
        lib = _lib.load()
        M = lib.irbfn_eval_num_metrics(int(mode))
        if M < 0:
            _lib.check(M, "irbfn_eval_num_metrics")
        self.mode = int(mode)
        self.names = METRIC_NAMES[self.mode]
        dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.stats = torch.zeros((M, 4), dtype=torch.float64, device=dev)
        self.stats[:, 3] = -math.inf
        self.argmax = torch.full((M,), -1, dtype=torch.int64, device=dev)
        self.hist = torch.zeros((M, NUM_BINS), dtype=torch.int64, device=dev)
        self.rows = torch.zeros((1,), dtype=torch.int64, device=dev)
        self._ws = torch.empty((int(lib.irbfn_eval_workspace_bytes(self.mode)),), dtype=torch.uint8, device=dev)

    @property
    def num_metrics(self) -> int:
        return len(self.names)

    def all_reduce(self) -> "ErrorStats":
        """Merges the ranks' statistics when ``torch.distributed`` is initialised (identity otherwise): SUM for n, sum, sum_sq,
        the histogram and the rows, MAX for max; every rank offers its argmax where its max is the global one (the int64
        maximum elsewhere) and a MIN over the offers keeps the lowest row."""
        if not distributed.is_dist():
            return self
        import torch
        import torch.distributed as dist
        sums = self.stats[:, :3].contiguous()
        dist.all_reduce(sums, op=dist.ReduceOp.SUM)
        gmax = self.stats[:, 3].contiguous()
        dist.all_reduce(gmax, op=dist.ReduceOp.MAX)
        offer = torch.where((self.stats[:, 3] == gmax) & (self.argmax >= 0), self.argmax, torch.full_like(self.argmax, _INT64_MAX))
        dist.all_reduce(offer, op=dist.ReduceOp.MIN)
        counts = torch.cat([self.hist.reshape(-1), self.rows])
        dist.all_reduce(counts, op=dist.ReduceOp.SUM)
        self.stats[:, :3] = sums
        self.stats[:, 3] = gmax
        self.argmax.copy_(torch.where(offer == _INT64_MAX, torch.full_like(offer, -1), offer))
        self.hist.copy_(counts[:-1].view_as(self.hist))
        self.rows.copy_(counts[-1:])
        return self

    def to_host(self):
        """(stats [M,4] float64, argmax [M], hist [M,512], rows) as NumPy, in ONE device-to-host copy."""
        import torch
        M = self.num_metrics
        flat = torch.cat([self.stats.view(torch.int64).reshape(-1), self.argmax, self.hist.reshape(-1), self.rows]).cpu().numpy()
        stats = flat[:4 * M].view(np.float64).reshape(M, 4).copy()
        return stats, flat[4 * M:5 * M].copy(), flat[5 * M:5 * M + M * NUM_BINS].reshape(M, NUM_BINS).copy(), int(flat[-1])

    def summary(self) -> dict:
        """{metric: {n, nonfinite, mean, rms, max, argmax, quantiles}} after one host synchronisation.  ``quantiles`` maps each
        q of (0.5, 0.95, 0.99) to the PAIR (lower_edge, upper_edge) of the histogram bin that holds the ceil(q n)-th smallest
        finite value: the quantile lies between them (edges are a factor <= 9/8 apart; the upper edge is capped at max); the
        exact value needs the per-row metrics (``per_row=True``).  mean / rms / max are NaN and argmax -1 while n = 0."""
        stats, argmax, hist, rows = self.to_host()
        out = {}
        for m, name in enumerate(self.names):
            n = int(stats[m, 0])
            d = {"n": n, "nonfinite": rows - n, "argmax": int(argmax[m])}
            if n == 0:
                d.update(mean=math.nan, rms=math.nan, max=math.nan, quantiles={q: (math.nan, math.nan) for q in QUANTILES})
            else:
                cum = np.cumsum(hist[m])
                qs = {}
                for q in QUANTILES:
                    k = int(np.searchsorted(cum, max(1, math.ceil(q * n)), side="left"))
                    qs[q] = (0.0 if k == 0 else bin_edge(k), min(bin_edge(k + 1), stats[m, 3]) if k < NUM_BINS - 1 else stats[m, 3])
                d.update(mean=stats[m, 1] / n, rms=math.sqrt(stats[m, 2] / n), max=float(stats[m, 3]), quantiles=qs)
            out[name] = d
        return out


def _run(stats: ErrorStats, sd, pd, yd, pp, row0: int, accumulate: int, err, torch, lib):
    """One call of the entry point on checked device tensors; err: [B, M] float32 tensor to fill, or None."""
    B, T = yd.shape[0], yd.shape[1] // 2
    st = lib.irbfn_eval_rollout_errors(stats.mode, _ptr(sd), _ptr(pd), _ptr(yd), pp, B, T, int(row0), int(accumulate),
                                       _ptr(err) if err is not None else C.c_void_p(None), _ptr(stats.stats), _ptr(stats.argmax),
                                       _ptr(stats.hist), _ptr(stats._ws), stats._ws.numel(), _stream_ptr(torch))
    _lib.check(st, "irbfn_eval_rollout_errors")
    if accumulate:
        stats.rows += B
    else:
        stats.rows.fill_(B)


def rollout_errors(mode: int, state0, y_pred, y, dyn_params=None, *, stats: ErrorStats = None, row0: int = 0,
                   per_row: bool = False):
    """Rolls y [B, 2T] (labels) and y_pred [B, 2T] out from state0 [B, S0] (7 single-track, 1 = v0 inline bicycle, 8 Frenet) and
    adds the rows' metrics to ``stats`` (None: a fresh ErrorStats); rows are numbered from ``row0`` for ``argmax``.
    -> stats, or (stats, err [B, M] float32 on the device) with ``per_row=True``.  dyn_params: the 13 dynamics parameters
    (dynamics.py:24-36); None for the inline bicycle."""
    torch = _lib.require_gpu()
    lib = _lib.load()
    mode = int(mode)
    fresh = stats is None
    if fresh:
        stats = ErrorStats(mode)
    elif stats.mode != mode:
        raise ValueError(f"stats hold mode {stats.mode}, not {mode}")
    sd, pd, yd = to_device_f32(state0, torch), to_device_f32(y_pred, torch), to_device_f32(y, torch)
    if yd.dim() != 2 or yd.shape[1] % 2 or yd.shape[1] < 2 or tuple(pd.shape) != tuple(yd.shape):
        raise ValueError("y and y_pred must both be [B, 2T]")
    B = yd.shape[0]
    if sd.numel() != B * _STATE0_COLS[mode]:
        raise ValueError(f"state0 must be [B, {_STATE0_COLS[mode]}]")
    keep, pp = _dyn(dyn_params)
    err = torch.empty((B, stats.num_metrics), dtype=torch.float32, device=yd.device) if per_row else None
    _run(stats, sd, pd, yd, pp, row0, 0 if fresh else 1, err, torch, lib)
    return (stats, err) if per_row else stats


def _check_net(net):
    if not isinstance(net, (WCRBFNet, DeeperWCRBFNet, ClusterWCRBFNet)):
        raise TypeError(f"evaluate_table takes a WCRBFNet, a DeeperWCRBFNet or a ClusterWCRBFNet, not {type(net).__name__}")


def _tree_to_device(tree, torch):
    """The parameter pytree with every leaf a device tensor: ``apply`` then recognises the leaves of the previous batch by
    identity instead of digesting host arrays batch after batch."""
    if isinstance(tree, dict):
        return {k: _tree_to_device(v, torch) for k, v in tree.items()}
    if isinstance(tree, torch.Tensor) and tree.is_cuda:
        return tree
    if isinstance(tree, torch.Tensor):
        return tree.to(torch.device("cuda", torch.cuda.current_device()))
    return torch.from_numpy(np.array(tree)).to(torch.device("cuda", torch.cuda.current_device()))


def _initial_state(kind: str, xb, torch):
    """The initial state the matching training loss takes from a batch of table inputs."""
    if kind == "cartesian":
        return xb[:, :1].contiguous()                                   # v0                       train_nmpc.py:319
    if kind == "cartesian_st":
        s = torch.zeros((xb.shape[0], 7), dtype=torch.float32, device=xb.device)
        s[:, 3], s[:, 5], s[:, 6] = xb[:, 0], xb[:, 6], xb[:, 5]        # [0,0,0,x0,0,x6,x5]       train_nmpc.py:260-266
        return s
    return torch.stack([xb[:, c] for c in _FRENET_STATE_COLS], dim=1)   # x[:, [0,0,1,2,3,5,6,7]]  train_nmpc_frenet.py:398


def evaluate_table(net, params: dict, x, y, kind: str, dyn_params=None, batch_size: int = 80000, per_row: bool = False,
                   mode: int = None):
    """``scripts/eval_irbfn_dnmpc.py`` for a whole table: x [N, D] inputs and y [N, 2T] label controls (arrays, or the ``.x`` /
    ``.y`` of a ``tables.DeviceTable``) -> ErrorStats of the net's predictions, or (stats, err [N_local, M]) with
    ``per_row=True``.  The rows are walked in order in batches of ``batch_size`` (the last one short); a batch is ``net.apply``
    then one kernel call that accumulates; nothing synchronises with the host inside the loop.

    kind selects the initial state from x as the matching training loss does: "cartesian" v0 = x[:, :1] -> inline bicycle;
    "cartesian_st" [0, 0, 0, x0, 0, x6, x5] -> single-track model (``mode=_lib.ROLLOUT_ST_KS`` for its kinematic form);
    "frenet" x[:, [0,0,1,2,3,5,6,7]] -> Frenet model.  net: a WCRBFNet, a DeeperWCRBFNet or a ClusterWCRBFNet (the first
    output of its ``apply``); any other type raises TypeError.  Under ``torch.distributed`` every rank evaluates its
    ``distributed.shard_range`` of the rows (numbered globally) and the statistics are merged; ``err`` stays the rank's own."""
    _check_net(net)
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {sorted(KINDS)}")
    default_mode, allowed, need_cols = KINDS[kind]
    mode = default_mode if mode is None else int(mode)
    if mode not in allowed:
        raise ValueError(f"kind '{kind}' evaluates with roll-out mode {allowed}, not {mode}")
    if batch_size < 1:
        raise ValueError("batch_size must be positive")
    torch = _lib.require_gpu()
    lib = _lib.load()
    xd, yd = to_device_f32(x, torch), to_device_f32(y, torch)
    N = xd.shape[0]
    if xd.dim() != 2 or yd.dim() != 2 or yd.shape[0] != N or xd.shape[1] != net.in_features or xd.shape[1] < need_cols:
        raise ValueError(f"x must be [N, {net.in_features}] with at least {need_cols} columns and y [N, 2T]")
    if yd.shape[1] != net.out_features or yd.shape[1] % 2:
        raise ValueError(f"the net's out_features ({net.out_features}) must be 2T, the width of y ({yd.shape[1]})")
    dev_params = _tree_to_device(params, torch)
    keep, pp = _dyn(dyn_params)
    stats = ErrorStats(mode)
    lo, hi = distributed.shard_range(N)
    err = torch.empty((hi - lo, stats.num_metrics), dtype=torch.float32, device=yd.device) if per_row else None
    for b0 in range(lo, hi, batch_size):
        b1 = min(b0 + batch_size, hi)
        xb = xd[b0:b1]
        out = net.apply(dev_params, xb)
        y_pred = to_device_f32(out[0] if isinstance(net, ClusterWCRBFNet) else out, torch)
        _run(stats, _initial_state(kind, xb, torch), y_pred, yd[b0:b1], pp, b0, 1, err[b0 - lo:b1 - lo] if per_row else None,
             torch, lib)
    stats.all_reduce()
    return (stats, err) if per_row else stats
