"""Training step on device: the counterparts of ``train_step_oneint`` /
``train_step_fullint`` (scripts/train_nmpc.py:258-300, :303-421) with
``optax.chain(clip_by_global_norm(max_grad_norm), adam(lr))`` (scripts/train_nmpc.py:231-233).

One step = fused forward (K1) -> loss/seed kernel -> parameter VJP (K2) -> [one all-reduce of the flat
gradient buffer when torch.distributed is initialised] -> clip + Adam kernel.  Parameters, Adam
moments and gradients live in ONE flat float32 buffer each (the pytree leaves are views), the step
count and the loss stay on the device: no host synchronisation per step (the reference does a
``jax.device_get`` per step, scripts/train_nmpc.py:477-479).

A ``WCRBFNet(use_float64=True)`` trains in float64, as the reference under --use_float64
(scripts/train_nmpc.py:41-42): float64 flat buffers, the float64 forward / VJP and the ``*_f64`` seed and
clip + Adam kernels.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _lib, distributed
from .dynamics import _dyn
from .model import ClusterWCRBFNet, DeeperWCRBFNet, WCRBFNet, _ptr, _stream_ptr, to_device_f32


class TrainState:
    """Stand-in of ``flax.training.train_state.TrainState`` for the hot path: ``params`` (pytree of views
    into a flat buffer), Adam moments, device-resident step count.  A fixed-centre / fixed-width net's buffers hold its
    live leaves only, so the clip by global norm runs over them (what optax does on the reduced tree)."""

    def __init__(self, net: WCRBFNet, flat, lr, max_grad_norm, b1, b2, eps):
        import torch
        self.net = net
        self.flat = flat
        self.m = torch.zeros_like(flat)
        self.v = torch.zeros_like(flat)
        # gradients + two trailing slots (loss * B_local, B_local) so that ONE all-reduce yields the global-batch
        # mean gradient and loss whatever the shard sizes are (distributed.shard_range hands out sizes that
        # differ by one row)
        self.gbuf = torch.zeros(flat.numel() + 2, dtype=flat.dtype, device=flat.device)
        self.g = self.gbuf[:flat.numel()]
        self.step = torch.zeros(1, dtype=torch.int32, device=flat.device)
        self.loss = torch.zeros(1, dtype=flat.dtype, device=flat.device)
        self.partials = torch.zeros(_lib.load().irbfn_train_loss_partials(), dtype=flat.dtype, device=flat.device)
        self.lr, self.max_grad_norm, self.b1, self.b2, self.eps = float(lr), float(max_grad_norm), float(b1), float(b2), float(eps)
        self.params = distributed.unflatten_params(net, self.flat)
        self.grads = distributed.unflatten_params(net, self.g)
        self.apply_fn = net.apply

    @classmethod
    def create(cls, net: WCRBFNet, params: dict, lr: float = 1e-3, max_grad_norm: float = 1.0,
               b1: float = 0.9, b2: float = 0.999, eps: float = 1e-8, opt_state=None) -> "TrainState":
        """opt_state: (mu pytree, nu pytree, count) to resume (``checkpoint.restore_opt_state``).  A ``use_float64`` net
        gets a float64 state: parameters, moments, gradient, loss and partials in float64."""
        torch = _lib.require_gpu()
        dtype = torch.float64 if getattr(net, "use_float64", False) else torch.float32
        if isinstance(net, WCRBFNet):
            net._check_shapes(params["params"] if "params" in params else params)    # a frozen net: its live leaves only
        flat = distributed.flatten_params(distributed.params_to_device(params, dtype=dtype)).clone()
        st = cls(net, flat, lr, max_grad_norm, b1, b2, eps)
        if dtype == torch.float32:
            # a training loop re-binds the parameters every step: the matrix-core kernels' "do the parameters fit" verdict is read
            # back for the first bind only (the kernels test the device-side verdict themselves; include/irbfn_hip.h,
            # IRBFN_OPT_GRAM_STICKY).  The float64 mode binds no float32 descriptor.
            net.set_options(gram_sticky=1)
        if opt_state is not None:
            st.m.copy_(distributed.flatten_params(distributed.params_to_device(opt_state[0], dtype=dtype)))
            st.v.copy_(distributed.flatten_params(distributed.params_to_device(opt_state[1], dtype=dtype)))
            st.step.fill_(int(opt_state[2]))
        return st

    def opt_state(self):
        """(mu pytree, nu pytree, count): what ``checkpoint.save_checkpoint(..., opt_state=)`` stores (one host sync)."""
        return (distributed.unflatten_params(self.net, self.m), distributed.unflatten_params(self.net, self.v),
                int(self.step.item()))


class ClusterTrainState(TrainState):
    """TrainState of a ``ClusterWCRBFNet`` (scripts/train_nmpc_frenet.py:424-453): the flat buffers hold the four
    leaves of the RBF stage followed by ``cluster.kernel`` [D,R] and ``cluster.bias`` [R]."""

    def __init__(self, net: ClusterWCRBFNet, flat, lr, max_grad_norm, b1, b2, eps):
        self._cluster = net
        super().__init__(net.stage, flat[:distributed.flat_param_count(net.stage)], lr, max_grad_norm, b1, b2, eps)
        import torch
        self.net = net
        self.flat = flat
        self.m, self.v = torch.zeros_like(flat), torch.zeros_like(flat)
        self.gbuf = torch.zeros(flat.numel() + 2, dtype=torch.float32, device=flat.device)
        self.g = self.gbuf[:flat.numel()]
        self.params, self.grads = self._views(self.flat), self._views(self.g)
        self.apply_fn = net.apply

    def _views(self, flat) -> dict:
        n = distributed.flat_param_count(self._cluster.stage)
        D, R = self._cluster.in_features, self._cluster.num_regions
        p = distributed.unflatten_params(self._cluster.stage, flat[:n])
        p["params"]["cluster"] = {"kernel": flat[n:n + D * R].view(D, R), "bias": flat[n + D * R:n + D * R + R].view(R)}
        return p

    @classmethod
    def create(cls, net: ClusterWCRBFNet, params: dict, lr: float = 1e-3, max_grad_norm: float = 1.0,
               b1: float = 0.9, b2: float = 0.999, eps: float = 1e-8, opt_state=None) -> "ClusterTrainState":
        """opt_state: (mu pytree, nu pytree, count) with the six leaves, to resume (``checkpoint.restore_opt_state``)."""
        torch = _lib.require_gpu()
        if getattr(net, "use_float64", False) or getattr(getattr(net, "stage", None), "use_float64", False):
            raise ValueError("ClusterTrainState has no float64 mode: ClusterWCRBFNet runs in float32")

        def flat6(tree):
            p = tree["params"] if "params" in tree else tree
            stage = distributed.flatten_params(distributed.params_to_device(p))
            return torch.cat([stage, to_device_f32(p["cluster"]["kernel"], torch).reshape(-1),
                              to_device_f32(p["cluster"]["bias"], torch).reshape(-1)]).clone()
        st = cls(net, flat6(params), lr, max_grad_norm, b1, b2, eps)
        if opt_state is not None:
            st.m.copy_(flat6(opt_state[0]))
            st.v.copy_(flat6(opt_state[1]))
            st.step.fill_(int(opt_state[2]))
        return st

    def opt_state(self):
        return self._views(self.m), self._views(self.v), int(self.step.item())


class DeeperTrainState(TrainState):
    """TrainState of a ``DeeperWCRBFNet`` (scripts/train_nmpc_frenet.py:388-417), float32 only: the flat buffers hold the eight
    leaves in ``DeeperWCRBFNet.LEAVES`` order.  A step keeps the stage output h1 of its forward for the VJP (the RBF stage
    runs once) and runs the stage VJP on K2m where the stage descriptor supports it (``stage_vjp_kernel``)."""

    @classmethod
    def create(cls, net: DeeperWCRBFNet, params: dict, lr: float = 1e-3, max_grad_norm: float = 1.0,
               b1: float = 0.9, b2: float = 0.999, eps: float = 1e-8, opt_state=None) -> "DeeperTrainState":
        """opt_state: (mu pytree, nu pytree, count) with the eight leaves, to resume (``checkpoint.restore_opt_state``)."""
        torch = _lib.require_gpu()
        if not isinstance(net, DeeperWCRBFNet):
            raise TypeError("DeeperTrainState trains a DeeperWCRBFNet (TrainState: WCRBFNet, ClusterTrainState: ClusterWCRBFNet)")
        net._check_shapes(params["params"] if "params" in params else params)
        flat = distributed.flatten_params(distributed.params_to_device(params)).clone()
        st = cls(net, flat, lr, max_grad_norm, b1, b2, eps)
        net.stage.set_options(gram_sticky=1)        # as TrainState.create: no read-back of the pack's verdict per re-bind
        if opt_state is not None:
            st.m.copy_(distributed.flatten_params(distributed.params_to_device(opt_state[0])))
            st.v.copy_(distributed.flatten_params(distributed.params_to_device(opt_state[1])))
            st.step.fill_(int(opt_state[2]))
        return st

    def stage_vjp_kernel(self, B: int) -> int:
        """The stage VJP's kernel for a batch of B: K2m where the descriptor takes it, else the automatic choice."""
        lib = _lib.load()
        import torch
        h = self.net.stage._handle(torch)
        return _lib.VJP_K2M if lib.irbfn_net_vjp_kernel_supported(h, _lib.VJP_K2M, int(B)) == 1 else _lib.VJP_AUTO


def _forward(state: TrainState, xd):
    """The step's forward -> (prediction, the keywords of its VJP): a DeeperTrainState keeps h1 for the stage VJP."""
    if isinstance(state, DeeperTrainState):
        y_pred, h1 = state.net.apply_with_hidden(state.params, xd)
        return y_pred, {"h1": h1, "stage_vjp_kernel": state.stage_vjp_kernel(xd.shape[0])}
    return state.net.apply(state.params, xd), {}


def _is_f64(state: TrainState, torch) -> bool:
    return state.flat.dtype == torch.float64


def _step_inputs(state: TrainState, x, y, torch):
    """x, y as contiguous device tensors of the state's dtype."""
    if _is_f64(state, torch):
        return WCRBFNet._dev_f64(x, torch), WCRBFNet._dev_f64(y, torch)
    return to_device_f32(x, torch), to_device_f32(y, torch)


def _fresh_loss(state: TrainState, torch):
    """Every step writes its loss into a 1-element device buffer of its own (caching allocator: no launch), so the
    tensor a step returns stays valid without a device-to-device copy per step."""
    state.loss = torch.empty_like(state.loss)


def _backward_and_update(state: TrainState, x, gy, torch, lib, **vjp_kw):
    """VJP -> [all-reduce] -> clip + Adam.  Returns the loss of the (global) batch, a 1-element device tensor."""
    state.net.vjp(state.params, x, gy, out=state.grads, **vjp_kw)
    loss = state.loss            # a buffer of this step's own (see _fresh_loss): no copy, never overwritten later
    if distributed.is_dist() and torch.distributed.get_world_size() > 1:
        # every rank normalised its seeds and its loss by its LOCAL batch: weight both by B_local, sum over the
        # ranks in one all-reduce of the flat buffer, divide by the global batch (exact for unequal shards)
        n, b_local = state.flat.numel(), float(x.shape[0])
        state.g.mul_(b_local)
        state.gbuf[n:n + 1].copy_(state.loss * b_local)
        state.gbuf[n + 1:].fill_(b_local)
        torch.distributed.all_reduce(state.gbuf, op=torch.distributed.ReduceOp.SUM)
        state.g.div_(state.gbuf[n + 1])
        loss = (state.gbuf[n:n + 1] / state.gbuf[n + 1]).clone()
    adam = lib.irbfn_adam_clip_step_f64 if _is_f64(state, torch) else lib.irbfn_adam_clip_step
    st = adam(_ptr(state.flat), _ptr(state.g), _ptr(state.m), _ptr(state.v), state.flat.numel(), _ptr(state.step), state.lr,
              state.b1, state.b2, state.eps, state.max_grad_norm, _ptr(state.partials), _stream_ptr(torch))
    _lib.check(st, adam.__name__)
    # the parameter leaves were updated in place behind torch's back: re-bind on the next apply
    getattr(state.net, "stage", state.net)._bound_fp.pop(torch.cuda.current_device(), None)
    return loss


def train_step_oneint(state: TrainState, x, y, dyn_params, clip_tie: float = 0.5) -> Tuple[TrainState, "object"]:
    """scripts/train_nmpc.py:258-300.  x [B,7], y [B,O>=2] device tensors -> (state, loss[1] on device)."""
    torch = _lib.require_gpu()
    lib = _lib.load()
    f64 = _is_f64(state, torch)
    xd, yd = _step_inputs(state, x, y, torch)
    B, O = yd.shape
    if xd.shape[1] < 7 or O != state.net.out_features or O < 2:
        raise ValueError("train_step_oneint needs x [B,7] and y [B,out_features >= 2]")
    y_pred, vjp_kw = _forward(state, xd)
    gy = torch.empty_like(y_pred)
    keep, pp = _dyn(dyn_params, np.float64 if f64 else np.float32)
    _fresh_loss(state, torch)
    seeds = lib.irbfn_train_seeds_oneint_f64 if f64 else lib.irbfn_train_seeds_oneint
    st = seeds(_ptr(xd), _ptr(y_pred), _ptr(yd), pp, float(clip_tie), _ptr(gy), _ptr(state.loss), _ptr(state.partials), B,
               xd.shape[1], O, _stream_ptr(torch))
    _lib.check(st, seeds.__name__)
    return state, _backward_and_update(state, xd, gy, torch, lib, **vjp_kw)


def train_step_fullint(state: TrainState, x, y, clip_tie: float = 0.5) -> Tuple[TrainState, "object"]:
    """scripts/train_nmpc.py:303-421.  x [B,D], y [B,2T] -> (state, loss[1] on device)."""
    torch = _lib.require_gpu()
    lib = _lib.load()
    xd, yd = _step_inputs(state, x, y, torch)
    B, O = yd.shape
    if O != state.net.out_features or O % 2:
        raise ValueError("train_step_fullint needs y [B, out_features = 2T]")
    y_pred, vjp_kw = _forward(state, xd)
    gy = torch.empty_like(y_pred)
    _fresh_loss(state, torch)
    seeds = lib.irbfn_train_seeds_fullint_f64 if _is_f64(state, torch) else lib.irbfn_train_seeds_fullint
    st = seeds(_ptr(xd), _ptr(y_pred), _ptr(yd), float(clip_tie), _ptr(gy), _ptr(state.loss), _ptr(state.partials), B,
               xd.shape[1], O // 2, _stream_ptr(torch))
    _lib.check(st, seeds.__name__)
    return state, _backward_and_update(state, xd, gy, torch, lib, **vjp_kw)


def train_step_frenet_fullint(state: TrainState, x, y, dyn_params, clip_tie: float = 0.5) -> Tuple[TrainState, "object"]:
    """Frenet ``train_step_fullint`` (scripts/train_nmpc_frenet.py:394-421).  x [B,8], y [B,2T] (T <= 16; the
    reference's tables hold T = 5) -> (state, loss[1] on device).  The gradient runs through
    ``integrate_frenet_mult`` on device (the adjoint of the low-speed Frenet model)."""
    torch = _lib.require_gpu()
    lib = _lib.load()
    f64 = _is_f64(state, torch)
    xd, yd = _step_inputs(state, x, y, torch)
    B, O = yd.shape
    if xd.shape[1] != 8 or O != state.net.out_features or O % 2 or O // 2 > 16:
        raise ValueError("train_step_frenet_fullint needs x [B,8] and y [B, out_features = 2T], T <= 16")
    y_pred, vjp_kw = _forward(state, xd)
    gy = torch.empty_like(y_pred)
    keep, pp = _dyn(dyn_params, np.float64 if f64 else np.float32)
    _fresh_loss(state, torch)
    seeds = lib.irbfn_train_seeds_frenet_fullint_f64 if f64 else lib.irbfn_train_seeds_frenet_fullint
    st = seeds(_ptr(xd), _ptr(y_pred), _ptr(yd), pp, float(clip_tie), _ptr(gy), _ptr(state.loss), _ptr(state.partials), B, 8,
               O // 2, _stream_ptr(torch))
    _lib.check(st, seeds.__name__)
    return state, _backward_and_update(state, xd, gy, torch, lib, **vjp_kw)


def train_step_st_fullint(state: TrainState, x, y, dyn_params, mode: int = _lib.ROLLOUT_ST_SELECT,
                          clip_tie: float = 0.5) -> Tuple[TrainState, "object"]:
    """A full-integration step through the single-track roll-out the planner uses (``integrate_st_mult``, ``mode`` =
    ``ROLLOUT_ST_SELECT``) or its kinematic part alone (``ROLLOUT_ST_KS``); the reference has no such step.  x [B, D >= 7] as
    for ``train_step_oneint``, y [B, 2T] (T <= 16) -> (state, loss[1] on device);
    loss = mean|y_pred - y| + mean|S_pred[:, :, [0,1,3,4]] - S_act[:, :, [0,1,3,4]]| over the T states of both roll-outs.
    The select model is differentiated branch by branch (``dynamics.rollout_vjp_select``).  float32 states of a ``WCRBFNet`` or
    a ``DeeperWCRBFNet`` only."""
    torch = _lib.require_gpu()
    lib = _lib.load()
    if isinstance(state, ClusterTrainState):
        raise ValueError("train_step_st_fullint has no cluster form: a ClusterTrainState trains with train_step_fullint_withcluster")
    if _is_f64(state, torch):
        raise ValueError("train_step_st_fullint runs in float32 only (the select model has no float64 form)")
    if mode not in (_lib.ROLLOUT_ST_SELECT, _lib.ROLLOUT_ST_KS):
        raise ValueError("train_step_st_fullint: mode must be ROLLOUT_ST_SELECT or ROLLOUT_ST_KS")
    xd, yd = _step_inputs(state, x, y, torch)
    B, O = yd.shape
    if xd.shape[1] < 7 or O != state.net.out_features or O % 2 or not 1 <= O // 2 <= 16:
        raise ValueError("train_step_st_fullint needs x [B, D >= 7] and y [B, out_features = 2T], 1 <= T <= 16")
    y_pred, vjp_kw = _forward(state, xd)
    gy = torch.empty_like(y_pred)
    keep, pp = _dyn(dyn_params)
    _fresh_loss(state, torch)
    st = lib.irbfn_train_seeds_st_fullint(int(mode), _ptr(xd), _ptr(y_pred), _ptr(yd), pp, float(clip_tie), _ptr(gy),
                                          _ptr(state.loss), _ptr(state.partials), B, xd.shape[1], O // 2, _stream_ptr(torch))
    _lib.check(st, "irbfn_train_seeds_st_fullint")
    return state, _backward_and_update(state, xd, gy, torch, lib, **vjp_kw)


def train_step_fullint_withcluster(state: ClusterTrainState, x, y, cluster_ids, dyn_params, clip_tie: float = 0.5):
    """``train_step_fullint_withcluster`` (scripts/train_nmpc_frenet.py:424-453): the Frenet full-integration loss plus
    ``optax.softmax_cross_entropy(logits, cluster_ids).mean()`` on the gate of a ClusterWCRBFNet.  x [B,8], y [B,2T],
    cluster_ids [B,R] (one-hot or soft labels) -> (state, loss[1] on device)."""
    torch = _lib.require_gpu()
    lib = _lib.load()
    xd, yd, cd = to_device_f32(x, torch), to_device_f32(y, torch), to_device_f32(cluster_ids, torch)
    B, O = yd.shape
    net = state.net
    if xd.shape[1] != 8 or O != net.out_features or O % 2 or O // 2 > 16 or tuple(cd.shape) != (B, net.num_regions):
        raise ValueError("train_step_fullint_withcluster needs x [B,8], y [B, out_features = 2T] (T <= 16), cluster_ids [B,R]")
    y_pred, logits = net.apply(state.params, xd)
    gy, glogits = torch.empty_like(y_pred), torch.empty_like(logits)
    keep, pp = _dyn(dyn_params)
    stream = _stream_ptr(torch)
    _fresh_loss(state, torch)
    st = lib.irbfn_train_seeds_frenet_fullint(_ptr(xd), _ptr(y_pred), _ptr(yd), pp, float(clip_tie), _ptr(gy),
                                              _ptr(state.loss), _ptr(state.partials), B, 8, O // 2, stream)
    _lib.check(st, "irbfn_train_seeds_frenet_fullint")
    st = lib.irbfn_softmax_xent(_ptr(logits), _ptr(cd), _ptr(glogits), _ptr(state.loss), _ptr(state.partials), 1, B,
                                net.num_regions, stream)
    _lib.check(st, "irbfn_softmax_xent")
    return state, _backward_and_update(state, xd, gy, torch, lib, glogits=glogits)


def train_epoch(state: TrainState, table, batch_size: int, only_onestep: bool = False, dyn_params=None):
    """scripts/train_nmpc.py:455-486: one pass over a ``tables.DeviceTable``.  Returns (state, losses [steps]
    on the device) -- the reference fetches every batch loss to the host (``jax.device_get``, :477-481);
    here nothing synchronises until the caller reads ``losses``.
    A ``ClusterTrainState`` takes a labelled table (``DeviceTable(labels=, num_classes=)``) and ``dyn_params`` and runs
    ``train_step_fullint_withcluster`` (scripts/train_nmpc_frenet.py:424-453) on every batch."""
    torch = _lib.require_gpu()
    losses = []
    cluster = isinstance(state, ClusterTrainState)
    if cluster:
        if getattr(table, "labels", None) is None:
            raise ValueError("train_epoch with a ClusterTrainState needs a labelled table: DeviceTable(labels=, num_classes=)")
        if dyn_params is None:
            raise ValueError("train_epoch with a ClusterTrainState needs dyn_params")
    for batch in table.epoch(batch_size):
        bx, by = batch[0], batch[1]
        if cluster:
            state, loss = train_step_fullint_withcluster(state, bx, by, batch[2], dyn_params)
        elif only_onestep:
            state, loss = train_step_oneint(state, bx, by, dyn_params)
        else:
            state, loss = train_step_fullint(state, bx, by)
        losses.append(loss)
    return state, (torch.cat(losses) if losses else torch.zeros(0, dtype=state.loss.dtype, device=state.flat.device))
