"""``WCRBFNet`` -- host-side mirror of the reference's Flax module (src/irbfn_mpc/model.py:98-198).

Same constructor fields as the reference / its YAML model card, same call surface
``WCRBFNet(**cfg).apply(params, x)`` with the same parameter pytree
``{"params": {"rbf_list": {"centers"[R,K,D], "log_sigs"[R,K]}, "linear": {"kernel"[K,O], "bias"[O]}}}``
(checkpoint layout).  The arithmetic runs in the HIP kernels behind ``libirbfn_hip.so``; torch is
used only for device memory and streams.  No CPU path: without the library or a GPU, calls raise.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, Optional, Sequence

import numpy as np

from . import _lib
from .flax_rbf import basis_name

_CFG_FIELDS = ("in_features", "out_features", "num_kernels", "basis_func", "num_regions", "lower_bounds",
               "upper_bounds", "dimension_ranges", "activation_idx", "delta")


NO_F64_HIDDEN = "the float64 mode has no hidden-layer kernel (construct the net with use_float64=False)"      # after the caller's prefix


def _inner(params: dict) -> dict:
    return params["params"] if "params" in params else params


def _digest(arr: np.ndarray) -> bytes:
    """Content digest of a host array (xxh3 at memory speed when xxhash is there, blake2b otherwise)."""
    buf = np.ascontiguousarray(arr)
    try:
        import xxhash
        return xxhash.xxh3_128_digest(memoryview(buf).cast("B"))
    except ImportError:
        import hashlib
        return hashlib.blake2b(memoryview(buf).cast("B"), digest_size=16).digest()


def _ptr(t) -> C.c_void_p:
    return C.c_void_p(t.data_ptr())


def _stream_ptr(torch) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def to_device_f32(a, torch, device=None):
    """numpy / torch (any float dtype, any device) -> contiguous float32 cuda tensor (no copy if already so)."""
    if isinstance(a, torch.Tensor):
        t = a
    else:
        arr = np.ascontiguousarray(np.asarray(a))
        t = torch.from_numpy(arr) if arr.flags.writeable else torch.tensor(arr)    # read-only arrays: torch wants a copy
    if t.dtype != torch.float32:
        t = t.to(torch.float32)     # float64 checkpoints are cast on load
    dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
    if t.device != dev:
        t = t.to(dev)
    return t.contiguous()


def like_input(out_t, ref, torch):
    """Give the result the flavour of the caller's input: numpy in -> numpy out, torch-cpu -> torch-cpu."""
    if isinstance(ref, torch.Tensor):
        return out_t if ref.is_cuda else out_t.cpu()
    return out_t.cpu().numpy()


def _load_card(cfg) -> dict:
    """A model card as a dict: cfg is a dict, an argparse.Namespace or the path of a YAML card."""
    if isinstance(cfg, str):
        import yaml
        with open(cfg, "r") as f:
            return yaml.safe_load(f)
    return cfg if isinstance(cfg, dict) else vars(cfg)


def _grown_ws(cache: dict, key, nbytes: int, torch, dev):
    """The byte workspace kept in cache[key], grown on demand and reused across steps."""
    ws = cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty((max(int(nbytes), 8),), dtype=torch.uint8, device=dev)
        cache[key] = ws
    return ws


def _check_out_leaf(t, shape, dtype, torch, what="vjp"):
    """A caller-provided gradient leaf (``out=``, e.g. a view of one flat buffer) must be what the kernels write."""
    if tuple(t.shape) != tuple(shape) or t.dtype != dtype or not t.is_cuda or not t.is_contiguous():
        raise ValueError(f"{what} out= leaves must be contiguous {str(dtype).split('.')[-1]} cuda tensors of the parameter shapes")


class WCRBFNet:
    """Interpolating RBF network (smooth region gate, R vmapped RBF layers, Dense).

    Fields as in src/irbfn_mpc/model.py:112-125.  ``centers`` / ``fixed_centers`` / ``fixed_width``
    select the reference's RBF layer class (model.py:131-140; the upstream classes are not in the reference
    snapshot: parity unpinned).  They share the forward arithmetic of ``RBFLayer`` and differ in which leaves train:

    * ``centers=C`` alone (warm start): ``init()`` takes the centres from C; the tree is the full one;
    * ``centers=C, fixed_centers=True``: the centres are constants of the net; the tree is
      ``{"rbf_list": {"log_sigs"}, "linear": {...}}``;
    * ``centers=C, fixed_width=True``: centres and widths are constants (widths from ``log_sigs=``, a scalar or
      [R,K]; default 0, RBFLayer's initial value -- the upstream value is not known); the tree is ``{"linear": {...}}``.

    C is [R,K,D] or [K,D] (the same centres in every region).  The flags without ``centers`` freeze nothing (with a
    warning).  A frozen net's ``init`` / ``vjp`` use the reduced tree and its ``apply`` / ``bind`` take it; a tree
    that carries a frozen leaf raises ``ValueError``.
    """

    def __init__(self, in_features: int, out_features: int, num_kernels: int, basis_func: Any,
                 num_regions: int, lower_bounds: Sequence[Sequence[float]],
                 upper_bounds: Sequence[Sequence[float]], dimension_ranges: Sequence[Sequence[int]],
                 activation_idx: Sequence[int], delta: Sequence[float], centers=None,
                 fixed_centers: bool = False, fixed_width: bool = False, use_float64: bool = False, log_sigs=None,
                 **_unused):
        self.in_features = int(in_features)
        self.out_features = int(out_features)
        self.num_kernels = int(num_kernels)
        self.basis_func = basis_name(basis_func)
        self.num_regions = int(num_regions)
        self.lower_bounds = [list(map(float, r)) for r in lower_bounds]
        self.upper_bounds = [list(map(float, r)) for r in upper_bounds]
        self.dimension_ranges = [list(map(int, r)) for r in dimension_ranges]
        self.activation_idx = list(activation_idx)
        self.delta = list(map(float, delta))
        self.fixed_centers, self.fixed_width = bool(fixed_centers), bool(fixed_width)
        # float64 mode = the reference's --use_float64 (scripts/train_nmpc.py:41-42): apply / vjp evaluate in float64 on the
        # GPU (irbfn_f64_*: plain f64 kernels, not the tuned float32 path) and return float64
        self.use_float64 = bool(use_float64)
        self._f64 = {}
        self._warned_f64 = False
        self.num_split_dimensions = len(self.activation_idx)          # model.py:128
        ns = self.num_split_dimensions
        if ns > self.in_features:
            raise ValueError("len(activation_idx) exceeds in_features")
        if len(self.lower_bounds) < ns or len(self.upper_bounds) < ns or len(self.delta) < ns:
            raise ValueError("lower_bounds / upper_bounds / delta must cover every split dimension")
        for i, r in enumerate(self.dimension_ranges):
            if len(r) < ns:
                raise ValueError(f"dimension_ranges[{i}] shorter than the number of split dimensions")
            for d in range(ns):
                if not (0 <= r[d] < len(self.lower_bounds[d]) and r[d] < len(self.upper_bounds[d])):
                    raise IndexError(f"dimension_ranges[{i}][{d}]={r[d]} indexes outside the bounds of dim {d}")
        self._init_frozen(centers, log_sigs)
        self._handles: Dict[int, C.c_void_p] = {}
        self._const_dev: Dict[tuple, tuple] = {}
        self._bound_fp: Dict[int, tuple] = {}
        self._keepalive: Dict[int, tuple] = {}
        self._vjp_ws: Dict[int, Any] = {}

    def _init_frozen(self, centers, log_sigs):
        """The layer class: which leaves are constants of the net (``frozen``) and their values."""
        R, K, D = self.num_regions, self.num_kernels, self.in_features
        self.centers = None
        if centers is not None:
            c = np.asarray(centers.detach().cpu() if hasattr(centers, "detach") else centers)
            if c.shape == (K, D):
                c = np.broadcast_to(c, (R, K, D))
            if c.shape != (R, K, D):
                raise ValueError(f"centers has shape {c.shape}, the model card implies ({R}, {K}, {D}) or ({K}, {D})")
            self.centers = np.ascontiguousarray(c, dtype=np.float64 if c.dtype == np.float64 else np.float32)
        elif self.fixed_centers or self.fixed_width:
            import warnings
            warnings.warn("WCRBFNet: fixed_centers / fixed_width without centers= freeze nothing (the reference loads the "
                          "centres from a file); every leaf trains", stacklevel=3)
        frozen = ()
        if self.centers is not None and self.fixed_width:
            frozen = ("centers", "log_sigs")
        elif self.centers is not None and self.fixed_centers:
            frozen = ("centers",)
        self.frozen = frozen
        self.log_sigs = None
        if "log_sigs" in frozen:
            ls = np.asarray(0.0 if log_sigs is None else log_sigs, dtype=np.float64)
            if ls.ndim == 0:
                ls = np.full((R, K), float(ls))
            if ls.shape != (R, K):
                raise ValueError(f"log_sigs has shape {ls.shape}, expected a scalar or ({R}, {K})")
            self.log_sigs = np.ascontiguousarray(ls)
        elif log_sigs is not None:
            raise ValueError("log_sigs= is the constant width of a fixed_width net (with centers=)")

    def live_leaves(self) -> tuple:
        """(group, name) of the leaves that train, in checkpoint order."""
        return tuple((g, n) for g, n in (("rbf_list", "centers"), ("rbf_list", "log_sigs"), ("linear", "kernel"), ("linear", "bias"))
                     if n not in self.frozen)

    def leaf_shapes(self) -> dict:
        R, K, D, O = self.num_regions, self.num_kernels, self.in_features, self.out_features
        return {"centers": (R, K, D), "log_sigs": (R, K), "kernel": (K, O), "bias": (O,)}

    def _const(self, torch, dtype):
        """The frozen leaves as device tensors, uploaded once per device and dtype."""
        key = (torch.cuda.current_device(), str(dtype))
        ent = self._const_dev.get(key)
        if ent is None:
            dev = torch.device("cuda", key[0])
            ent = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dtype) if a is not None else None
                        for a in (self.centers if "centers" in self.frozen else None, self.log_sigs))
            self._const_dev[key] = ent
        return ent

    def _leaves(self, p: dict, torch, dtype=None) -> list:
        """[centers, log_sigs, kernel, bias] of a (checked) tree, the frozen ones from the net."""
        c = p["rbf_list"]["centers"] if "centers" not in self.frozen else self._const(torch, dtype or torch.float32)[0]
        ls = p["rbf_list"]["log_sigs"] if "log_sigs" not in self.frozen else self._const(torch, dtype or torch.float32)[1]
        return [c, ls, p["linear"]["kernel"], p["linear"]["bias"]]

    # ------------------------------------------------------------------ construction helpers
    @classmethod
    def from_config(cls, cfg, use_float64: bool = False, centers=None) -> "WCRBFNet":
        """cfg: dict, argparse.Namespace or path of a YAML model card (the file the reference writes at
        scripts/train_nmpc.py:431-450 and reloads at src/irbfn_mpc/irbfn_planner.py:46-79).  The reference's card does not
        record --use_float64 (a process-wide jax flag there): pass ``use_float64=True`` for that mode.  A card written by
        ``config()`` of a float64 net holds ``use_float64: True`` and keeps the mode.  centers: the centres file's array,
        which the card does not hold (as in the reference); with it the card's ``fixed_centers`` / ``fixed_width`` (and
        ``log_sigs``) restore the layer class."""
        cfg = _load_card(cfg)
        extra = {k: cfg[k] for k in ("fixed_centers", "fixed_width", "log_sigs") if cfg.get(k) is not None}
        return cls(**{k: cfg[k] for k in _CFG_FIELDS}, use_float64=use_float64 or bool(cfg.get("use_float64", False)),
                   centers=centers, **extra)

    def config(self) -> dict:
        cfg = {k: getattr(self, k) for k in _CFG_FIELDS}
        if self.use_float64:           # float32 cards stay as the reference writes them
            cfg["use_float64"] = True
        if self.fixed_centers:
            cfg["fixed_centers"] = True
        if self.fixed_width:
            cfg["fixed_width"] = True
            if self.log_sigs is not None:
                ls = self.log_sigs
                cfg["log_sigs"] = float(ls.flat[0]) if np.all(ls == ls.flat[0]) else ls.tolist()
        return cfg

    def init(self, seed: int = 0, dtype=np.float32) -> dict:
        """Fresh parameter pytree with the reference initialisers: centers ~ N(0,1), log_sigs = 0
        (flax_rbf.py:246-256), Dense kernel lecun_normal, bias 0 (flax.linen.Dense defaults)."""
        rng = np.random.default_rng(seed)
        R, K, D, O = self.num_regions, self.num_kernels, self.in_features, self.out_features
        std = 1.0 / np.sqrt(K) / 0.87962566103423978   # truncated-normal correction of lecun_normal
        kern = np.clip(rng.normal(size=(K, O)), -2, 2) * std
        centers = rng.normal(size=(R, K, D)).astype(dtype)
        if self.centers is not None:           # warm start / the net's constant centres
            centers = self.centers.astype(dtype)
        p = {"rbf_list": {"centers": centers, "log_sigs": np.zeros((R, K), dtype)},
             "linear": {"kernel": kern.astype(dtype), "bias": np.zeros((O,), dtype)}}
        for name in self.frozen:               # a frozen net's tree holds the live leaves only
            del p["rbf_list"][name]
        if not p["rbf_list"]:
            del p["rbf_list"]
        return {"params": p}

    # ------------------------------------------------------------------ descriptor management
    def _gate_tables(self, dtype=np.float32):
        ns = self.num_split_dimensions
        mr = max([1] + [max(len(self.lower_bounds[d]), len(self.upper_bounds[d])) for d in range(ns)])
        lo = np.zeros((max(ns, 1), mr), dtype)
        hi = np.zeros((max(ns, 1), mr), dtype)
        for d in range(ns):
            lo[d, :len(self.lower_bounds[d])] = self.lower_bounds[d]
            hi[d, :len(self.upper_bounds[d])] = self.upper_bounds[d]
        delta = np.asarray(self.delta[:ns] if ns else [0.0], dtype)
        nr = min(len(self.dimension_ranges), self.num_regions)   # .at[:, i].set past R is dropped
        dr = np.asarray([r[:ns] for r in self.dimension_ranges[:nr]], np.int32).reshape(nr, ns)
        return ns, mr, lo, hi, delta, np.ascontiguousarray(dr), nr

    def _handle(self, torch) -> C.c_void_p:
        dev = torch.cuda.current_device()
        h = self._handles.get(dev)
        if h is None:
            lib = _lib.load()
            ns, mr, lo, hi, delta, dr, nr = self._gate_tables()
            h = C.c_void_p()
            st = lib.irbfn_net_create(
                C.byref(h), self.in_features, self.num_regions, self.num_kernels, self.out_features,
                _lib.BASIS_ENUM[self.basis_func], ns, mr, lo.ctypes.data_as(C.c_void_p),
                hi.ctypes.data_as(C.c_void_p), delta.ctypes.data_as(C.c_void_p),
                dr.ctypes.data_as(C.c_void_p), nr)
            _lib.check(st, "irbfn_net_create")
            self._handles[dev] = h
        return h

    def set_options(self, **opts) -> "WCRBFNet":
        """Per-descriptor kernel selection / launch geometry (``irbfn_net_set_option``; names = keys of
        ``_lib.OPTIONS``, e.g. ``fwd_kernel=_lib.FWD_K1``).  For A/B measurements and the reduced-precision
        report of BASELINE config 5; the defaults are the product path."""
        torch = _lib.require_gpu()
        lib = _lib.load()
        h = self._handle(torch)
        for k, v in opts.items():
            _lib.check(lib.irbfn_net_set_option(h, _lib.OPTIONS[k], int(v)), f"irbfn_net_set_option({k}={v})")
            if k == "fwd_gamma_kernel" or (k == "vjp_kernel" and self.num_regions > 1):
                # the option decides which images irbfn_net_set_params packs (FWDG_K1G, VJP_K2G_GAMMA): the next bind packs again
                self._bound_fp.pop(torch.cuda.current_device(), None)
        return self

    def __del__(self):
        try:
            lib = _lib.load()
            for h in self._handles.values():
                lib.irbfn_net_destroy(h)
        except Exception:
            pass
        self._handles = {}

    # ------------------------------------------------------------------ parameters
    def _check_shapes(self, p: dict):
        want = self.leaf_shapes()
        rbf = p.get("rbf_list", {})
        for name in self.frozen:
            if name in rbf:
                raise ValueError(f"params carry rbf_list.{name}, a constant of this net (fixed_centers={self.fixed_centers}, "
                                 f"fixed_width={self.fixed_width}): pass the tree of the live leaves {self.live_leaves()}")
        for g, n in self.live_leaves():
            if g not in p or n not in p[g]:
                raise ValueError(f"params lack {g}.{n}")
            got = tuple(p[g][n].shape)
            if want[n] != got:
                raise ValueError(f"params {n} has shape {got}, the model card implies {want[n]}")

    @staticmethod
    def _fingerprint(leaves, torch) -> tuple:
        """What ``bind`` remembers of the leaves it uploaded, to skip an identical upload.  A torch tensor is
        remembered as (the tensor OBJECT itself, data_ptr, _version): the strong reference keeps its id / storage from
        being recycled by a later, different tensor while it is cached, and any in-place write bumps ``_version``.  A
        NumPy array is remembered by CONTENT (a digest of its bytes, 0.3 MB at config 2), never by identity: ids and
        buffers of dropped temporaries are reused by CPython / the allocator -- exactly what
        ``net.apply(jax.tree.map(np.asarray, p), x)`` inside a ``pure_callback`` produces every step -- and a frozen
        array can be thawed, changed and frozen again."""
        fp = []
        for a in leaves:
            if isinstance(a, torch.Tensor):
                fp.append(("t", a, a.data_ptr(), a._version))
            else:
                arr = np.asarray(a)
                fp.append(("n", _digest(arr), arr.shape, str(arr.dtype)))
        return tuple(fp)

    @staticmethod
    def _same_fingerprint(old, new) -> bool:
        if old is None or len(old) != len(new):
            return False
        for o, n in zip(old, new):
            if o[0] != n[0]:
                return False
            if o[0] == "t":
                if o[1] is not n[1] or o[2:] != n[2:]:
                    return False
            elif o[1:] != n[1:]:
                return False
        return True

    def bind(self, params: dict) -> "WCRBFNet":
        """Uploads / re-packs the parameter pytree for the current device (irbfn_net_set_params)."""
        torch = _lib.require_gpu()
        lib = _lib.load()
        p = _inner(params)
        self._check_shapes(p)
        leaves = self._leaves(p, torch)
        dev = torch.cuda.current_device()
        fp = self._fingerprint(leaves, torch)
        if self._same_fingerprint(self._bound_fp.get(dev), fp):
            return self
        h = self._handle(torch)
        t = [to_device_f32(a, torch) for a in leaves]
        st = lib.irbfn_net_set_params(h, _ptr(t[0]), _ptr(t[1]), _ptr(t[2]), _ptr(t[3]), _stream_ptr(torch))
        _lib.check(st, "irbfn_net_set_params")
        self._keepalive[dev] = tuple(t)     # until the pack kernel has run
        self._bound_fp[dev] = fp
        return self

    # ------------------------------------------------------------------ forward
    def __call__(self, x):
        """Forward with the currently bound parameters: x[B,D] -> out[B,O]  (model.py:169-198)."""
        torch = _lib.require_gpu()
        lib = _lib.load()
        if torch.cuda.current_device() not in self._bound_fp:
            raise ValueError("WCRBFNet: no parameters bound on this device; call apply(params, x) or bind(params)")
        shape = tuple(x.shape)
        if len(shape) != 2 or shape[1] != self.in_features:
            raise ValueError(f"x must have shape (B, {self.in_features}), got {shape}")
        xd = to_device_f32(x, torch)
        B = shape[0]
        out = torch.empty((B, self.out_features), dtype=torch.float32, device=xd.device)
        if B:
            st = lib.irbfn_net_forward(self._handle(torch), _ptr(xd), _ptr(out), B, _stream_ptr(torch))
            _lib.check(st, "irbfn_net_forward")
        return like_input(out, x, torch)

    def apply(self, params: dict, x):
        """Drop-in for ``WCRBFNet.apply(params, x)`` / ``state.apply_fn(state.params, x)``
        (src/irbfn_mpc/irbfn_planner.py:31).  ``use_float64=True``: evaluated in float64 (``apply64``)."""
        if self.use_float64:
            return self.apply64(params, x)
        self._warn_if_float64(params)
        self.bind(params)
        return self(x)

    # ------------------------------------------------------------------ float64 mode
    def _warn_if_float64(self, params: dict):
        """A --use_float64 checkpoint (float64 centers / log_sigs) handed to the float32 path: say so once."""
        if self._warned_f64:
            return
        p = _inner(params)
        dts = {str(getattr(p[g][n], "dtype", "")) for g, n in self.live_leaves() if g in p and n in p[g]}
        if any("float64" in d for d in dts):
            import warnings
            warnings.warn("WCRBFNet: float64 parameter leaves are evaluated in float32 (within 1e-5 of a float64 run); construct "
                          "the net with use_float64=True for the float64 mode of the reference (--use_float64)", stacklevel=3)
            self._warned_f64 = True

    def _f64_card(self, torch):
        dev = torch.cuda.current_device()
        ent = self._f64.get(dev)
        if ent is None:
            ns, mr, lo, hi, delta, dr, nr = self._gate_tables(np.float64)
            tens = [torch.from_numpy(a).cuda() for a in (lo, hi, delta, dr if dr.size else np.zeros((1, 1), np.int32))]
            card = _lib.F64Card(self.in_features, self.num_regions, self.num_kernels, self.out_features,
                                _lib.BASIS_ENUM[self.basis_func], ns, mr, nr, tens[0].data_ptr(), tens[1].data_ptr(),
                                tens[2].data_ptr(), tens[3].data_ptr())
            ent = (card, tens, {})
            self._f64[dev] = ent
        return ent

    @staticmethod
    def _dev_f64(a, torch):
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(a)))
        return t.to(device=torch.device("cuda", torch.cuda.current_device()), dtype=torch.float64).contiguous()

    def apply64(self, params: dict, x):
        """``apply`` in float64 (the reference under --use_float64, scripts/train_nmpc.py:41-42) -> float64 [B,O]."""
        torch = _lib.require_gpu()
        lib = _lib.load()
        p = _inner(params)
        self._check_shapes(p)
        ent = self._f64_card(torch)
        card = ent[0]
        c, l, k, b = (self._dev_f64(a, torch) for a in self._leaves(p, torch, torch.float64))
        xd = self._dev_f64(x, torch)
        if xd.dim() != 2 or xd.shape[1] != self.in_features:
            raise ValueError(f"x must have shape (B, {self.in_features}), got {tuple(xd.shape)}")
        B = xd.shape[0]
        out = torch.empty((B, self.out_features), dtype=torch.float64, device=xd.device)
        nbytes = int(lib.irbfn_f64_workspace_bytes(C.byref(card), B, 0))
        ws = _grown_ws(ent[2], "ws", nbytes, torch, xd.device)
        st = lib.irbfn_f64_forward(C.byref(card), _ptr(c), _ptr(l), _ptr(k), _ptr(b), _ptr(xd), _ptr(out), B, _ptr(ws), nbytes,
                                   _stream_ptr(torch))
        _lib.check(st, "irbfn_f64_forward")
        return like_input(out, x, torch)

    F64_VJP_MAX_O = 16      # irbfn_f64_vjp's limit (include/irbfn_hip.h)

    def vjp64(self, params: dict, x, gout, out: Optional[dict] = None) -> dict:
        """Parameter VJP in float64 (``jax.value_and_grad`` of the reference under --use_float64) -> float64 gradient pytree.
        out: caller-provided float64 gradient leaves (e.g. views of the flat buffer of a float64 ``TrainState``)."""
        torch = _lib.require_gpu()
        lib = _lib.load()
        p = _inner(params)
        self._check_shapes(p)
        R, K, D, O = self.num_regions, self.num_kernels, self.in_features, self.out_features
        if O > self.F64_VJP_MAX_O:
            raise ValueError(f"the float64 VJP supports out_features <= {self.F64_VJP_MAX_O}, this net has {O}")
        ent = self._f64_card(torch)
        card = ent[0]
        c, l, k = (self._dev_f64(a, torch) for a in self._leaves(p, torch, torch.float64)[:3])
        xd, gd = self._dev_f64(x, torch), self._dev_f64(gout, torch)
        B = xd.shape[0]
        if tuple(gd.shape) != (B, self.out_features):
            raise ValueError(f"gout must have shape ({B}, {self.out_features}), got {tuple(gd.shape)}")
        # a frozen net: the full float64 VJP into scratch for the frozen leaves, the live ones returned
        full = {n: torch.empty(shp, dtype=torch.float64, device=xd.device) for n, shp in self.leaf_shapes().items()}
        if out is not None:
            o = _inner(out)
            for g, n in self.live_leaves():
                _check_out_leaf(o[g][n], full[n].shape, torch.float64, torch, "vjp64")
                full[n] = o[g][n]
        gc, gl, gk, gb = full["centers"], full["log_sigs"], full["kernel"], full["bias"]
        nbytes = int(lib.irbfn_f64_workspace_bytes(C.byref(card), B, 1))
        ws = _grown_ws(ent[2], "ws", nbytes, torch, xd.device)
        st = lib.irbfn_f64_vjp(C.byref(card), _ptr(c), _ptr(l), _ptr(k), _ptr(xd), _ptr(gd), _ptr(gc), _ptr(gl), _ptr(gk), _ptr(gb),
                               B, _ptr(ws), nbytes, _stream_ptr(torch))
        _lib.check(st, "irbfn_f64_vjp")
        conv = (lambda t: t) if out is not None else (lambda t: like_input(t, x, torch))
        return self._grad_tree(full, conv)

    def _grad_tree(self, leaves: dict, conv) -> dict:
        """The gradient pytree of the live leaves."""
        g = {}
        for grp, n in self.live_leaves():
            g.setdefault(grp, {})[n] = conv(leaves[n])
        return {"params": g}

    def gate(self, x):
        """``_region_activation`` (model.py:42-95): x[B,D] -> gamma[B,R]."""
        torch = _lib.require_gpu()
        lib = _lib.load()
        xd = to_device_f32(x, torch)
        B = xd.shape[0]
        g = torch.empty((B, self.num_regions), dtype=torch.float32, device=xd.device)
        if B:
            _lib.check(lib.irbfn_net_gate(self._handle(torch), _ptr(xd), _ptr(g), B, _stream_ptr(torch)),
                       "irbfn_net_gate")
        return like_input(g, x, torch)

    def hidden(self, params: dict, x):
        """The hidden layer h[b,k] = sum_r gamma[b,r] phi[b,r,k] of x[B,D] -> [B,K] float32 (``irbfn_net_hidden``): what
        ``apply`` multiplies by ``linear/kernel``, so ``apply(params, x) == hidden(params, x) @ kernel + bias`` up to float32
        rounding.  The design matrix of ``linear_fit.fit_linear``; the reference has no counterpart.  The float64 mode has
        no hidden-layer kernel: a ``use_float64`` net raises ``ValueError``."""
        if self.use_float64:
            raise ValueError(f"WCRBFNet.hidden: {NO_F64_HIDDEN}")
        torch = _lib.require_gpu()
        self._warn_if_float64(params)
        self.bind(params)
        shape = tuple(x.shape)
        if len(shape) != 2 or shape[1] != self.in_features:
            raise ValueError(f"x must have shape (B, {self.in_features}), got {shape}")
        xd = to_device_f32(x, torch)
        h = torch.empty((shape[0], self.num_kernels), dtype=torch.float32, device=xd.device)
        self._hidden_into(xd, h, torch)
        return like_input(h, x, torch)

    def _hidden_into(self, xd, h, torch):
        """irbfn_net_hidden of the bound parameters into the first K columns of the float32 cuda matrix h [B, ldh >= K]."""
        B = xd.shape[0]
        if B:
            st = _lib.load().irbfn_net_hidden(self._handle(torch), _ptr(xd), _ptr(h), h.stride(0), B, _stream_ptr(torch))
            _lib.check(st, "irbfn_net_hidden")

    # ------------------------------------------------------------------ backward
    def vjp(self, params: dict, x, gout, out: Optional[dict] = None) -> dict:
        """Parameter VJP: cotangent gout[B,O] -> gradient pytree (same structure as ``params``).
        Replaces ``jax.value_and_grad(loss_fn)(params)`` restricted to the network
        (scripts/train_nmpc.py:297-298).  The gradient w.r.t. x is ``vjp_x``."""
        if self.use_float64 and out is None:
            return self.vjp64(params, x, gout)
        torch = _lib.require_gpu()
        if out is not None and _inner(out)["linear"]["kernel"].dtype == torch.float64:
            return self.vjp64(params, x, gout, out=out)      # float64 leaves: the float64 VJP writes into them
        lib = _lib.load()
        self._warn_if_float64(params)
        self.bind(params)
        xd, gd = to_device_f32(x, torch), to_device_f32(gout, torch)
        B = xd.shape[0]
        if tuple(gd.shape) != (B, self.out_features):
            raise ValueError(f"gout must have shape ({B}, {self.out_features}), got {tuple(gd.shape)}")
        R, K, D, O = self.num_regions, self.num_kernels, self.in_features, self.out_features
        dev = xd.device
        shapes = self.leaf_shapes()
        full = {}
        if out is not None:      # caller-provided gradient leaves (e.g. views of one flat buffer)
            o = _inner(out)
            for g, n in self.live_leaves():
                _check_out_leaf(o[g][n], shapes[n], torch.float32, torch)
                full[n] = o[g][n]
        else:
            for g, n in self.live_leaves():
                full[n] = torch.empty(shapes[n], dtype=torch.float32, device=dev)
        gc, gl, gk, gb = (full.get(n) for n in ("centers", "log_sigs", "kernel", "bias"))
        h = self._handle(torch)
        nbytes = int(lib.irbfn_net_vjp_workspace_bytes(h, B))
        ws = _grown_ws(self._vjp_ws, dev.index, nbytes, torch, dev)
        if self.frozen:          # the frozen leaves are neither computed (K2g) nor written
            st = lib.irbfn_net_vjp_frozen(h, _ptr(xd), _ptr(gd), _ptr(gc) if gc is not None else None,
                                          _ptr(gl) if gl is not None else None, _ptr(gk), _ptr(gb), B, _ptr(ws), nbytes,
                                          _stream_ptr(torch))
            _lib.check(st, "irbfn_net_vjp_frozen")
        else:
            st = lib.irbfn_net_vjp(h, _ptr(xd), _ptr(gd), _ptr(gc), _ptr(gl), _ptr(gk), _ptr(gb), B, _ptr(ws), nbytes,
                                   _stream_ptr(torch))
            _lib.check(st, "irbfn_net_vjp")
        conv = (lambda t: t) if out is not None else (lambda t: like_input(t, x, torch))
        return self._grad_tree(full, conv)

    # ------------------------------------------------------------------ query VJP
    def _check_xg(self, xd, gd):
        B = xd.shape[0]
        if xd.dim() != 2 or xd.shape[1] != self.in_features:
            raise ValueError(f"x must have shape (B, {self.in_features}), got {tuple(xd.shape)}")
        if tuple(gd.shape) != (B, self.out_features):
            raise ValueError(f"gout must have shape ({B}, {self.out_features}), got {tuple(gd.shape)}")
        return B

    def vjp_x(self, params: dict, x, gout):
        """Query VJP: cotangent gout[B,O] -> gx[B,D] = ``jax.vjp(lambda x: apply(params, x), x)[1](gout)``, the RBF term and
        the term through the smooth region gate (``irbfn_net_vjp_x``; nothing in the reference takes this gradient).  Numpy in,
        numpy out; cuda in, cuda out.  ``use_float64=True``: evaluated in float64 (``vjp_x64``).  Frozen-leaf nets need
        nothing special: the kernel reads the bound images."""
        if self.use_float64:
            return self.vjp_x64(params, x, gout)
        torch = _lib.require_gpu()
        lib = _lib.load()
        self._warn_if_float64(params)
        self.bind(params)
        xd, gd = to_device_f32(x, torch), to_device_f32(gout, torch)
        B = self._check_xg(xd, gd)
        gx = torch.empty((B, self.in_features), dtype=torch.float32, device=xd.device)
        if B:
            st = lib.irbfn_net_vjp_x(self._handle(torch), _ptr(xd), _ptr(gd), _ptr(gx), B, _stream_ptr(torch))
            _lib.check(st, "irbfn_net_vjp_x")
        return like_input(gx, x, torch)

    def vjp_x64(self, params: dict, x, gout):
        """``vjp_x`` in float64 (``irbfn_f64_vjp_x``) -> float64 [B,D]; any out_features."""
        torch = _lib.require_gpu()
        lib = _lib.load()
        p = _inner(params)
        self._check_shapes(p)
        card = self._f64_card(torch)[0]
        c, l, k = (self._dev_f64(a, torch) for a in self._leaves(p, torch, torch.float64)[:3])
        xd, gd = self._dev_f64(x, torch), self._dev_f64(gout, torch)
        B = self._check_xg(xd, gd)
        gx = torch.empty((B, self.in_features), dtype=torch.float64, device=xd.device)
        st = lib.irbfn_f64_vjp_x(C.byref(card), _ptr(c), _ptr(l), _ptr(k), _ptr(xd), _ptr(gd), _ptr(gx), B, None, 0,
                                 _stream_ptr(torch))
        _lib.check(st, "irbfn_f64_vjp_x")
        return like_input(gx, x, torch)

    def input_jacobian(self, params: dict, x):
        """d apply(params, x)[b, o] / d x[b, d] -> [B, O, D]: the sensitivity of every output to the query.  Built from
        ``out_features`` one-hot cotangents, i.e. O launches of ``vjp_x`` (fine for the reference's O <= 10)."""
        torch = _lib.require_gpu()
        f64 = self.use_float64
        xd = self._dev_f64(x, torch) if f64 else to_device_f32(x, torch)
        B, O = xd.shape[0], self.out_features
        jac = torch.empty((B, O, self.in_features), dtype=xd.dtype, device=xd.device)
        g = torch.zeros((B, O), dtype=xd.dtype, device=xd.device)
        for o in range(O):
            g[:, o] = 1.0
            jac[:, o, :] = self.vjp_x(params, xd, g)
            g[:, o] = 0.0
        return like_input(jac, x, torch)

    def last_launch(self) -> dict:
        torch = _lib.require_gpu()
        lib = _lib.load()
        buf = C.create_string_buffer(128)
        g, b = C.c_int(0), C.c_int(0)
        lib.irbfn_net_last_launch(self._handle(torch), buf, 128, C.byref(g), C.byref(b))
        return {"kernel": buf.value.decode(), "grid": g.value, "block": b.value}


def _no_frozen(cls_name: str, kw: dict):
    if kw.get("centers") is not None and (kw.get("fixed_centers") or kw.get("fixed_width")):
        raise NotImplementedError(f"{cls_name} with fixed centres / widths is not supported (WCRBFNet is)")


class DeeperWCRBFNet:
    """``DeeperWCRBFNet`` of the reference (src/irbfn_mpc/model.py:201-289): the RBF stage followed by
    Dense(64) -> relu -> Dense(64) -> relu -> Dense(out_features).  Parameter pytree (checkpoint layout):
    ``{"rbf_list": {centers, log_sigs}, "linear_pre1": {kernel[K,64], bias}, "linear_pre2":
    {kernel[64,64], bias}, "linear": {kernel[64,O], bias}}``.  The RBF stage + linear_pre1 run in the fused RBF
    kernel (64-wide Dense), the rest in ``irbfn_mlp_head_forward``; ``vjp`` = ``irbfn_mlp_head_vjp`` followed by the
    RBF-stage VJP seeded with the cotangent of linear_pre1's output."""

    HIDDEN = 64          # model.py:254-255

    def __init__(self, in_features, out_features, num_kernels, basis_func, num_regions, lower_bounds,
                 upper_bounds, dimension_ranges, activation_idx, delta, use_float64: bool = False, **_unused):
        _no_frozen("DeeperWCRBFNet", _unused)
        if use_float64:
            raise ValueError("DeeperWCRBFNet has no float64 mode (its MLP head runs in float32); build it with use_float64=False")
        self.out_features = int(out_features)
        self.in_features = int(in_features)
        self.stage = WCRBFNet(in_features=in_features, out_features=self.HIDDEN, num_kernels=num_kernels,
                              basis_func=basis_func, num_regions=num_regions, lower_bounds=lower_bounds,
                              upper_bounds=upper_bounds, dimension_ranges=dimension_ranges,
                              activation_idx=activation_idx, delta=delta)
        self._fp = None
        self._head = None

    @classmethod
    def from_config(cls, cfg) -> "DeeperWCRBFNet":
        cfg = _load_card(cfg)
        return cls(**{k: cfg[k] for k in _CFG_FIELDS}, use_float64=bool(cfg.get("use_float64", False)))

    LEAVES = (("rbf_list", "centers"), ("rbf_list", "log_sigs"), ("linear_pre1", "kernel"), ("linear_pre1", "bias"),
              ("linear_pre2", "kernel"), ("linear_pre2", "bias"), ("linear", "kernel"), ("linear", "bias"))

    def live_leaves(self) -> tuple:
        """(group, name) of the eight leaves, in the order of the flat training buffers (distributed.flatten_params)."""
        return self.LEAVES

    def group_leaf_shapes(self) -> dict:
        """{(group, name): shape} of the parameter pytree."""
        R, K, D, H, O = self.stage.num_regions, self.stage.num_kernels, self.in_features, self.HIDDEN, self.out_features
        return {("rbf_list", "centers"): (R, K, D), ("rbf_list", "log_sigs"): (R, K), ("linear_pre1", "kernel"): (K, H),
                ("linear_pre1", "bias"): (H,), ("linear_pre2", "kernel"): (H, H), ("linear_pre2", "bias"): (H,),
                ("linear", "kernel"): (H, O), ("linear", "bias"): (O,)}

    def _check_shapes(self, p: dict):
        for (g, n), shp in self.group_leaf_shapes().items():
            if g not in p or n not in p[g]:
                raise ValueError(f"params lack {g}.{n}")
            if tuple(p[g][n].shape) != shp:
                raise ValueError(f"params {g}.{n} has shape {tuple(p[g][n].shape)}, the model card implies {shp}")

    def _stage_and_head(self, params: dict, xd, torch):
        """(h1, [w2, b2, w3, b3]) as device tensors: the stage output linear_pre1(rbf_out) [B, 64] (model.py:283) and the
        head's leaves, shapes checked."""
        p = _inner(params)
        H, O = self.HIDDEN, self.out_features
        for name, shp in (("linear_pre2", (H, H)), ("linear", (H, O))):
            if tuple(p[name]["kernel"].shape) != shp:
                raise ValueError(f"params {name}.kernel has shape {tuple(p[name]['kernel'].shape)}, expected {shp}")
        stage_params = {"rbf_list": p["rbf_list"], "linear": p["linear_pre1"]}
        h1 = self.stage.apply(stage_params, xd)                     # linear_pre1(rbf_out)   model.py:283
        head = [to_device_f32(a, torch) for a in (p["linear_pre2"]["kernel"], p["linear_pre2"]["bias"],
                                                  p["linear"]["kernel"], p["linear"]["bias"])]
        return h1, head

    def _forward(self, params: dict, xd, torch, lib):
        """(out, h1) as device tensors: h1 = linear_pre1(rbf_out) [B, 64] (model.py:283), out the head's output."""
        H, O = self.HIDDEN, self.out_features
        h1, head = self._stage_and_head(params, xd, torch)
        B = xd.shape[0]
        out = torch.empty((B, O), dtype=torch.float32, device=xd.device)
        st = lib.irbfn_mlp_head_forward(_ptr(h1), _ptr(head[0]), _ptr(head[1]), _ptr(head[2]), _ptr(head[3]), _ptr(out),
                                        B, H, H, O, _stream_ptr(torch))
        _lib.check(st, "irbfn_mlp_head_forward")
        return out, h1

    def apply(self, params: dict, x):
        torch = _lib.require_gpu()
        out, _ = self._forward(params, to_device_f32(x, torch), torch, _lib.load())
        return like_input(out, x, torch)

    def apply_with_hidden(self, params: dict, x):
        """``apply`` that also returns the stage output h1 [B, 64] (linear_pre1's output), which ``vjp(h1=)`` reuses instead
        of running the RBF stage a second time.  -> (out [B, O], h1 [B, 64]), in the flavour of x."""
        torch = _lib.require_gpu()
        out, h1 = self._forward(params, to_device_f32(x, torch), torch, _lib.load())
        return like_input(out, x, torch), like_input(h1, x, torch)

    def _head_backward(self, params: dict, x, gout, h1, what: str, head_out=None):
        """The head's backward (``irbfn_mlp_head_vjp``) -> (stage_params, xd, gh1, (gw2, gb2, gw3, gb3)): gh1 [B, 64] is the
        cotangent of linear_pre1's output, the seed of the stage's VJPs.  h1: the stage output, computed here if None.
        head_out: the caller's four gradient leaves of the head; fresh tensors otherwise."""
        torch = _lib.require_gpu()
        lib = _lib.load()
        p = _inner(params)
        H, O = self.HIDDEN, self.out_features
        stage_params = {"rbf_list": p["rbf_list"], "linear": p["linear_pre1"]}
        xd, gd = to_device_f32(x, torch), to_device_f32(gout, torch)
        B = xd.shape[0]
        if tuple(gd.shape) != (B, O):
            raise ValueError(f"gout must have shape ({B}, {O})")
        if h1 is None:
            h1 = self.stage.apply(stage_params, xd)
        elif not isinstance(h1, torch.Tensor) or tuple(h1.shape) != (B, H) or h1.dtype != torch.float32 or not h1.is_cuda \
                or not h1.is_contiguous():
            raise ValueError(f"{what} h1= must be the contiguous float32 cuda stage output [{B}, {H}] of apply_with_hidden")
        w2, b2, w3 = (to_device_f32(a, torch) for a in (p["linear_pre2"]["kernel"], p["linear_pre2"]["bias"], p["linear"]["kernel"]))
        dev = xd.device
        new = lambda *shp: torch.empty(shp, dtype=torch.float32, device=dev)
        gw2, gb2, gw3, gb3 = head_out if head_out is not None else (new(H, H), new(H), new(H, O), new(O))
        gh1 = new(B, H)
        nbytes = int(lib.irbfn_mlp_head_vjp_workspace_bytes(H, H, O))
        if nbytes < 0:
            _lib.check(nbytes, "irbfn_mlp_head_vjp_workspace_bytes")
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        st = lib.irbfn_mlp_head_vjp(_ptr(h1), _ptr(w2), _ptr(b2), _ptr(w3), _ptr(gd), _ptr(gh1), _ptr(gw2), _ptr(gb2),
                                    _ptr(gw3), _ptr(gb3), B, H, H, O, _ptr(ws), nbytes, _stream_ptr(torch))
        _lib.check(st, "irbfn_mlp_head_vjp")
        return stage_params, xd, gh1, (gw2, gb2, gw3, gb3)

    def vjp_x(self, params: dict, x, gout, h1=None):
        """Query VJP of the whole model: gout[B,O] -> gx[B,D].  The head backward gives the cotangent of linear_pre1's output
        (``irbfn_mlp_head_vjp``; its parameter gradients are by-products here), the stage's ``vjp_x`` takes it to x.
        h1: the stage output of ``apply_with_hidden``, as for ``vjp``."""
        torch = _lib.require_gpu()
        stage_params, xd, gh1, _ = self._head_backward(params, x, gout, h1, "vjp_x")
        return like_input(self.stage.vjp_x(stage_params, xd, gh1), x, torch)

    def vjp(self, params: dict, x, gout, out: Optional[dict] = None, h1=None, stage_vjp_kernel: Optional[int] = None) -> dict:
        """Parameter VJP of the whole model: cotangent gout[B,O] -> gradient pytree with the structure of ``params``
        (what ``jax.value_and_grad`` returns for a DeeperWCRBFNet, scripts/train_nmpc_frenet.py:388-389,416-417).

        out: caller-provided contiguous float32 cuda leaves (e.g. views of a flat buffer), written and returned.
        h1: the stage output of ``apply_with_hidden`` for these params and x: the RBF stage is not run again.
        stage_vjp_kernel: ``_lib.VJP_*`` for the stage VJP of this call only; the stage's option is restored afterwards."""
        torch = _lib.require_gpu()
        lib = _lib.load()
        head_out = stage_out = None
        if out is not None:
            o = _inner(out)
            for (g, n), shp in self.group_leaf_shapes().items():
                _check_out_leaf(o[g][n], shp, torch.float32, torch)
            head_out = (o["linear_pre2"]["kernel"], o["linear_pre2"]["bias"], o["linear"]["kernel"], o["linear"]["bias"])
            stage_out = {"rbf_list": o["rbf_list"], "linear": o["linear_pre1"]}
        stage_params, xd, gh1, (gw2, gb2, gw3, gb3) = self._head_backward(params, x, gout, h1, "vjp", head_out)
        if stage_vjp_kernel is None:
            gs = self.stage.vjp(stage_params, xd, gh1, out=stage_out)["params"]
        else:                    # this call only: the descriptor's own choice is put back whatever happens
            h = self.stage._handle(torch)
            prev = C.c_int(0)
            _lib.check(lib.irbfn_net_get_option(h, _lib.OPTIONS["vjp_kernel"], C.byref(prev)), "irbfn_net_get_option")
            _lib.check(lib.irbfn_net_set_option(h, _lib.OPTIONS["vjp_kernel"], int(stage_vjp_kernel)),
                       f"irbfn_net_set_option(vjp_kernel={stage_vjp_kernel})")
            try:
                gs = self.stage.vjp(stage_params, xd, gh1, out=stage_out)["params"]
            finally:
                lib.irbfn_net_set_option(h, _lib.OPTIONS["vjp_kernel"], prev.value)
        conv = (lambda t: t) if out is not None else (lambda t: like_input(t, x, torch))
        return {"params": {"rbf_list": {k: conv(v) for k, v in gs["rbf_list"].items()},
                           "linear_pre1": {k: conv(v) for k, v in gs["linear"].items()},
                           "linear_pre2": {"kernel": conv(gw2), "bias": conv(gb2)},
                           "linear": {"kernel": conv(gw3), "bias": conv(gb3)}}}


class ClusterWCRBFNet:
    """``ClusterWCRBFNet`` of the reference (src/irbfn_mpc/model.py:341-414): R RBF layers mixed by a learned
    softmax gate ``softmax(Dense(R)(x))`` instead of the tanh indicator.  Parameter pytree: ``{"rbf_list":
    {centers[R,K,D], log_sigs[R,K]}, "linear": {kernel[K,O], bias[O]}, "cluster": {kernel[D,R], bias[R]}}``.
    ``apply`` returns ``(out, logits)`` like the reference module; ``vjp`` is the parameter VJP of both outputs (what
    ``train_step_fullint_withcluster`` differentiates, scripts/train_nmpc_frenet.py:424-453).  The reference trains it at
    R = 500, D = 8, O = 10 (scripts/ckpts/dnmpc_500_clusters/checkpoint_0, K = 10;
    dnmpc_500_clusters_numk50/checkpoint_100, K = 50); those checkpoints are not in this repository, so parity is
    against the oracle restatement on synthetic parameters at their shapes (tests/test_gpu_cluster_scale.py)."""

    def __init__(self, in_features, out_features, num_kernels, basis_func, num_regions, use_float64: bool = False, **_unused):
        _no_frozen("ClusterWCRBFNet", _unused)
        if use_float64:
            raise ValueError("ClusterWCRBFNet has no float64 mode (its softmax gate runs in float32); build it with use_float64=False")
        self.in_features, self.out_features = int(in_features), int(out_features)
        self.num_regions = int(num_regions)
        self._gate_ws = {}
        # descriptor with R regions and no gate tables: the region weights come from the softmax gate
        self.stage = WCRBFNet(in_features=in_features, out_features=out_features, num_kernels=num_kernels,
                              basis_func=basis_func, num_regions=num_regions, lower_bounds=[], upper_bounds=[],
                              dimension_ranges=[], activation_idx=[], delta=[])

    def set_options(self, **opts) -> "ClusterWCRBFNet":
        """``WCRBFNet.set_options`` of the RBF stage, e.g. ``fwd_gamma_kernel=_lib.FWDG_K1G``: ``apply`` and the planning
        tick on the matrix-core kernel ``rbf_fwd_f16gram_gamma`` / ``rbf_tick_f16gram_gamma``."""
        self.stage.set_options(**opts)
        return self

    def _bind_and_gate(self, params: dict, xd, torch, lib):
        """Binds the stage to the RBF leaves and runs the softmax gate (model.py:402-404) -> (logits, gamma), [B, R] each."""
        return self._gate(params, xd, torch, lib)[:2]

    def _gate(self, params: dict, xd, torch, lib):
        """``_bind_and_gate`` that also returns the gate's kernel on the device -> (logits, gamma, wc)."""
        p = _inner(params)
        D, R = self.in_features, self.num_regions
        if tuple(p["cluster"]["kernel"].shape) != (D, R) or tuple(p["cluster"]["bias"].shape) != (R,):
            raise ValueError(f"params cluster.kernel / bias must be [{D},{R}] / [{R}]")
        self.stage.bind({"rbf_list": p["rbf_list"], "linear": p["linear"]})
        B = xd.shape[0]
        if tuple(xd.shape) != (B, D):
            raise ValueError(f"x must be [B, {D}]")
        wc, bc = to_device_f32(p["cluster"]["kernel"], torch), to_device_f32(p["cluster"]["bias"], torch)
        logits = torch.empty((B, R), dtype=torch.float32, device=xd.device)
        gamma = torch.empty((B, R), dtype=torch.float32, device=xd.device)
        st = lib.irbfn_cluster_gate(_ptr(xd), _ptr(wc), _ptr(bc), _ptr(logits), _ptr(gamma), B, D, R, _stream_ptr(torch))
        _lib.check(st, "irbfn_cluster_gate")
        return logits, gamma, wc

    def apply(self, params: dict, x):
        torch = _lib.require_gpu()
        lib = _lib.load()
        xd = to_device_f32(x, torch)
        logits, gamma = self._bind_and_gate(params, xd, torch, lib)
        B, O = xd.shape[0], self.out_features
        out = torch.empty((B, O), dtype=torch.float32, device=xd.device)
        st = lib.irbfn_net_forward_gamma(self.stage._handle(torch), _ptr(xd), _ptr(gamma), _ptr(out), B, _stream_ptr(torch))
        _lib.check(st, "irbfn_net_forward_gamma")
        return like_input(out, x, torch), like_input(logits, x, torch)

    def vjp_x(self, params: dict, x, gout, glogits=None):
        """Query VJP of ``apply``: cotangents gout[B,O] of ``out`` and (optionally) glogits[B,R] of ``logits`` -> gx[B,D].
        ``irbfn_net_vjp_x_gamma`` gives the RBF term at fixed region weights and the cotangent of those weights; the softmax
        backward and the [B,R] x [R,D] product with the gate's kernel run in torch on the device."""
        torch = _lib.require_gpu()
        lib = _lib.load()
        D, R, O = self.in_features, self.num_regions, self.out_features
        xd, gd = to_device_f32(x, torch), to_device_f32(gout, torch)
        B = xd.shape[0]
        if tuple(xd.shape) != (B, D) or tuple(gd.shape) != (B, O):
            raise ValueError(f"x must be [B, {D}] and gout [B, {O}]")
        logits, gamma, wc = self._gate(params, xd, torch, lib)
        dgamma = torch.empty((B, R), dtype=torch.float32, device=xd.device)
        gx = torch.empty((B, D), dtype=torch.float32, device=xd.device)
        if B:
            stream = _stream_ptr(torch)
            st = lib.irbfn_net_vjp_x_gamma(self.stage._handle(torch), _ptr(xd), _ptr(gamma), _ptr(gd), _ptr(gx), _ptr(dgamma), B,
                                           stream)
            _lib.check(st, "irbfn_net_vjp_x_gamma")
            # softmax backward (model.py:402-404), then logits = x Wc + bc
            dlogits = gamma * (dgamma - (gamma * dgamma).sum(dim=1, keepdim=True))
            if glogits is not None:
                gl_in = to_device_f32(glogits, torch)
                if tuple(gl_in.shape) != (B, R):
                    raise ValueError(f"glogits must be [B, {R}]")
                dlogits = dlogits + gl_in
            gx = gx + dlogits @ wc.t()
        return like_input(gx, x, torch)

    def vjp(self, params: dict, x, gout, glogits=None, out: Optional[dict] = None) -> dict:
        """Parameter VJP of ``apply``: cotangents gout[B,O] of ``out`` and (optionally) glogits[B,R] of ``logits`` ->
        gradient pytree with the structure of ``params`` (rbf_list / linear / cluster).  The gate is recomputed (one
        [B,D]x[D,R] pass), K2 runs with the softmax weights, the cotangent of those weights comes from
        ``irbfn_net_vjp_gamma`` and goes back through softmax + Dense in ``irbfn_cluster_gate_vjp``."""
        torch = _lib.require_gpu()
        lib = _lib.load()
        D, R, O, K = self.in_features, self.num_regions, self.out_features, self.stage.num_kernels
        if O > 16:
            raise ValueError("ClusterWCRBFNet.vjp supports out_features <= 16 (the reference trains it with 10)")
        xd, gd = to_device_f32(x, torch), to_device_f32(gout, torch)
        B = xd.shape[0]
        if tuple(xd.shape) != (B, D) or tuple(gd.shape) != (B, O):
            raise ValueError(f"x must be [B, {D}] and gout [B, {O}]")
        gl_in = None
        if glogits is not None:
            gl_in = to_device_f32(glogits, torch)
            if tuple(gl_in.shape) != (B, R):
                raise ValueError(f"glogits must be [B, {R}]")
        dev = xd.device
        shapes = {"centers": (R, K, D), "log_sigs": (R, K), "kernel": (K, O), "bias": (O,), "ckernel": (D, R), "cbias": (R,)}
        if out is not None:
            o = _inner(out)
            leaves = {"centers": o["rbf_list"]["centers"], "log_sigs": o["rbf_list"]["log_sigs"], "kernel": o["linear"]["kernel"],
                      "bias": o["linear"]["bias"], "ckernel": o["cluster"]["kernel"], "cbias": o["cluster"]["bias"]}
            for n, t in leaves.items():
                _check_out_leaf(t, shapes[n], torch.float32, torch)
        else:
            leaves = {n: torch.empty(shp, dtype=torch.float32, device=dev) for n, shp in shapes.items()}
        logits, gamma = self._bind_and_gate(params, xd, torch, lib)         # after every check of the arguments
        dgamma = torch.empty((B, R), dtype=torch.float32, device=dev)
        stream = _stream_ptr(torch)
        h = self.stage._handle(torch)
        nbytes = int(lib.irbfn_net_vjp_workspace_bytes(h, B))
        ws = _grown_ws(self.stage._vjp_ws, dev.index, nbytes, torch, dev)
        st = lib.irbfn_net_vjp_gamma(h, _ptr(xd), _ptr(gamma), _ptr(gd), _ptr(leaves["centers"]), _ptr(leaves["log_sigs"]),
                                     _ptr(leaves["kernel"]), _ptr(leaves["bias"]), _ptr(dgamma), B, _ptr(ws), nbytes, stream)
        _lib.check(st, "irbfn_net_vjp_gamma")
        gbytes = int(lib.irbfn_cluster_gate_vjp_workspace_bytes(D, R))
        gws = _grown_ws(self._gate_ws, dev.index, gbytes, torch, dev)
        st = lib.irbfn_cluster_gate_vjp(_ptr(xd), _ptr(gamma), _ptr(dgamma), _ptr(gl_in) if gl_in is not None else None,
                                        _ptr(logits), _ptr(leaves["ckernel"]), _ptr(leaves["cbias"]), B, D, R, _ptr(gws), gbytes,
                                        stream)
        _lib.check(st, "irbfn_cluster_gate_vjp")
        conv = (lambda t: t) if out is not None else (lambda t: like_input(t, x, torch))
        return {"params": {"rbf_list": {"centers": conv(leaves["centers"]), "log_sigs": conv(leaves["log_sigs"])},
                           "linear": {"kernel": conv(leaves["kernel"]), "bias": conv(leaves["bias"])},
                           "cluster": {"kernel": conv(leaves["ckernel"]), "bias": conv(leaves["cbias"])}}}


class _State:
    """Minimal stand-in of flax's TrainState for ``pred_step``: ``apply_fn`` + ``params``."""

    def __init__(self, apply_fn, params):
        self.apply_fn, self.params = apply_fn, params


def make_state(net: WCRBFNet, params: dict) -> _State:
    return _State(net.apply, params)


def pred_step(state, x):
    """``pred_step(state, x)`` of src/irbfn_mpc/irbfn_planner.py:29-32."""
    return state.apply_fn(state.params, x)
