"""Float64 NumPy statement of the Dense head of DeeperWCRBFNet (src/irbfn_mpc/model.py:254-256, 283-287) and of its adjoint,
written by hand; the per-element cancellation scales the head tests state their bounds against; the input generators of
those tests; and thin callers of the head's C ABI (``irbfn_mlp_head_forward`` / ``irbfn_mlp_head_vjp``) with h1 given as data.

    a1 = max(h1, 0)        z2 = a1 W2 + b2        a2 = max(z2, 0)        out = a2 W3 + b3
    t = g W3^T             dz = [z2 > 0] t        gh1 = [h1 > 0] (dz W2^T)
    gw2 = a1^T dz          gb2 = sum_b dz         gw3 = a2^T g           gb3 = sum_b g

The strict ``>`` is jax.nn.relu's convention: relu'(0) = 0.  ``np.maximum`` propagates NaN, as jnp.maximum does.  Nothing here
goes through the oracle's torch branch.

Scales (every quantity below is >= 0; an evaluation in float32 with n-term sums in any order is within n u (1 + n u) of them):
    S2   = a1 |W2| + |b2|                               the terms of z2
    Sout = a2 |W3| + |b3| + S2 |W3|                     the terms of out + what the rounding of z2 brings
    G    = |g| |W3|^T                                   the terms of t
    Sgh1 = |dz| |W2|^T + G |W2|^T                       the terms of gh1 + what the rounding of t brings
    Sgw2 = a1^T |dz| + a1^T ([z2 > 0] G)                the terms of gw2 + row by row what the rounding of dz brings
    Sgb2 = sum_b |dz| + sum_b [z2 > 0] G
    Sgw3 = a2^T |g| + ([z2 > 0] S2)^T |g|               the terms of gw3 + row by row what the rounding of a2 brings
    Sgb3 = sum_b |g|                                    g is data: nothing propagated
"""
import numpy as np

U32 = 2.0 ** -24                     # unit round-off of float32
H = 64                               # Dense(64), Dense(64): model.py:254-255
LEAF_NAMES = ("gw2", "gb2", "gw3", "gb3")


def any_order_bound(n):
    """Worst case of an n-term float32 sum of products in any order, relative to the sum of the absolute terms."""
    return n * U32 * (1.0 + n * U32)


def _f64(*a):
    return [np.asarray(v, np.float64) for v in a]


def forward64(h1, W2, b2, W3, b3):
    """-> dict(a1, z2, a2, out, S2, Sout), float64."""
    h1, W2, b2, W3, b3 = _f64(h1, W2, b2, W3, b3)
    with np.errstate(invalid="ignore", over="ignore"):
        a1 = np.maximum(h1, 0.0)
        z2 = a1 @ W2 + b2
        a2 = np.maximum(z2, 0.0)
        out = a2 @ W3 + b3
        S2 = a1 @ np.abs(W2) + np.abs(b2)
        Sout = a2 @ np.abs(W3) + np.abs(b3) + S2 @ np.abs(W3)
    return dict(a1=a1, z2=z2, a2=a2, out=out, S2=S2, Sout=Sout)


def backward64(h1, W2, b2, W3, g):
    """The hand-written adjoint -> dict(gh1, gw2, gb2, gw3, gb3, dz, z2, S2, G and the scales Sgh1, Sgw2, Sgb2, Sgw3, Sgb3)."""
    h1, W2, b2, W3, g = _f64(h1, W2, b2, W3, g)
    f = forward64(h1, W2, b2, W3, np.zeros(W3.shape[1]))
    a1, z2, a2, S2 = f["a1"], f["z2"], f["a2"], f["S2"]
    with np.errstate(invalid="ignore", over="ignore"):
        t = g @ W3.T
        dz = np.where(z2 > 0.0, t, 0.0)
        gh1 = np.where(h1 > 0.0, dz @ W2.T, 0.0)
        gw2, gb2 = a1.T @ dz, dz.sum(0)
        gw3, gb3 = a2.T @ g, g.sum(0)
        G = np.abs(g) @ np.abs(W3).T
        Gm = np.where(z2 > 0.0, G, 0.0)
        S2m = np.where(z2 > 0.0, S2, 0.0)
        Sgh1 = np.abs(dz) @ np.abs(W2).T + G @ np.abs(W2).T
        Sgw2 = a1.T @ np.abs(dz) + a1.T @ Gm
        Sgb2 = np.abs(dz).sum(0) + Gm.sum(0)
        Sgw3 = a2.T @ np.abs(g) + S2m.T @ np.abs(g)
        Sgb3 = np.abs(g).sum(0)
    return dict(gh1=gh1, gw2=gw2, gb2=gb2, gw3=gw3, gb3=gb3, dz=dz, z2=z2, S2=S2, G=G,
                Sgh1=Sgh1, Sgw2=Sgw2, Sgb2=Sgb2, Sgw3=Sgw3, Sgb3=Sgb3)


# ---------------------------------------------------------------- plain float32 evaluations (the yardstick of the factor 4)
def _chain32(a, W, b):
    """a W + b in float32, the terms added one at a time in index order (a product, then an addition: two roundings a term)."""
    acc = np.broadcast_to(np.asarray(b, np.float32), (a.shape[0], W.shape[1])).copy()
    for i in range(W.shape[0]):
        acc += a[:, i:i + 1] * W[i]
    return acc


def forward32(h1, W2, b2, W3, b3):
    h1, W2, b2, W3, b3 = (np.asarray(v, np.float32) for v in (h1, W2, b2, W3, b3))
    a1 = np.maximum(h1, np.float32(0))
    z2 = _chain32(a1, W2, b2)
    a2 = np.maximum(z2, np.float32(0))
    return dict(a1=a1, z2=z2, a2=a2, out=_chain32(a2, W3, b3))


def backward32(h1, W2, b2, W3, g):
    """float32 NumPy: gh1 with index-order chains; the four summed leaves in their natural form (``a1.T @ dz``, ``sum(0)``)."""
    h1, W2, b2, W3, g = (np.asarray(v, np.float32) for v in (h1, W2, b2, W3, g))
    f = forward32(h1, W2, b2, W3, np.zeros(W3.shape[1], np.float32))
    zero = np.float32(0)
    t = _chain32(g, np.ascontiguousarray(W3.T), np.zeros(H, np.float32))
    dz = np.where(f["z2"] > 0, t, zero)
    gh1 = np.where(h1 > 0, _chain32(dz, np.ascontiguousarray(W2.T), np.zeros(H, np.float32)), zero)
    return dict(gh1=gh1, gw2=f["a1"].T @ dz, gb2=dz.sum(0), gw3=f["a2"].T @ g, gb3=g.sum(0), z2=f["z2"])


def worst_ratio(got, ref, scale):
    """max |got - ref| / scale over the elements with a positive scale; an element of scale 0 must be exact."""
    got, ref, scale = _f64(got, ref, scale)
    err = np.abs(got - ref)
    live = scale > 0
    assert (err[~live] == 0).all(), "an element whose every term is 0 is not 0"
    return float((err[live] / scale[live]).max()) if live.any() else 0.0


# ---------------------------------------------------------------- generators
def lattice_case(B, O, seed):
    """h1, W2, W3, g in {-1, 0, 1}, b2, b3 in {-2 .. 2}: every product and every partial sum in any order is a small integer,
    so every correct float32 evaluation returns the float64 result exactly (see ``lattice_is_exact``)."""
    rng = np.random.default_rng(seed)
    tri = lambda *s: rng.integers(-1, 2, size=s).astype(np.float32)
    bias = lambda n: rng.integers(-2, 3, size=n).astype(np.float32)
    return dict(h1=tri(B, H), W2=tri(H, H), b2=bias(H), W3=tri(H, O), b3=bias(O), g=tri(B, O))


def lattice_largest_sum(c):
    """An upper bound of the largest sum of absolute terms of any intermediate or result of the head's forward and backward
    on the case: the largest scale (each scale holds the absolute terms of its quantity, and more)."""
    f = forward64(c["h1"], c["W2"], c["b2"], c["W3"], c["b3"])
    r = backward64(c["h1"], c["W2"], c["b2"], c["W3"], c["g"])
    sums = [f["S2"], f["Sout"]] + [r[k] for k in ("G", "Sgh1", "Sgw2", "Sgb2", "Sgw3", "Sgb3")]
    return max(float(s.max()) for s in sums if s.size)


def lattice_is_exact(c):
    """The condition under which float32 == float64 on a lattice case: all sums of absolute terms stay below 2^24."""
    return lattice_largest_sum(c) < 2.0 ** 24


MASK_MARGIN = 4 * 65 * U32           # rows with some |z2| <= MASK_MARGIN * S2 are redrawn: float32 and float64 masks may differ there
REDRAW_CAP = 0.01


def near_kink_rows(h1, W2, b2):
    f = forward64(h1, W2, b2, np.zeros((H, 1)), np.zeros(1))
    return (np.abs(f["z2"]) <= MASK_MARGIN * f["S2"]).any(axis=1)


def real_case(B, O, seed, w3_col_spread=False):
    """float32-rounded normals: h1, g ~ N(0, 1), W ~ N(0, 1) / 8, biases ~ 0.1 N(0, 1); w3_col_spread: the columns of W3 scaled
    by 10^e, e spread evenly over [-3, 3].  Rows with a z2 entry within MASK_MARGIN of the kink are redrawn until none is left.
    -> (case, share of rows that were redrawn at least once)."""
    rng = np.random.default_rng(seed)
    nrm = lambda s, *shape: (rng.normal(size=shape) * s).astype(np.float32)
    W2, b2, W3, b3 = nrm(1 / 8, H, H), nrm(0.1, H), nrm(1 / 8, H, O), nrm(0.1, O)
    if w3_col_spread:
        W3 = (W3 * (10.0 ** np.linspace(-3, 3, O))[None, :]).astype(np.float32)
    h1, g = nrm(1.0, B, H), nrm(1.0, B, O)
    bad = near_kink_rows(h1, W2, b2)
    redrawn = bad.copy()
    while bad.any():
        idx = np.flatnonzero(bad)
        h1[idx] = nrm(1.0, idx.size, H)
        bad[idx] = near_kink_rows(h1[idx], W2, b2)
    return dict(h1=h1, W2=W2, b2=b2, W3=W3, b3=b3, g=g), float(redrawn.mean())


def keep_clear_rows(h1, W2, b2, B):
    """For h1 rows that come from a stage (the golden net): the first B rows clear of the kink, and the share of the rows
    passed over on the way (the redrawn ones).  h1 must hold enough rows."""
    bad = near_kink_rows(h1, W2, b2)
    good = np.flatnonzero(~bad)
    assert good.size >= B, "draw more rows"
    last = good[B - 1]
    return good[:B], float(bad[:last + 1].sum()) / B


# ---------------------------------------------------------------- the ABI, h1 given as data
def _ptr(t):
    import ctypes as C
    return C.c_void_p(t.data_ptr() if t is not None else None)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def gpu_forward(h1, W2, b2, W3, b3):
    """``irbfn_mlp_head_forward`` on device tensors -> out [B, O] (device)."""
    import torch
    from irbfn_amd import _lib
    from irbfn_amd.model import _stream_ptr
    B, O = h1.shape[0], W3.shape[1]
    out = torch.full((B, O), float("nan"), dtype=torch.float32, device="cuda")
    st = _lib.load().irbfn_mlp_head_forward(_ptr(h1), _ptr(W2), _ptr(b2), _ptr(W3), _ptr(b3), _ptr(out), B, H, H, O, _stream_ptr(torch))
    assert st == 0, st
    return out


def gpu_vjp(h1, W2, b2, W3, g, out=None, ws=None):
    """``irbfn_mlp_head_vjp`` on device tensors -> dict(gh1, gw2, gb2, gw3, gb3) (device).  out: the caller's four leaves
    (gw2, gb2, gw3, gb3).  Every output starts as NaN: an element the kernels do not write shows."""
    import torch
    from irbfn_amd import _lib
    from irbfn_amd.model import _stream_ptr
    lib = _lib.load()
    B, O = h1.shape[0], W3.shape[1]
    new = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device="cuda")
    gh1 = new(B, H)
    gw2, gb2, gw3, gb3 = out if out is not None else (new(H, H), new(H), new(H, O), new(O))
    nb = int(lib.irbfn_mlp_head_vjp_workspace_bytes(H, H, O))
    assert nb > 0, nb
    if ws is None:
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    st = lib.irbfn_mlp_head_vjp(_ptr(h1), _ptr(W2), _ptr(b2), _ptr(W3), _ptr(g), _ptr(gh1), _ptr(gw2), _ptr(gb2), _ptr(gw3), _ptr(gb3),
                                B, H, H, O, _ptr(ws), nb, _stream_ptr(torch))
    assert st == 0, st
    return dict(gh1=gh1, gw2=gw2, gb2=gb2, gw3=gw3, gb3=gb3)
