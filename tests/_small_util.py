"""Helpers of tests/test_gpu_small_batch.py (K1s, `rbf_fwd_clane`) and tests/test_gpu_mfma_forward.py (K1m, `rbf_fwd_mfma`).

The planner's rules are restated here in Python (small_plan, mfma_plan) so that a test states the geometry it expects instead of
reading it back from the run; the launch goes through the raw `irbfn_net_forward` into a buffer with NaN rows behind row B
(forward_guarded), so that a row the kernel did not write -- or wrote behind the batch -- shows.

Bounds (the project's own, none new):
  fast bases     |got - ref| <= 1e-5 |ref| + 3e-6 scale element-wise, scale = sum_k |gamma phi_k W_ko| + |bias_o| (_terms_scale), and
                 |got - K1| <= 4e-6 scale + 1e-6 against the forced all-float32 kernel K1 on the same input
                 (tests/test_gpu_parity.py::test_small_batch_kernel_and_tiled_kernel_agree, ::test_forward_trained_checkpoints);
  generic bases  max|got - ref| / max|ref| <= 2e-5 (tests/test_gpu_parity.py::test_forward_all_bases): terms of both signs make the
                 scale meaningless."""
import numpy as np

from test_gpu_gram import _terms_scale
from irbfn_amd import _lib
from irbfn_amd.model import WCRBFNet, _ptr, _stream_ptr
from oracle import irbfn_oracle as orc

FAST = {"gaussian": 0, "gaussian_wide": 0, "gaussian_wider": 0, "inverse_quadratic": 1, "inverse_multiquadric": 2}
GUARD = 64                      # NaN rows behind row B

COMPILED_OP = (2, 4, 5, 8, 10, 16, 32, 64, 100, 128)


def bclass(basis):
    return FAST.get(basis, 3)


def padded_D(D):
    return 3 if D <= 3 else 4 if D == 4 else 7 if D <= 7 else 8


def padded_O(O):
    return next(op for op in COMPILED_OP if O <= op)


def _cdiv(a, b):
    return -(-a // b)


def small_plan(N, B, OP):
    """K1s (small_geometry): one query per tile, blocks of 256 lanes x cpl centres, the centre blocks bounded by 256, by 4096
    workgroups per launch and by the 4 Mi floats of partial sums -> (cpl, nb, grid)."""
    cpl, nb = 1, _cdiv(N, 256)
    while nb > 1 and (nb > 256 or nb * B > 4096 or nb * B * OP > (4 << 20)):
        cpl *= 2
        nb = _cdiv(N, 256 * cpl)
    return cpl, nb, nb * B


def small_name(D, O, basis):
    return f"rbf_fwd_clane<D={padded_D(D)},OP={padded_O(O)},BC={bclass(basis)},QT=1>"


def mfma_lds_bytes(D, O, QJ, nw):
    OW, cw, rows = 16 * _cdiv(O, 16), (D + 1 + 3) & ~3, 16 * QJ
    return 4 * max(nw * 16 * (cw + OW), rows * D, nw * rows * (OW + 1) + rows)


def mfma_plan(D, N, B, O):
    """K1m (plan_mfma): tiles of 16 QJ rows, enough waves per block for 8192 (narrow) / 2048 (wide) waves in the launch, at
    least two 16-centre chunks per wave, the reduction tile inside 160 KB of LDS -> (NT, QJ, nw, grid)."""
    wide = O > 16
    QJ = 2 if wide else 4
    tiles = _cdiv(B, 16 * QJ)
    nw = min(16, max(1, _cdiv(2048 if wide else 8192, tiles)))
    nw = 1 << (nw.bit_length() - 1)
    chunks = _cdiv(N, 16)
    while nw > 1 and chunks // nw < 2:
        nw //= 2
    while nw > 1 and mfma_lds_bytes(D, O, QJ, nw) > 160 * 1024:
        nw //= 2
    return _cdiv(O, 16), QJ, nw, tiles


def mfma_name(D, O, basis):
    return f"rbf_fwd_mfma<D={D},NT={_cdiv(O, 16)},QJ={2 if O > 16 else 4},BC={bclass(basis)}>"


# ------------------------------------------------------------------------------------------------ launches
def forward_into(net, params, x, buf, kernel=_lib.FWD_AUTO):
    """The raw irbfn_net_forward of x[B, D] into the device buffer `buf` (at least B rows) with `kernel` forced."""
    import torch
    lib = _lib.load()
    net.set_options(fwd_kernel=kernel)
    try:
        net.bind(params)
        xt = torch.tensor(np.ascontiguousarray(x, dtype=np.float32)).cuda()
        st = lib.irbfn_net_forward(net._handle(torch), _ptr(xt), _ptr(buf), x.shape[0], _stream_ptr(torch))
        _lib.check(st, "irbfn_net_forward")
        torch.cuda.current_stream().synchronize()
    finally:
        net.set_options(fwd_kernel=_lib.FWD_AUTO)


def nan_buffer(rows, O):
    import torch
    return torch.full((rows, O), float("nan"), dtype=torch.float32, device="cuda")


def forward_guarded(net, params, x, kernel=_lib.FWD_AUTO):
    """-> (out[B, O], what the launch reports).  The GUARD rows behind row B are asserted to be NaN still."""
    B = x.shape[0]
    buf = nan_buffer(B + GUARD, net.out_features)
    forward_into(net, params, x, buf, kernel)
    launch = net.last_launch()
    out = buf.cpu().numpy()
    assert np.isnan(out[B:]).all(), f"{launch['kernel']} wrote behind row {B}"
    return out[:B], launch


# ------------------------------------------------------------------------------------------------ references
def oracle(cfg, params, x):
    """(ref, scale) in float64.  A card without gated coordinates is outside orc.region_activation: every region with a row in
    dimension_ranges has the activation 1 (model.py:70), as tests/test_gpu_gram_setup.py states it for one region."""
    p64, x64 = orc.cast_params(params, np.float64), np.asarray(x, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if len(cfg["activation_idx"]) == 0:
            pp = p64["params"]
            nr = min(len(cfg["dimension_ranges"]), cfg["num_regions"])
            phi = orc.rbf_layer(x64, pp["rbf_list"]["centers"], pp["rbf_list"]["log_sigs"], cfg["basis_func"])[:, :nr, :].sum(axis=1)
            W, b = pp["linear"]["kernel"], pp["linear"]["bias"]
            return phi @ W + b, np.abs(phi) @ np.abs(W) + np.abs(b)
        return orc.wcrbfnet_apply(cfg, p64, x64), _terms_scale(cfg, p64, x64)


def fast_err(got, ref, scale):
    """max over the elements of |got - ref| / (1e-5 |ref| + 3e-6 scale): inside the bound up to 1."""
    return float((np.abs(got - ref) / (1e-5 * np.abs(ref) + 3e-6 * scale)).max())


def k1_err(got, k1, scale):
    """max of |got - K1| / (4e-6 scale + 1e-6): inside the bound up to 1."""
    return float((np.abs(got.astype(np.float64) - k1) / (4e-6 * scale + 1e-6)).max())


def generic_err(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def check(tag, cfg, params, x, got, net=None, ref=None, scale=None):
    """Prints and asserts the bounds of the module docstring for got = the kernel's output on x; with `net`, the forced K1 runs
    on the same input (fast bases)."""
    if ref is None:
        ref, scale = oracle(cfg, params, x)
    assert got.shape == ref.shape and got.dtype == np.float32
    if cfg["basis_func"] not in FAST:
        e = generic_err(got, ref)
        print(f"{tag}: max|err|/max|ref| {e:.2e} (bound 2e-5)")
        assert e <= 2e-5, tag
        return
    e = fast_err(got, ref, scale)
    line = f"{tag}: err/bound {e:.3f}, max err/scale {float((np.abs(got - ref) / scale).max()):.2e}"
    ek = None
    if net is not None:
        k1, launch = forward_guarded(net, params, x, _lib.FWD_K1)
        assert launch["kernel"].startswith("rbf_fwd_qlane<"), launch
        ek = k1_err(got, k1, scale)
        line += f", against K1 {ek:.3f} of its bound"
    print(line)
    assert e <= 1.0, tag
    assert ek is None or ek <= 1.0, tag


# ------------------------------------------------------------------------------------------------ nets with several regions
def region_net(D, K, O, basis, lows, highs, ranges, delta, rows=None, seed=0):
    """R = len(ranges) regions gated on the first len(lows) coordinates; region r takes range ranges[r][d] of coordinate d and its
    centres lie in that box (+- 0.2; the other coordinates in [-1.2, 1.2]).  rows: how many rows of `ranges` the card keeps
    (regions without a row stay 0, model.py:88-93)."""
    R, ns = len(ranges), len(lows)
    rng = np.random.default_rng(7919 * D + 31 * K + R + seed)
    c = rng.uniform(-1.2, 1.2, size=(R, K, D))
    for r in range(R):
        for d in range(ns):
            c[r, :, d] = rng.uniform(lows[d][ranges[r][d]] - 0.2, highs[d][ranges[r][d]] + 0.2, size=K)
    cfg = {"in_features": D, "out_features": O, "num_kernels": K, "basis_func": basis, "num_regions": R,
           "lower_bounds": [list(map(float, v)) for v in lows], "upper_bounds": [list(map(float, v)) for v in highs],
           "dimension_ranges": [list(map(int, v)) for v in ranges[:R if rows is None else rows]],
           "activation_idx": list(range(ns)), "delta": [float(v) for v in delta]}
    params = {"params": {"rbf_list": {"centers": c.astype(np.float32), "log_sigs": rng.uniform(-0.5, 0.3, size=(R, K)).astype(np.float32)},
                         "linear": {"kernel": (rng.normal(size=(K, O)) * 0.2).astype(np.float32),
                                    "bias": (0.05 + np.abs(rng.normal(size=(O,))) * 0.1).astype(np.float32)}}}
    return cfg, params


def region_queries(B, D, lows, highs, ranges, delta, seed):
    """Row b lies in the box of region b % R; two rows of three are then moved to a border of that box in one gated coordinate:
    exactly onto it (b % 3 == 1) or within 0.3 / delta of it (b % 3 == 2), where the neighbouring range's factor is 0.35 .. 0.65."""
    rng = np.random.default_rng(seed)
    R, ns = len(ranges), len(lows)
    x = rng.uniform(-1.0, 1.0, size=(B, D))
    for b in range(B):
        r = ranges[b % R]
        for d in range(ns):
            x[b, d] = rng.uniform(lows[d][r[d]], highs[d][r[d]])
        if ns and b % 3:
            d = int(rng.integers(ns))
            edge = (lows, highs)[int(rng.integers(2))][d][r[d]]
            x[b, d] = edge + (0.0 if b % 3 == 1 else rng.uniform(-0.3, 0.3) / delta[d])
    return x.astype(np.float32)


def nonfinite_rows(x, gated, ungated, rows):
    """Writes NaN / +-Inf into the given rows of x (in place): rows = seven row numbers for a NaN in an ungated coordinate, a NaN in
    a gated one, a row that is all NaN, +Inf and -Inf in gated coordinates, +Inf and -Inf in ungated ones.
    -> (rows with a NaN, rows with an Inf)."""
    n_u, n_g, n_all, pg, mg, pu, mu = rows
    x[n_u, ungated[0]] = np.nan
    x[n_g, gated[-1]] = np.nan
    x[n_all, :] = np.nan
    x[pg, gated[0]] = np.inf
    x[mg, gated[-1]] = -np.inf
    x[pu, ungated[-1]] = np.inf
    x[mu, ungated[0]] = -np.inf
    return [n_u, n_g, n_all], [pg, mg, pu, mu]


def check_nonfinite(tag, cfg, params, x, got, nan_rows, inf_rows):
    """NaN exactly where the oracle gives NaN, the Inf rows within rtol 1e-5 / atol 1e-6 of the oracle (as
    tests/test_gpu_parity.py::test_forward_nan_and_inf_propagate), every other row inside the bound."""
    ref, scale = oracle(cfg, params, x)
    assert np.isnan(ref[nan_rows]).all() and np.isfinite(np.delete(ref, nan_rows, axis=0)).all()      # the inputs do what the case says
    assert np.array_equal(np.isnan(got), np.isnan(ref)), tag
    assert np.isfinite(got[inf_rows]).all() and np.allclose(got[inf_rows], ref[inf_rows], rtol=1e-5, atol=1e-6), tag
    rest = np.setdiff1d(np.arange(x.shape[0]), nan_rows + inf_rows)
    e = fast_err(got[rest], ref[rest], scale[rest])
    print(f"{tag}: err/bound {e:.3f} on the {len(rest)} finite rows; NaN rows {nan_rows}, Inf rows {inf_rows} as the oracle")
    assert e <= 1.0, tag
