"""The closed-form output-layer fit on the GPU (run on the MI355X box with ``-m gpu``): irbfn_syrk_f64 through the C ABI on guarded
buffers, irbfn_net_hidden against the float64 oracle, then ``fit_linear`` end to end (cases and bounds: tests/_linear_fit_util.py).

Gram matrix: integer rows bit for bit against NumPy int64; float rows within rows 2^-53 sum_n |z_ni z_nj| per entry.  z carries NaN
guard rows past `rows` and NaN guard columns in [M, ldz); g is prefilled with NaN and carries guard elements past M * M; the
workspace is prefilled with 0x5A and carries a guarded tail.

Hidden layer: |h - h64| <= 1e-5 |h64| + 3e-6 sum_r gamma64 max(1, |phi64|) per entry.  Largest err / bound, printed by the tests:
checkpoint fixtures 0.061, 0.044, 0.062, 0.034 (in the order of CKPT_RUNS); synthetic nets per basis: gaussian 0.027,
gaussian_wide 0.030, gaussian_wider 0.028, inverse_quadratic 0.027, linear 0.035, quadratic 0.032, multiquadric 0.033,
inverse_multiquadric 0.028, spline 0.047, poisson_one 0.021, poisson_two 0.016, matern32 0.030, matern52 0.035 (the float32
restatement of the reference: 0.019 - 0.068, tests/test_linear_fit_cpu.py).  fit_linear on the end-to-end case:
sqrt(J_fit) = sqrt(J_ref) = 0.083947 against e = 4.55e-4."""
import ctypes as C

import numpy as np
import pytest
import torch

import _linear_fit_util as lu
from conftest import CKPT_RUNS, load_ckpt_fixture
from irbfn_amd import _lib, linear_fit
from irbfn_amd.model import WCRBFNet, _ptr, _stream_ptr
from oracle import irbfn_oracle as orc

pytestmark = pytest.mark.gpu
TILE = 64                        # rows / columns of g per block (kSyTile)
CHUNK = 32                       # rows of z staged at a time (kSyChunk)
SLAB_ROWS = 256                  # no slab but the last is shorter (kSySlabRows)
GUARD = 3
OK, BAD_ARG, NO_PARAMS = 0, -1, -4
MS = (1, 15, 16, 17, 63, 64, 65, 129)
ROWS = (1, 3, 4, 5, 63, 64, 65, 1000)


class Syrk:
    """irbfn_syrk_f64 calls on guarded, prefilled buffers; g as a NumPy array after every call."""

    def __init__(self, z, pad_cols=GUARD):
        self.lib = _lib.load()
        z = np.ascontiguousarray(z, np.float32)
        self.rows, self.M = z.shape
        self.ldz = self.M + pad_cols
        zg = np.full((self.rows + GUARD, self.ldz), np.nan, np.float32)
        zg[:self.rows, :self.M] = z
        self.zg = torch.from_numpy(zg).cuda()
        self.g = torch.full((self.M * self.M + GUARD,), float("nan"), dtype=torch.float64, device="cuda")

    def run(self, row0=0, rows=None, accumulate=0):
        rows = self.rows - row0 if rows is None else rows
        need = self.lib.irbfn_syrk_f64_workspace_bytes(rows, self.M)
        assert need >= 0 and need < 1 << 30
        ws = torch.full((need + 8 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda")      # the kernels must not rely on a cleared workspace
        zp = C.c_void_p(self.zg.data_ptr() + 4 * row0 * self.ldz)
        st = self.lib.irbfn_syrk_f64(zp, self.ldz, rows, self.M, _ptr(self.g), accumulate, _ptr(ws), need, _stream_ptr(torch))
        assert st == OK, st
        torch.cuda.synchronize()
        assert (ws[need:] == 0x5A).all() and torch.isnan(self.g[self.M * self.M:]).all()
        self.need = need
        return self.g[:self.M * self.M].cpu().numpy().reshape(self.M, self.M)


@pytest.mark.parametrize("M", MS)
def test_syrk_integer_rows_are_exact(gpu, M):
    z = lu.integer_rows(max(ROWS), M, seed=M)
    for rows in ROWS:
        g = Syrk(z[:rows]).run()
        assert g.tobytes() == lu.gram_int(z[:rows]).tobytes(), (M, rows)


def test_syrk_exact_over_several_slabs_and_tiles(gpu):
    lib = _lib.load()
    # one tile pair: ceil(1100 / SLAB_ROWS) = 5 slabs of ceil(220 / CHUNK) CHUNK = 224 rows, the last one of 204 (six chunks and 12 rows)
    rows, M = 1100, 17
    assert -(-rows // SLAB_ROWS) == 5 and -(-(rows // 5) // CHUNK) * CHUNK == 224
    assert lib.irbfn_syrk_f64_workspace_bytes(rows, M) == 5 * TILE * TILE * 8
    z = lu.integer_rows(rows, M, seed=11)
    assert Syrk(z).run().tobytes() == lu.gram_int(z).tobytes()
    # 16 tiles a side with a ragged last one (1011 = 15 * 64 + 51), 136 pairs, 16 slabs of 256 rows and a last one of 4
    z = lu.integer_rows(4100, 1011, seed=12)
    s = Syrk(z)
    g = s.run()
    assert s.need == 136 * 17 * TILE * TILE * 8
    assert g.tobytes() == lu.gram_int(z).tobytes()


@pytest.mark.parametrize("M,rows", ((17, 5), (65, 1000), (129, 333)))
def test_syrk_float_rows_meet_the_summation_bound(gpu, M, rows):
    z = lu.float_rows(rows, M, seed=M + rows)
    ref, bound = lu.gram_ref(z), lu.gram_bound(z)
    s = Syrk(z)
    g = s.run()
    assert np.isfinite(g).all()                                         # accumulate = 0 never reads the NaN prefill
    assert (np.abs(g - ref) <= bound).all()
    assert g.tobytes() == g.T.copy().tobytes()                          # symmetric bit for bit
    assert s.run().tobytes() == g.tobytes()                             # a repeat is bit-identical
    # two halves added onto a g zeroed by accumulate = 0, rows = 0
    half = rows // 2
    zero = s.run(rows=0)
    assert (zero == 0).all()
    s.run(row0=0, rows=half, accumulate=1)
    g2 = s.run(row0=half, accumulate=1)
    assert (np.abs(g2 - ref) <= bound).all() and g2.tobytes() == g2.T.copy().tobytes()
    assert s.run(rows=0, accumulate=1).tobytes() == g2.tobytes()        # nothing to add: untouched


def test_syrk_nan_stays_in_its_row_and_column(gpu):
    z = lu.float_rows(300, 70, seed=1).copy()
    z[123, 66] = np.nan
    g = Syrk(z).run()
    bad = np.zeros((70, 70), bool)
    bad[66, :] = bad[:, 66] = True
    assert np.isnan(g[bad]).all() and np.isfinite(g[~bad]).all()
    z[123, 66] = 0.0
    assert (np.abs(g[~bad] - lu.gram_ref(z)[~bad]) <= lu.gram_bound(z)[~bad]).all()


def test_syrk_refusals_launch_nothing(gpu):
    lib = _lib.load()
    z = torch.zeros((8, 20), dtype=torch.float32, device="cuda")
    g = torch.full((400,), float("nan"), dtype=torch.float64, device="cuda")
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    need = lib.irbfn_syrk_f64_workspace_bytes(8, 17)

    def call(M=17, ldz=20, nbytes=ws.numel()):
        return lib.irbfn_syrk_f64(_ptr(z), ldz, 8, M, _ptr(g), 0, _ptr(ws), nbytes, _stream_ptr(torch))
    assert call(M=0) == BAD_ARG and call(M=8193, ldz=8200) == BAD_ARG and call(ldz=16) == BAD_ARG and call(nbytes=need - 1) == BAD_ARG
    torch.cuda.synchronize()
    assert torch.isnan(g).all()
    assert call() == OK
    torch.cuda.synchronize()
    assert (g[:289] == 0).all() and torch.isnan(g[289:]).all()


def test_syrk_wrapper(gpu):
    z = lu.integer_rows(300, 21, seed=2)
    zt = torch.from_numpy(z).cuda()
    g = linear_fit.syrk(zt)
    assert g.dtype == torch.float64 and g.cpu().numpy().tobytes() == lu.gram_int(z).tobytes()
    wide = torch.full((300, 30), float("nan"), dtype=torch.float32, device="cuda")
    wide[:, :21] = zt
    out = torch.zeros((21, 21), dtype=torch.float64, device="cuda")
    linear_fit.syrk(wide[:, :21], out=out, accumulate=True)              # a strided view is read in place
    linear_fit.syrk(zt, out=out, accumulate=True)
    assert out.cpu().numpy().tobytes() == (2 * lu.gram_int(z)).tobytes()
    with pytest.raises(ValueError):
        linear_fit.syrk(zt, out=torch.zeros((20, 21), dtype=torch.float64, device="cuda"))


# ------------------------------------------------------------------ hidden layer
def _hidden_guarded(net, x32, ldh):
    """irbfn_net_hidden of the bound net into a NaN-prefilled [B + GUARD, ldh] buffer: the [B, K] block, guards checked."""
    lib = _lib.load()
    B, K = x32.shape[0], net.num_kernels
    xd = torch.from_numpy(np.vstack([x32, np.full((GUARD, x32.shape[1]), np.nan, np.float32)])).cuda()
    h = torch.full((B + GUARD, ldh), float("nan"), dtype=torch.float32, device="cuda")
    st = lib.irbfn_net_hidden(net._handle(torch), _ptr(xd), _ptr(h), ldh, B, _stream_ptr(torch))
    assert st == OK, st
    torch.cuda.synchronize()
    assert torch.isnan(h[B:]).all() and torch.isnan(h[:, K:]).all()
    return h[:B, :K].cpu().numpy()


@pytest.mark.parametrize("run", CKPT_RUNS)
def test_hidden_of_the_trained_checkpoints(gpu, run):
    cfg, params, x, out64, _, _ = load_ckpt_fixture(run)
    x32 = x.astype(np.float32)
    h64, bound = lu.hidden_ref(cfg, params, x32)
    net = WCRBFNet.from_config(cfg)
    net.bind(params)
    K = net.num_kernels
    worst = 0.0
    for B in (1, 63, 64, 65, 257):
        idx = np.arange(B) % x32.shape[0]
        for ldh in (K, K + 3):
            h = _hidden_guarded(net, x32[idx], ldh)
            worst = max(worst, lu.ratio(h, h64[idx], bound[idx]))
    assert "rbf_hidden<" in net.last_launch()["kernel"]
    print(f"{run}: hidden err/bound {worst:.3f}")
    assert worst <= 1.0
    # consistency: hidden @ W + bias against apply, within twice the forward tolerance of tests/test_gpu_parity.py
    W = np.asarray(params["params"]["linear"]["kernel"], np.float64)
    b = np.asarray(params["params"]["linear"]["bias"], np.float64)
    hid = net.hidden(params, x32)
    assert hid.dtype == np.float32 and hid.shape == h64.shape
    out = net.apply(params, x32).astype(np.float64)
    tol = 1e-5 * np.abs(out64) + 3e-6 * (np.abs(h64) @ np.abs(W))
    assert (np.abs(hid.astype(np.float64) @ W + b - out) <= 2 * tol).all()
    assert net.hidden(params, torch.from_numpy(x32)).device.type == "cpu" and net.hidden(params, torch.from_numpy(x32).cuda()).is_cuda


@pytest.mark.parametrize("basis", lu.BASES)
def test_hidden_of_every_basis(gpu, basis):
    worst = 0.0
    for D in lu.SYN_DIMS:
        for K in lu.SYN_KS:
            cfg, params, x, h64, bound = lu.synthetic_case(D, K, basis)
            net = WCRBFNet.from_config(cfg)
            net.bind(params)
            worst = max(worst, lu.ratio(_hidden_guarded(net, x, K + 1), h64, bound))
    print(f"{basis}: hidden err/bound {worst:.3f}")
    assert worst <= 1.0


def test_hidden_rows_are_independent_and_repeats_identical(gpu):
    cfg, params, x, _, _, _ = load_ckpt_fixture(CKPT_RUNS[1])            # 128 regions
    x32 = np.tile(x.astype(np.float32), (3, 1))[:130]
    net = WCRBFNet.from_config(cfg)
    a = net.hidden(params, x32)
    assert a.tobytes() == net.hidden(params, x32).tobytes()
    xn = x32.copy()
    xn[70, 1] = np.nan
    b = net.hidden(params, xn)
    assert np.isnan(b[70]).all()
    keep = np.arange(130) != 70
    assert b[keep].tobytes() == a[keep].tobytes()


def test_hidden_status(gpu):
    lib = _lib.load()
    cfg, params, x, h64, _ = lu.synthetic_case(3, 17, "gaussian")
    net = WCRBFNet.from_config(cfg)
    xd = torch.from_numpy(x).cuda()
    h = torch.full((x.shape[0], 17), float("nan"), dtype=torch.float32, device="cuda")
    call = lambda xp, hp, ldh, B: lib.irbfn_net_hidden(net._handle(torch), xp, hp, ldh, B, _stream_ptr(torch))
    assert call(_ptr(xd), _ptr(h), 17, x.shape[0]) == NO_PARAMS
    net.bind(params)
    assert call(_ptr(xd), _ptr(h), 16, x.shape[0]) == BAD_ARG and call(None, _ptr(h), 17, 4) == BAD_ARG
    assert call(_ptr(xd), None, 17, 4) == BAD_ARG and call(_ptr(xd), _ptr(h), 17, -1) == BAD_ARG
    assert call(None, None, 0, 0) == OK
    torch.cuda.synchronize()
    assert torch.isnan(h).all()


# ------------------------------------------------------------------ fit_linear
def _fit_net(frozen=False):
    cfg, centers, log_sigs, x, y, h64, gsum = lu.fit_case()
    if frozen:
        net = WCRBFNet.from_config(dict(cfg, fixed_centers=True, fixed_width=True, log_sigs=log_sigs[None].tolist()), centers=centers)
        return net, net.init()
    net = WCRBFNet.from_config(cfg)
    p = net.init()
    p["params"]["rbf_list"]["centers"] = centers[None].copy()
    p["params"]["rbf_list"]["log_sigs"] = log_sigs[None].copy()
    return net, p


@pytest.mark.parametrize("fit_bias", (True, False))
@pytest.mark.parametrize("ridge", (0.0, 1e-2))
def test_fit_linear_is_the_solve_of_the_kernels_own_gram(gpu, ridge, fit_bias):
    cfg, centers, log_sigs, x, y, h64, gsum = lu.fit_case()
    net, p = _fit_net()
    new, fit = linear_fit.fit_linear(net, p, x, y, ridge=ridge, fit_bias=fit_bias, batch_size=512)      # 512 + 512 + 476
    assert fit.n == 1500
    h = net.hidden(p, x).astype(np.float64)
    G = lu.stacked_gram(h, y.astype(np.float64))
    ref = linear_fit.NormalEquations(net, G=torch.from_numpy(G)).solve(ridge=ridge, fit_bias=fit_bias)
    W, b = fit.kernel.cpu().numpy(), fit.bias.cpu().numpy()
    Wr, br = ref.kernel.numpy(), ref.bias.numpy()
    assert np.abs(W - Wr).max() <= 1e-9 * np.abs(Wr).max()
    assert np.abs(b - br).max() <= 1e-9 * np.abs(br).max() if fit_bias else (b == 0).all()
    lin = new["params"]["linear"]
    assert lin["kernel"].dtype == np.float32 and lin["bias"].dtype == np.float32
    assert np.array_equal(lin["kernel"], W.astype(np.float32)) and np.array_equal(lin["bias"], b.astype(np.float32))
    assert new["params"]["rbf_list"]["centers"] is p["params"]["rbf_list"]["centers"]


def test_fit_linear_is_optimal_up_to_the_hidden_layers_tolerance(gpu):
    cfg, centers, log_sigs, x, y, h64, gsum = lu.fit_case()
    assert np.linalg.cond(np.hstack([h64, np.ones((1500, 1))])) < 100
    net, p = _fit_net()
    ridge = 1e-8
    _, fit = linear_fit.fit_linear(net, p, x, y, ridge=ridge, batch_size=512)
    y64 = y.astype(np.float64)
    lam = ridge * np.trace(h64.T @ h64) / 48
    Wr, br, _ = lu.lstsq_ref(h64, y64, lam, True)
    J = lambda W, b: (((h64 @ W + b - y64) ** 2).sum() + lam * (W ** 2).sum()) / 1500
    tol = lambda W: np.sqrt(((1e-5 * np.abs(h64) @ np.abs(W) + 3e-6 * gsum[:, None] * np.abs(W).sum(0)[None]) ** 2).sum(1).mean())
    Wf, bf = fit.kernel.cpu().numpy(), fit.bias.cpu().numpy()
    e = tol(Wf) + tol(Wr)
    print(f"sqrt(J_fit) {np.sqrt(J(Wf, bf)):.6f}  sqrt(J_ref) {np.sqrt(J(Wr, br)):.6f}  e {e:.2e}  ridge_abs {fit.ridge_abs:.3e}")
    assert abs(fit.ridge_abs - lam) <= 1e-4 * lam
    assert np.sqrt(J(Wf, bf)) <= np.sqrt(J(Wr, br)) + e


def test_fit_linear_of_a_fixed_width_net(gpu):
    cfg, centers, log_sigs, x, y, h64, gsum = lu.fit_case()
    net, p = _fit_net(frozen=True)
    assert set(p["params"]) == {"linear"}
    new, fit = linear_fit.fit_linear(net, p, torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())
    assert set(new["params"]) == {"linear"} and set(new["params"]["linear"]) == {"kernel", "bias"}
    out = net.apply(new, x).astype(np.float64)
    mse = ((out - y.astype(np.float64)) ** 2).mean()
    W = np.abs(fit.kernel.cpu().numpy())
    tol = 1e-5 * np.abs(out) + 3e-6 * (np.abs(h64) @ W)                  # the forward tolerance, per entry of the residual
    # apply against the float64 net, the float64 net against the kernel's own hidden layer times W: twice the tolerance per entry
    # (the float32 cast of W, 6e-8 |h| |W|, is inside the 0.1); rss from G: 1e-9 y^T y as on the CPU
    res, d = np.abs(out - y), 2.1 * tol
    assert abs(mse - fit.mse) <= (2 * res * d + d ** 2).mean() + 1e-9 * (y.astype(np.float64) ** 2).mean()
    assert fit.mse < 0.05 ** 2 * 1.2                                     # the noise floor of the labels


def test_fit_linear_refusals(gpu):
    cfg, centers, log_sigs, x, y, h64, gsum = lu.fit_case()
    net, p = _fit_net()
    with pytest.raises(ValueError, match="rows"):
        linear_fit.fit_linear(net, p, x[:100], y[:99])
    with pytest.raises(ValueError):
        linear_fit.fit_linear(net, p, x[:, :2], y)
    with pytest.raises(ValueError):
        linear_fit.fit_linear(net, p, x, y[:, :2])
    with pytest.raises(ValueError, match="float64"):
        linear_fit.fit_linear(WCRBFNet.from_config(cfg, use_float64=True), p, x, y)
