"""The Dense head of DeeperWCRBFNet (irbfn_amd/csrc/mlp_head.hip) through its C ABI, h1 given as data, against the float64
NumPy reference of tests/_head_util.py (its own checks: tests/test_head_reference_cpu.py).

A  integer-lattice inputs: every correct float32 evaluation equals the float64 result exactly, so ``array_equal`` -- over the
   grid-stride of the backward (a second tile per wave from B = 32 769), the forward's (from 65 537), every O padded to 16,
   the one-lane-per-row forward for O > 16 with its direct-store branch (O > 64), and relu'(0) = 0.
B  real-valued inputs: error relative to each element's cancellation scale, within the any-order float32 worst case AND
   within 4 x what a plain float32 NumPy evaluation makes of the same inputs (DESIGN 2's margin).
C  properties: determinism, row independence, exact homogeneity in g, the flat-buffer layout of DeeperTrainState, refusals.
D  non-finite rows: NaN / +Inf / -Inf follow the reference; a NaN query gives a NaN row end to end.
E  one Deeper training step at the reference's batch (B = 80 000) against float64 torch.autograd."""
import ctypes as C
from itertools import cycle

import numpy as np
import pytest
import torch

import _head_util as hu
from conftest import load_deeper_fixture
from irbfn_amd import _lib, configs, planner, train
from irbfn_amd.model import DeeperWCRBFNet, _stream_ptr
from oracle import irbfn_oracle as orc

pytestmark = pytest.mark.gpu

H = hu.H
GRADS = ("gh1",) + hu.LEAF_NAMES
NARROW_O = (1, 2, 3, 10, 15, 16)
BWD_B = (1, 31, 32, 33, 129, 4099, 32767, 32768, 32769, 32897, 65537, 80000, 200000)
FWD_B = (1, 31, 32, 33, 127, 128, 129, 4099, 65535, 65536, 65537, 65665, 80000, 200000)
WIDE_O = (17, 20, 63, 64, 65, 100, 128)
WIDE_B = (1, 63, 64, 65, 3001)


def _cycled(Bs, Os):
    return [(B, O) for B, O in zip(Bs, cycle(Os))]


def _fwd(c):
    return hu.gpu_forward(*(hu.dev(c[k]) for k in ("h1", "W2", "b2", "W3", "b3"))).cpu().numpy()


def _bwd(c, **kw):
    r = hu.gpu_vjp(*(hu.dev(c[k]) for k in ("h1", "W2", "b2", "W3", "g")), **kw)
    return {k: v.cpu().numpy() for k, v in r.items()}


def _ref_bwd(c):
    return hu.backward64(c["h1"], c["W2"], c["b2"], c["W3"], c["g"])


def _ref_fwd(c):
    return hu.forward64(c["h1"], c["W2"], c["b2"], c["W3"], c["b3"])


# ------------------------------------------------------------------ A: integer lattice, exact
@pytest.mark.parametrize("B,O", _cycled(BWD_B, NARROW_O))
def test_lattice_backward_is_exact(gpu, B, O):
    c = hu.lattice_case(B, O, seed=7 * B + O)
    assert hu.lattice_is_exact(c)
    ref, got = _ref_bwd(c), _bwd(c)
    for k in GRADS:
        assert got[k].shape == ref[k].shape
        assert np.array_equal(got[k].astype(np.float64), ref[k]), (k, B, O, int((got[k] != ref[k]).sum()))


@pytest.mark.parametrize("B,O", _cycled(FWD_B, NARROW_O))
def test_lattice_forward_is_exact(gpu, B, O):
    c = hu.lattice_case(B, O, seed=11 * B + O)
    assert hu.lattice_is_exact(c)
    ref, got = _ref_fwd(c)["out"], _fwd(c)
    assert np.array_equal(got.astype(np.float64), ref), (B, O, int((got != ref).sum()))


@pytest.mark.parametrize("B", WIDE_B)
@pytest.mark.parametrize("O", WIDE_O)
def test_lattice_wide_forward_is_exact(gpu, O, B):
    c = hu.lattice_case(B, O, seed=13 * B + O)
    assert hu.lattice_is_exact(c)
    ref, got = _ref_fwd(c)["out"], _fwd(c)
    assert np.array_equal(got.astype(np.float64), ref), (B, O, int((got != ref).sum()))


# ------------------------------------------------------------------ B: real values, accuracy
def _check_forward(c, what):
    f64, f32 = _ref_fwd(c), hu.forward32(c["h1"], c["W2"], c["b2"], c["W3"], c["b3"])
    got = _fwd(c)
    assert np.isfinite(got).all()
    r, r32, worst = hu.worst_ratio(got, f64["out"], f64["Sout"]), hu.worst_ratio(f32["out"], f64["out"], f64["Sout"]), hu.any_order_bound(65)
    print(f"[head] {what} out: max |err| / Sout = {r:.2e}  (float32 NumPy {r32:.2e}, any-order worst case {worst:.2e})")
    assert r <= worst and r <= 4 * r32, (what, r, r32, worst)


def _check_backward(c, what):
    B = c["h1"].shape[0]
    ref, r32, got = _ref_bwd(c), hu.backward32(c["h1"], c["W2"], c["b2"], c["W3"], c["g"]), _bwd(c)
    assert ((r32["z2"] > 0) == (ref["z2"] > 0)).all()                 # clear of the kink: float32 and float64 masks agree
    fails = []
    for k in GRADS:
        assert np.isfinite(got[k]).all(), k
        worst = hu.any_order_bound(65 if k == "gh1" else B + 80)
        r, rn = hu.worst_ratio(got[k], ref[k], ref["S" + k]), hu.worst_ratio(r32[k], ref[k], ref["S" + k])
        print(f"[head] {what} {k}: max |err| / S{k} = {r:.2e}  (float32 NumPy {rn:.2e}, any-order worst case {worst:.2e})")
        if not (r <= worst and r <= 4 * rn):
            fails.append((k, r, rn, worst))
    assert not fails, (what, fails)


@pytest.mark.parametrize("B", [33, 4099, 32769, 80000])
@pytest.mark.parametrize("O", [2, 10, 16])
def test_real_valued_head_accuracy(gpu, O, B):
    c, share = hu.real_case(B, O, seed=1000 * O + B)
    print(f"[head] real B={B} O={O}: {100 * share:.2f} % of the rows redrawn")
    assert share <= hu.REDRAW_CAP
    _check_forward(c, f"real B={B} O={O}")
    _check_backward(c, f"real B={B} O={O}")


@pytest.mark.parametrize("B", [4099, 80000])
def test_w3_columns_spread_over_six_decades(gpu, B):
    c, share = hu.real_case(B, 10, seed=77 + B, w3_col_spread=True)
    assert share <= hu.REDRAW_CAP
    _check_forward(c, f"W3 columns 1e-3..1e3 B={B}")
    _check_backward(c, f"W3 columns 1e-3..1e3 B={B}")


def _golden_f32():
    cfg, P, _, _ = load_deeper_fixture()
    return cfg, {"params": {g: {n: np.asarray(v, np.float32) for n, v in d.items()} for g, d in P["params"].items()}}


def _golden_queries(cfg, B, seed):
    rng = np.random.default_rng(seed)
    ns = len(cfg["activation_idx"])
    lo = np.array([min(cfg["lower_bounds"][d]) for d in range(ns)]); hi = np.array([max(cfg["upper_bounds"][d]) for d in range(ns)])
    return rng.uniform(lo, hi, size=(B, cfg["in_features"])).astype(np.float32)


@pytest.mark.parametrize("B", [4099, 80000])
def test_golden_head_accuracy(gpu, B):
    """The reference checkpoint's head (O = 10) on h1 from its own stage."""
    cfg, P = _golden_f32()
    p = P["params"]
    net = DeeperWCRBFNet.from_config(cfg)
    x = _golden_queries(cfg, B + B // 20 + 64, seed=B)
    h1 = net.stage.apply({"rbf_list": p["rbf_list"], "linear": p["linear_pre1"]}, x)
    rows, share = hu.keep_clear_rows(h1, p["linear_pre2"]["kernel"], p["linear_pre2"]["bias"], B)
    print(f"[head] golden B={B}: {100 * share:.2f} % of the rows passed over (near the kink)")
    assert share <= hu.REDRAW_CAP
    rng = np.random.default_rng(B + 1)
    c = dict(h1=np.ascontiguousarray(h1[rows]), W2=p["linear_pre2"]["kernel"], b2=p["linear_pre2"]["bias"], W3=p["linear"]["kernel"],
             b3=p["linear"]["bias"], g=rng.normal(size=(B, 10)).astype(np.float32))
    _check_forward(c, f"golden B={B}")
    _check_backward(c, f"golden B={B}")


@pytest.mark.parametrize("B", [33, 4099, 32769, 80000])
@pytest.mark.parametrize("O", [20, 100])
def test_real_valued_wide_forward_accuracy(gpu, O, B):
    c, share = hu.real_case(B, O, seed=1000 * O + B)
    assert share <= hu.REDRAW_CAP
    _check_forward(c, f"wide B={B} O={O}")


# ------------------------------------------------------------------ C: properties
def test_two_calls_agree(gpu):
    c, _ = hu.real_case(80000, 10, seed=5)
    a, b = _bwd(c), _bwd(c)
    for k in GRADS:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(_fwd(c), _fwd(c))
    w, _ = hu.real_case(3001, 100, seed=6)
    assert np.array_equal(_fwd(w), _fwd(w))


def _permuted(c, perm):
    return dict(c, h1=np.ascontiguousarray(c["h1"][perm]), g=np.ascontiguousarray(c["g"][perm]))


def test_a_permuted_batch_gives_permuted_rows(gpu):
    c, _ = hu.real_case(70001, 10, seed=8)
    perm = np.random.default_rng(9).permutation(70001)
    assert np.array_equal(_fwd(_permuted(c, perm)), _fwd(c)[perm])
    w, _ = hu.real_case(3001, 20, seed=10)
    permw = np.random.default_rng(11).permutation(3001)
    assert np.array_equal(_fwd(_permuted(w, permw)), _fwd(w)[permw])
    c, _ = hu.real_case(40001, 16, seed=12)
    perm = np.random.default_rng(13).permutation(40001)
    assert np.array_equal(_bwd(_permuted(c, perm))["gh1"], _bwd(c)["gh1"][perm])


@pytest.mark.parametrize("k", [-20, -1, 3, 40])
def test_scaling_g_by_a_power_of_two_scales_every_gradient_exactly(gpu, k):
    c, _ = hu.real_case(40001, 10, seed=14)
    one, scaled = _bwd(c), _bwd(dict(c, g=c["g"] * np.float32(2.0 ** k)))
    for n in GRADS:
        assert np.array_equal(scaled[n], one[n] * np.float32(2.0 ** k)), n


def test_an_empty_batch_gives_zero_weight_gradients(gpu):
    lib = _lib.load()
    c, _ = hu.real_case(4, 10, seed=15)
    w2, b2, w3, b3 = (hu.dev(c[k]) for k in ("W2", "b2", "W3", "b3"))
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")
    gw2, gb2, gw3, gb3 = nan(H, H), nan(H), nan(H, 10), nan(10)
    nb = int(lib.irbfn_mlp_head_vjp_workspace_bytes(H, H, 10))
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    p, null = hu._ptr, C.c_void_p(None)
    st = lib.irbfn_mlp_head_vjp(null, p(w2), p(b2), p(w3), null, null, p(gw2), p(gb2), p(gw3), p(gb3), 0, H, H, 10, p(ws), nb,
                                _stream_ptr(torch))
    assert st == 0
    for t in (gw2, gb2, gw3, gb3):
        assert bool((t == 0).all())
    # an empty batch reads no h1: a misaligned address is no error there
    assert lib.irbfn_mlp_head_vjp(C.c_void_p(ws.data_ptr() + 4), p(w2), p(b2), p(w3), null, null, p(gw2), p(gb2), p(gw3), p(gb3), 0, H, H,
                                  10, p(ws), nb, _stream_ptr(torch)) == 0
    assert lib.irbfn_mlp_head_forward(null, p(w2), p(b2), p(w3), p(b3), null, 0, H, H, 10, _stream_ptr(torch)) == 0


@pytest.mark.parametrize("O", [3, 10, 16])
def test_gradients_into_views_of_a_flat_buffer_at_odd_offsets(gpu, O):
    """The layout of DeeperTrainState: the four head gradients are views of one flat float buffer, at float offsets that
    are not multiples of 4.  Equal to the contiguous result, and not a float outside the views is written."""
    c, _ = hu.real_case(4099, O, seed=16 + O)
    plain = _bwd(c)
    sizes = (H * H, H, H * O, O)
    flat = torch.full((sum(sizes) + 32,), float("nan"), device="cuda")
    views, off = [], 1
    for n, shape in zip(sizes, ((H, H), (H,), (H, O), (O,))):
        views.append(flat[off:off + n].view(shape))
        off += n + 3                                                  # a gap of NaN guards ...
        off += 1 - off % 2                                            # ... and the next offset is odd again
    assert all((v.data_ptr() - flat.data_ptr()) // 4 % 2 == 1 for v in views)
    got = _bwd(c, out=tuple(views))
    written = torch.zeros_like(flat, dtype=torch.bool)
    for k, v in zip(hu.LEAF_NAMES, views):
        assert np.array_equal(got[k], plain[k]), k
        start = (v.data_ptr() - flat.data_ptr()) // 4
        written[start:start + v.numel()] = True
    assert bool(torch.isnan(flat[~written]).all()) and not bool(torch.isnan(flat[written]).any())
    assert np.array_equal(got["gh1"], plain["gh1"])


def test_refusals(gpu):
    lib = _lib.load()
    c, _ = hu.real_case(64, 10, seed=20)
    d = {k: hu.dev(v) for k, v in c.items()}
    p, s = hu._ptr, _stream_ptr(torch)
    out, gh1 = torch.empty((64, 10), device="cuda"), torch.empty((64, H), device="cuda")
    gw2, gb2, gw3, gb3 = (torch.empty(n, device="cuda") for n in (H * H, H, H * 17, 17))
    nb = int(lib.irbfn_mlp_head_vjp_workspace_bytes(H, H, 10))
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    vjp = lambda h1, O, nbytes: lib.irbfn_mlp_head_vjp(p(h1), p(d["W2"]), p(d["b2"]), p(d["W3"]), p(d["g"]), p(gh1), p(gw2), p(gb2),
                                                       p(gw3), p(gb3), 64, H, H, O, p(ws), nbytes, s)
    assert vjp(d["h1"], 10, nb - 1) == -1                                          # a workspace one byte short: BAD_ARG
    assert vjp(d["h1"], 17, nb) == -2 and lib.irbfn_mlp_head_vjp_workspace_bytes(H, H, 17) == -2     # O = 17: UNSUPPORTED
    assert vjp(d["h1"], 10, nb) == 0
    # h1 at a float offset that is not a multiple of 4 (16 bytes): BAD_ARG from all three entry points; the same rows aligned: OK
    buf = torch.zeros(64 * H + 8, device="cuda")
    for shift in (1, 2, 3):
        h1 = buf[shift:shift + 64 * H].view(64, H)
        h1.copy_(d["h1"])
        assert h1.data_ptr() % 16 != 0
        assert vjp(h1, 10, nb) == -1
        assert lib.irbfn_mlp_head_forward(p(h1), p(d["W2"]), p(d["b2"]), p(d["W3"]), p(d["b3"]), p(out), 64, H, H, 10, s) == -1
        assert lib.irbfn_mlp_head_tick(p(h1), p(d["W2"]), p(d["b2"]), p(d["W3"]), p(d["b3"]), _lib.ROLLOUT_FRENET_LS, None, None, None,
                                       p(out), None, 64, H, H, 10, 5, s) == -1
    h1 = buf[4:4 + 64 * H].view(64, H)
    h1.copy_(d["h1"])
    ref = hu.gpu_forward(d["h1"], d["W2"], d["b2"], d["W3"], d["b3"])
    assert torch.equal(hu.gpu_forward(h1, d["W2"], d["b2"], d["W3"], d["b3"]), ref)


def test_two_half_batches_add_up_to_the_whole(gpu):
    """gh1 of the halves is the whole batch's, bit for bit (rows are independent).  The summed leaves of the halves add up to
    the whole batch's within bound B applied to the three evaluations, each on its own scale: the sum of their any-order
    worst cases, and 4 x the sum of what float32 NumPy makes of the same three inputs."""
    B, cut = 40001, 17003
    c, _ = hu.real_case(B, 10, seed=21)
    cases = [c] + [dict(c, h1=c["h1"][s], g=c["g"][s]) for s in (slice(0, cut), slice(cut, B))]
    whole, *halves = [_bwd(q) for q in cases]
    assert np.array_equal(np.concatenate([h["gh1"] for h in halves]), whole["gh1"])
    refs = [_ref_bwd(q) for q in cases]
    r32 = [hu.backward32(q["h1"], q["W2"], q["b2"], q["W3"], q["g"]) for q in cases]
    for k in hu.LEAF_NAMES:
        worst = sum(hu.any_order_bound(q["h1"].shape[0] + 80) * r["S" + k] for q, r in zip(cases, refs))
        tol32 = 4 * sum(hu.worst_ratio(n[k], r[k], r["S" + k]) * r["S" + k] for n, r in zip(r32, refs))
        diff = np.abs(halves[0][k].astype(np.float64) + halves[1][k].astype(np.float64) - whole[k])
        print(f"[head] halves {k}: max |sum of halves - whole| / (4 x float32 NumPy) = {(diff / tol32).max():.2e}, "
              f"/ any-order worst case = {(diff / worst).max():.2e}")
        assert (diff <= worst).all() and (diff <= tol32).all(), k


# ------------------------------------------------------------------ D: non-finite rows
def _spoiled(c, B):
    """NaN, +Inf and -Inf at single entries of h1: rows inside a 32-row tile and last rows of a tile, the batch's last row."""
    h1 = c["h1"].copy()
    marks = {(5, 7): np.nan, (31, 0): np.inf, (63, 63): -np.inf, (100, 33): np.inf, (127, 12): np.nan, (B - 1, 20): np.nan,
             (B - 40, 40): -np.inf}
    for (r, col), v in marks.items():
        h1[r, col] = v
    return dict(c, h1=h1), sorted({r for r, _ in marks})


@pytest.mark.parametrize("B,O", [(200, 10), (33001, 3), (33001, 16)])
def test_non_finite_rows_follow_the_reference(gpu, B, O):
    """Lattice values, so that everything finite is exact: out and the five gradients equal the NumPy reference, NaN where it
    has NaN and the same +-Inf; the other rows' out and gh1 are the clean run's, bit for bit."""
    c = hu.lattice_case(B, O, seed=B + O)
    assert hu.lattice_is_exact(c)
    bad, rows = _spoiled(c, B)
    clean_rows = np.setdiff1d(np.arange(B), rows)
    out, clean_out = _fwd(bad), _fwd(c)
    ref_out = _ref_fwd(bad)["out"]
    assert np.isnan(ref_out[5]).all() and np.isnan(ref_out[B - 1]).all()           # the reference propagates NaN
    assert np.array_equal(out.astype(np.float64), ref_out, equal_nan=True), np.flatnonzero((out != ref_out).any(1) & ~np.isnan(ref_out).any(1))
    assert np.array_equal(out[clean_rows], clean_out[clean_rows])
    got, clean, ref = _bwd(bad), _bwd(c), _ref_bwd(bad)
    assert np.isnan(ref["gw3"]).any() and np.isnan(ref["gw2"]).any()
    for k in GRADS:
        assert np.array_equal(got[k].astype(np.float64), ref[k], equal_nan=True), k
    assert np.array_equal(got["gh1"][clean_rows], clean["gh1"][clean_rows])
    # the tick's controls are the forward's
    d = [hu.dev(bad[k]) for k in ("h1", "W2", "b2", "W3", "b3")]
    if O % 2 == 0:
        ctrl = torch.empty((B, O), device="cuda")
        st = _lib.load().irbfn_mlp_head_tick(*(hu._ptr(t) for t in d), _lib.ROLLOUT_FRENET_LS, None, None, None, hu._ptr(ctrl), None,
                                             B, H, H, O, O // 2, _stream_ptr(torch))
        assert st == 0 and np.array_equal(ctrl.cpu().numpy(), out, equal_nan=True)


@pytest.mark.parametrize("O", [20, 100])
def test_non_finite_rows_in_the_wide_forward(gpu, O):
    B = 300
    c = hu.lattice_case(B, O, seed=O)
    bad, rows = _spoiled(c, B)
    out, ref = _fwd(bad), _ref_fwd(bad)["out"]
    assert np.isnan(ref[5]).all()
    assert np.array_equal(out.astype(np.float64), ref, equal_nan=True)


def test_a_nan_query_gives_a_nan_row_end_to_end(gpu):
    """The golden net: a NaN query row gives a NaN output row from DeeperWCRBFNet.apply and a NaN controls row from
    planner.plan_tick; the other rows are unchanged.  (Nothing is asserted on the states of that row: the roll-out clips.)"""
    cfg, P = _golden_f32()
    net = DeeperWCRBFNet.from_config(cfg)
    B, T = 300, cfg["out_features"] // 2
    x = _golden_queries(cfg, B, seed=3)
    rng = np.random.default_rng(4)
    st = np.hstack([rng.normal(size=(B, 1)) * 0.2, rng.normal(size=(B, 1)) * 0.2, rng.normal(size=(B, 1)) * 0.1,
                    rng.uniform(1, 6, size=(B, 1)), rng.normal(size=(B, 3)) * 0.1, rng.normal(size=(B, 1)) * 0.05]).astype(np.float32)
    mirror = (rng.random(B) < 0.5).astype(np.int32)
    bad = x.copy()
    bad[[7, 31, 290], [2, 0, 5]] = np.nan
    rows = [7, 31, 290]
    others = np.setdiff1d(np.arange(B), rows)
    clean_out, out = net.apply(P, x), net.apply(P, bad)
    print(f"[head] end to end: stage kernel {net.stage.last_launch()['kernel']}")
    assert np.isnan(out[rows]).all() and np.array_equal(out[others], clean_out[others])
    tick = lambda q: planner.plan_tick(net, P, torch.from_numpy(q).cuda(), torch.from_numpy(mirror).cuda(), torch.from_numpy(st).cuda(),
                                       configs.DYN_PARAMS, mode=_lib.ROLLOUT_FRENET_LS)
    (c0, s0), (c1, s1) = tick(x), tick(bad)
    c0, c1, s0, s1 = (t.cpu().numpy() for t in (c0, c1, s0, s1))
    assert np.isnan(c1[rows]).all() and np.array_equal(c1[others], c0[others]) and np.array_equal(s1[others], s0[others])


# ------------------------------------------------------------------ E: one training step at the reference's batch
def test_deeper_train_step_at_the_reference_batch(gpu):
    """train_step_frenet_fullint on the golden net at B = 80 000 (scripts/train_nmpc_frenet.py's batch: a wave of the head's
    backward walks three tiles) against float64 torch.autograd, accumulated over row chunks, under the bounds of
    tests/test_gpu_deeper_train.py::_check_step."""
    from test_gpu_deeper_train import DP, LEAVES, _check_step, _golden, _tparams
    B, chunk = 80000, 8000
    cfg, P, x, y = _golden(B=B, seed=31)
    tp = _tparams(P)
    xt, yt = torch.tensor(x, dtype=torch.float64), torch.tensor(y, dtype=torch.float64)
    loss_ref = 0.0
    for i in range(0, B, chunk):                           # the two means of _frenet_loss as sums over the chunks
        xs, ys = xt[i:i + chunk], yt[i:i + chunk]
        y_pred = orc.deeper_wcrbfnet_apply(cfg, tp, xs)
        init = xs[:, [0, 0, 1, 2, 3, 5, 6, 7]]
        actual = orc.integrate_frenet_mult(torch.hstack((init, ys)), DP)
        pred = orc.integrate_frenet_mult(torch.hstack((init, y_pred)), DP)
        part = (y_pred - ys).abs().sum() / (B * ys.shape[1]) + (pred - actual).abs().sum() / (B * pred[0].numel())
        part.backward()
        loss_ref += float(part.detach())
    g = np.concatenate([tp["params"][g_][n].grad.numpy().reshape(-1) for g_, n in LEAVES])
    flat = np.concatenate([np.asarray(P["params"][g_][n], np.float64).reshape(-1) for g_, n in LEAVES])
    p_new, _, _ = orc.adam_update(flat, orc.clip_by_global_norm(g, 1.0), np.zeros_like(flat), np.zeros_like(flat), 1, lr=1e-3)
    net = DeeperWCRBFNet.from_config(cfg)
    state = train.DeeperTrainState.create(net, P, lr=1e-3, max_grad_norm=1.0)
    state, loss = train.train_step_frenet_fullint(state, torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), DP)
    print(f"[head] train step B={B}: loss {float(loss):.8f} (float64 {loss_ref:.8f}), "
          f"max |g - g64| / max |g64| = {np.abs(state.g.cpu().numpy() - g).max() / np.abs(g).max():.2e}")
    _check_step(state, loss, (loss_ref, g, p_new))
