"""The loss-seed, clip + Adam and cross-entropy kernels (irbfn_amd/csrc/train_step.hip; softmax_xent of rbf_vjp.hip) through their C
ABI, y_pred given as data, against the float64 statements of tests/_train_step_util.py (their own checks:
tests/test_train_step_reference_cpu.py).  Every output buffer and `partials` is NaN before every call, so an element a kernel
leaves unwritten, or a partial it reads without having written it, shows.

float32 bound (tests/_rollout_util.assert_states_close over the whole case): |err| <= 1e-5 (|ref| + scale), or 4 x the error of the
float32 NumPy statement on the same inputs + 1e-7 scale; scale = max |ref| of the case (lr for the Adam update).  The float32
statement's error is measured in the test.  float64 bounds are those of tests/test_gpu_train_f64.py (loss 1e-12 |ref|, gy 1e-10
max |gy_ref|, Adam 1e-13 max |p|).  Rows the float64 statement flags as ambiguous (within 1e-5 of a kink without sitting on it:
_train_step_util) are checked for finiteness only in float32, and their share is capped at 5 % in every case.

The test ids name the kernel instance a case runs (the Frenet seeds under the name they had before they became instances of
seeds_multistep_kernel, see instance()); each prints its largest err / bound (pytest -s; profiles/train_step_parity.txt)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _train_step_util as tu
from irbfn_amd import _lib, configs
from irbfn_amd.model import _ptr, _stream_ptr

pytestmark = pytest.mark.gpu

NP = {False: np.float32, True: np.float64}
BIG = 262144 + 257                       # the seed kernels stride from 1024 x 256 rows
TIES = (0.0, 0.5, 1.0)
REF_N = {"oneint": 2, "fullint": 5, "frenet": 5}
TIGHT_D = {"oneint": 7, "fullint": 1, "frenet": 8}
ENTRY = {"oneint": "irbfn_train_seeds_oneint", "fullint": "irbfn_train_seeds_fullint", "frenet": "irbfn_train_seeds_frenet_fullint"}


def _dp(f64):
    """the dynamics parameters as the ABI receives them: (host array, the same values in float64)"""
    host = np.array(configs.DYN_PARAMS, NP[f64])
    return host, host.astype(np.float64)


def instance(kind, n, f64):
    """the kernel instance the launchers of train_step.hip pick (frenet: seeds_multistep_kernel<FRENET_LS, 5 / 16, S>, under the
    name the test ids have carried since before it was folded with the single-track seeds)"""
    if kind == "oneint":
        return "seeds_oneint_kernel<%s>" % ("double" if f64 else "float")
    if kind == "frenet":
        return "seeds_frenet_fullint_kernel<%d,%s>" % (5 if n <= 5 else 16, "double" if f64 else "float")
    if f64:
        return "seeds_fullint_f64_kernel<%d>" % (8 if n <= 8 else 64)
    return "seeds_fullint_kernel<8,5>" if n == 5 else ("seeds_fullint_kernel<8>" if n <= 8 else "seeds_fullint_kernel<64>")


def _id(kind, n, D, B, f64=False):
    return f"{instance(kind, n, f64)}-n{n}-D{D}-B{B}"


def _nan(shape, f64):
    return torch.full(shape, float("nan"), dtype=torch.float64 if f64 else torch.float32, device="cuda")


def _dev(a, f64):
    return torch.from_numpy(np.ascontiguousarray(a, NP[f64])).cuda()


def call_seeds(kind, x, yp, y, tie, f64=False, partials=None, gy=None):
    """-> (status, gy, loss) of one call of the entry point on NaN-filled gy / loss / partials"""
    lib = _lib.load()
    B, O = yp.shape
    xd, ypd, yd = _dev(x, f64), _dev(yp, f64), _dev(y, f64)
    gy = _nan((B, O), f64) if gy is None else gy
    loss = _nan((1,), f64)
    partials = _nan((lib.irbfn_train_loss_partials(),), f64) if partials is None else partials
    fn = getattr(lib, ENTRY[kind] + ("_f64" if f64 else ""))
    host, _ = _dp(f64)
    head = (_ptr(xd), _ptr(ypd), _ptr(yd)) + (() if kind == "fullint" else (host.ctypes.data_as(C.c_void_p),))
    st = fn(*head, float(tie), _ptr(gy), _ptr(loss), _ptr(partials), B, x.shape[1], O if kind == "oneint" else O // 2, _stream_ptr(torch))
    torch.cuda.synchronize()
    return st, gy.cpu().numpy(), float(loss.item())


def statement(kind, x, yp, y, tie, f64, B_total=None):
    dp = _dp(f64)[1]
    with np.errstate(invalid="ignore", over="ignore"):
        if kind == "fullint":
            return tu.seeds_fullint(x, yp, y, tie, B_total)
        return (tu.seeds_oneint if kind == "oneint" else tu.seeds_frenet_fullint)(x, yp, y, dp, tie, B_total)


def statement32(kind, x, yp, y, tie, B_total=None):
    with np.errstate(invalid="ignore", over="ignore"):
        if kind == "fullint":
            return tu.seeds_fullint_f32(x, yp, y, tie, B_total)
        return (tu.seeds_oneint_f32 if kind == "oneint" else tu.seeds_frenet_fullint_f32)(x, yp, y, _dp(False)[0], tie, B_total)


def _rows(B):
    return (0, B - 1, BIG - 100 if B == BIG else 1)


@functools.lru_cache(maxsize=None)
def case(kind, n, D, B, f64=False):
    """One seeded batch with its tie / zero rows, and per tie the float64 statement (and the float32 one for float32 cases):
    computed once, shared by the tests, never written to.  At B = 262 401 only tie = 0.5 is stated for every row; tie = 0 and 1
    are stated for the spliced rows and the rows from 1000 before the stride boundary to the end, normalised by the whole batch (B_total) --
    the other rows' gy does not depend on tie, which the tests assert of the kernel's output bit for bit."""
    seed = 1000 * n + 10 * D + B % 1000 + (7 if f64 else 0)
    make = {"oneint": tu.oneint_case, "fullint": tu.fullint_case, "frenet": tu.frenet_case}[kind]
    x, yp, y = make(B, n, D, seed)
    used = tu.splice_rows(kind, x, yp, y, _rows(B), _dp(f64)[1])
    some = np.union1d(sorted(used.values()), np.arange(262144 - 1000, B)) if B == BIG else None
    refs = {}
    for tie in TIES:
        rows = None if tie == 0.5 else some
        sub = (x, yp, y) if rows is None else (x[rows], yp[rows], y[rows])
        loss, gy, amb = statement(kind, *sub, tie, f64, B)
        loss32, gy32 = (None, None) if f64 else statement32(kind, *sub, tie, B)
        refs[tie] = dict(loss=loss, gy=gy, amb=amb, loss32=loss32, gy32=gy32, rows=rows)
    for a in (x, yp, y):
        a.setflags(write=False)
    return dict(kind=kind, n=n, x=x, yp=yp, y=y, used=used, refs=refs)


def check_seeds32(c, tie, what):
    """one float32 call of case c at `tie` under the float32 rule; returns gy and the loss"""
    kind, r = c["kind"], c["refs"][tie]
    rows = slice(None) if r["rows"] is None else r["rows"]
    amb, gy_ref, gy32 = r["amb"], r["gy"], r["gy32"]
    st, gy, loss = call_seeds(kind, c["x"], c["yp"], c["y"], tie)
    assert st == 0
    print(f"[train_step] {what} tie={tie}: ambiguous rows {100 * amb.mean():.2f} % (cap 5 %)")
    assert amb.mean() <= tu.AMBIGUOUS_CAP
    assert np.isfinite(gy).all()
    keep = ~amb
    # the float32 statement itself is within rounding of the float64 one on the rows kept: had it taken the other side of a kink
    # (an error of sgn / (B T 8) or more, >= 8e-3 of the scale in these cases), 4 x its error would make the bound below vacuous.
    # Rounding: <= 64 steps x a few float32 ulps of O(1) states, 3e-5 of the scale at the longest horizons; 1e-4 sits between.
    e32 = np.abs(gy32[keep].astype(np.float64) - gy_ref[keep]).max() / np.abs(gy_ref[keep]).max()
    print(f"[train_step] {what} tie={tie}: float32 statement max |err| / scale {e32:.2e}")
    assert e32 <= tu.TWIN_CAP, (what, tie, e32)
    r_gy = tu.ratio32(gy[rows][keep], gy_ref[keep], gy32[keep])
    r_loss = tu.ratio32([loss], [r["loss"]], [r["loss32"]]) if r["rows"] is None else 0.0     # stated for the whole batch only
    print(f"[train_step] {what} tie={tie}: gy err/bound {r_gy:.3g}, loss err/bound {r_loss:.3g}")
    assert r_gy <= 1.0 and r_loss <= 1.0, (what, tie, r_gy, r_loss)
    full_amb = c["refs"][0.5]["amb"]
    for name, row in c["used"].items():                      # the spliced rows are not ambiguous: they sit ON their kinks
        assert not full_amb[row], name
    if "zero" in c["used"]:                                  # y_pred == y: both roll-outs are the same arithmetic, sgn(0) = 0
        assert (gy[c["used"]["zero"]] == 0).all()
    return gy, loss


def check_ties32(c, what):
    """tie = 0, 0.5, 1: each under the rule at its own reference; the tie rows move with tie, and no other unambiguous row changes a bit"""
    out = {tie: check_seeds32(c, tie, what) for tie in TIES}
    g = {tie: o[0] for tie, o in out.items()}
    assert out[0.0][1] == out[0.5][1] == out[1.0][1]          # the loss does not depend on tie
    ties = [c["used"][k] for k in ("tie_lo", "tie_hi") if k in c["used"]]
    # an ambiguous row may sit exactly ON a bound in float32 (7 + 0.1 a rounds to 7 for |a| < 2.4e-6: one row of the 262 401 of the
    # fullint case does), where the kernel rightly answers with `tie`: the rows that must not move are the unambiguous ones
    others = np.setdiff1d(np.flatnonzero(~c["refs"][0.5]["amb"]), ties)
    assert np.array_equal(g[0.0][others], g[0.5][others]) and np.array_equal(g[0.0][others], g[1.0][others])
    for r in ties:
        assert (g[1.0][r] != g[0.0][r]).any(), r


# ------------------------------------------------------------------ seed kernels, float32
HORIZONS = ([("fullint", n, D) for n in (1, 4, 5, 6, 8, 9, 64) for D in (1, 7)] + [("frenet", n, D) for n in (1, 5, 6, 16) for D in (8, 10)]
            + [("oneint", n, D) for n in (2, 3, 10) for D in (7, 9)])
BATCHES = [(kind, B) for kind in ("oneint", "fullint", "frenet") for B in (1, 255, 256, 257, 1000)]


@pytest.mark.parametrize("kind,n,D", HORIZONS, ids=[_id(k, n, D, 1000) for k, n, D in HORIZONS])
def test_seeds_f32_every_horizon_and_row_pitch(gpu, kind, n, D):
    check_ties32(case(kind, n, D, 1000), _id(kind, n, D, 1000))


@pytest.mark.parametrize("kind,B", BATCHES, ids=[_id(k, REF_N[k], TIGHT_D[k], B) for k, B in BATCHES])
def test_seeds_f32_batch_sizes(gpu, kind, B):
    check_ties32(case(kind, REF_N[kind], TIGHT_D[kind], B), _id(kind, REF_N[kind], TIGHT_D[kind], B))


@pytest.mark.parametrize("kind", ["oneint", "fullint", "frenet"], ids=[_id(k, REF_N[k], TIGHT_D[k], BIG) for k in ("oneint", "fullint", "frenet")])
def test_seeds_f32_grid_stride(gpu, kind):
    """B = 262 144 + 257: the last 257 rows are a block's second pass; tie rows at 0 and B - 1, the zero row at 262 301."""
    c = case(kind, REF_N[kind], TIGHT_D[kind], BIG)
    assert c["used"]["tie_hi"] >= 262144 and c["used"]["zero"] >= 262144
    check_ties32(c, _id(kind, REF_N[kind], TIGHT_D[kind], BIG))


REPEAT = [("oneint", 2, BIG), ("fullint", 5, 70001), ("fullint", 6, 1000), ("fullint", 64, 1000), ("frenet", 5, 70001), ("frenet", 16, 1000)]


@pytest.mark.parametrize("f64", [False, True], ids=["float", "double"])
@pytest.mark.parametrize("kind,n,B", REPEAT, ids=[f"{k}-n{n}-B{B}" for k, n, B in REPEAT])
def test_seeds_repeat_call_is_bit_equal(gpu, kind, n, B, f64):
    """the loss is a two-stage sum in a fixed order: two calls agree in every bit of gy and of the loss"""
    make = {"oneint": tu.oneint_case, "fullint": tu.fullint_case, "frenet": tu.frenet_case}[kind]
    x, yp, y = make(B, n, TIGHT_D[kind], seed=B + n)
    a = call_seeds(kind, x, yp, y, 0.5, f64)
    b = call_seeds(kind, x, yp, y, 0.5, f64)
    assert a[0] == 0 and np.array_equal(a[1], b[1]) and a[2] == b[2] and np.isfinite(a[2]) and np.isfinite(a[1]).all()


@pytest.mark.parametrize("f64", [False, True], ids=["float", "double"])
@pytest.mark.parametrize("kind", ["oneint", "fullint", "frenet"])
def test_seeds_empty_batch(gpu, kind, f64):
    """B = 0: IRBFN_OK, loss 0, gy untouched (and no row pointer is needed)."""
    lib = _lib.load()
    n, D = REF_N[kind], TIGHT_D[kind]
    guard, loss, partials = _nan((64,), f64), _nan((1,), f64), _nan((lib.irbfn_train_loss_partials(),), f64)
    fn = getattr(lib, ENTRY[kind] + ("_f64" if f64 else ""))
    host, _ = _dp(f64)
    null = C.c_void_p(None)
    for rows in (null, _ptr(guard)):
        head = (rows, rows, rows) + (() if kind == "fullint" else (host.ctypes.data_as(C.c_void_p),))
        loss.fill_(float("nan"))
        st = fn(*head, 0.5, _ptr(guard), _ptr(loss), _ptr(partials), 0, D, n, _stream_ptr(torch))
        torch.cuda.synchronize()
        assert st == 0 and float(loss.item()) == 0.0 and bool(torch.isnan(guard).all())


def _with_rows(c, marks, which):
    """copies of the case's arrays with marks {(row, col): value} written into `which` (x / yp / y)"""
    a = {k: c[k].copy() for k in ("x", "yp", "y")}
    for (r, col), v in marks.items():
        a[which][r, col] = v
    return a


@pytest.mark.parametrize("kind,n", [("oneint", 2), ("oneint", 3), ("fullint", 5), ("fullint", 6), ("fullint", 9), ("fullint", 64), ("frenet", 5),
                                    ("frenet", 6), ("frenet", 16)], ids=lambda v: str(v))
def test_seeds_f32_infinite_predictions_are_ordinary_rows(gpu, kind, n):
    """+-Inf in y_pred: clip maps it to a bound, so the roll-out and its adjoint stay finite and the reference has an answer --
    an infinite loss wherever the prediction loss covers that column (every column but the inner ones of fullint), an infinite
    gy entry for the L2 loss of oneint.  Compared like any other row: finite entries under the rule, infinite ones exactly.
    (fullint: the columns are inner ones, 1 and T + 1, where only the roll-out sees the prediction.)"""
    B = 1000
    c = case(kind, n, TIGHT_D[kind], B)
    O = c["yp"].shape[1]
    cols = (1, n + 1) if kind == "fullint" else (0, O - 1)
    clear = np.setdiff1d(np.flatnonzero(~c["refs"][0.5]["amb"]), list(c["used"].values()))
    r0, r1, r2 = clear[0], clear[len(clear) // 2], clear[-1]
    a = _with_rows(c, {(r0, cols[0]): np.inf, (r1, cols[1]): -np.inf, (r2, cols[0]): -np.inf, (r2, cols[1]): np.inf}, "yp")
    with np.errstate(invalid="ignore", over="ignore"):
        loss_ref, gy_ref, amb = statement(kind, a["x"], a["yp"], a["y"], 0.5, False)
    loss32, gy32 = statement32(kind, a["x"], a["yp"], a["y"], 0.5)
    assert not np.isnan(gy_ref).any() and (~amb[[r0, r1, r2]]).sum() >= 2 and np.isinf(loss_ref) == (kind != "fullint")
    st, gy, loss = call_seeds(kind, a["x"], a["yp"], a["y"], 0.5)
    keep = ~amb
    r = tu.ratio32(gy[keep], gy_ref[keep], gy32[keep])
    print(f"[train_step] {instance(kind, n, False)} Inf rows: gy err/bound {r:.3g}")
    assert st == 0 and r <= 1.0
    assert tu.ratio32([loss], [loss_ref], [loss32]) <= 1.0


@pytest.mark.parametrize("which", ["x", "yp", "y"])
@pytest.mark.parametrize("kind,n", [("oneint", 2), ("fullint", 5), ("fullint", 6), ("fullint", 9), ("fullint", 64), ("frenet", 5), ("frenet", 6),
                                    ("frenet", 16)], ids=lambda v: str(v))
def test_seeds_f32_a_nan_row_spoils_the_loss_and_no_other_row(gpu, kind, n, which):
    """A NaN in x, y_pred or y of one row: the loss is NaN, and every other row's gy is bit-equal to the same batch with that row
    finite.  The NaN row's own gy is deliberately not pinned: the kernels' sgn(NaN) is 0 as torch.sign's is, where jnp.sign(NaN)
    is NaN, and JAX -- the reference's framework -- is not among this project's test dependencies to arbitrate."""
    B = 600
    c = case(kind, n, TIGHT_D[kind], 1000)
    clean = {k: c[k][:B] for k in ("x", "yp", "y")}
    col = {"x": 0, "yp": c["yp"].shape[1] - 1, "y": 0}[which]
    bad = {k: v.copy() for k, v in clean.items()}
    bad[which][257, col] = np.nan
    st0, gy0, loss0 = call_seeds(kind, clean["x"], clean["yp"], clean["y"], 0.5)
    st1, gy1, loss1 = call_seeds(kind, bad["x"], bad["yp"], bad["y"], 0.5)
    others = np.setdiff1d(np.arange(B), [257])
    assert st0 == 0 and st1 == 0 and np.isfinite(loss0) and np.isnan(loss1)
    assert np.array_equal(gy0[others], gy1[others]) and np.isfinite(gy1[others]).all()


# ------------------------------------------------------------------ seed kernels, float64
F64_CASES = [(k, n, D, (257, 1000)[i % 2]) for i, (k, n, D) in enumerate(HORIZONS)]
F64_CASES += [(k, REF_N[k], TIGHT_D[k], B) for k in ("oneint", "fullint", "frenet") for B in (1, 257, 1000)
              if (k, REF_N[k], TIGHT_D[k], B) not in F64_CASES] + [("oneint", 2, 7, BIG)]


@pytest.mark.parametrize("kind,n,D,B", F64_CASES, ids=[_id(k, n, D, B, True) for k, n, D, B in F64_CASES])
def test_seeds_f64(gpu, kind, n, D, B):
    c = case(kind, n, D, B, True)
    g = {}
    for tie in TIES:
        r = c["refs"][tie]
        rows = slice(None) if r["rows"] is None else r["rows"]
        loss_ref, gy_ref, amb = c["refs"][0.5]["loss"], r["gy"], r["amb"]
        assert amb.mean() <= tu.AMBIGUOUS_CAP
        st, gy, loss = call_seeds(kind, c["x"], c["yp"], c["y"], tie, True)
        e_loss, e_gy = abs(loss - loss_ref) / (1e-12 * abs(loss_ref)), np.abs(gy[rows] - gy_ref).max() / (1e-10 * np.abs(gy_ref).max())
        print(f"[train_step] {_id(kind, n, D, B, True)} tie={tie}: gy err/bound {e_gy:.3g}, loss err/bound {e_loss:.3g}, "
              f"ambiguous rows {100 * amb.mean():.2f} % (cap 5 %)")
        assert st == 0 and e_loss <= 1.0 and e_gy <= 1.0
        g[tie] = gy
    ties = [c["used"][k] for k in ("tie_lo", "tie_hi") if k in c["used"]]
    others = np.setdiff1d(np.arange(B), ties)
    assert np.array_equal(g[0.0][others], g[0.5][others]) and np.array_equal(g[0.0][others], g[1.0][others])
    if "zero" in c["used"]:
        assert (g[0.5][c["used"]["zero"]] == 0).all()


# ------------------------------------------------------------------ clip + Adam
HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)


def _hyper(f64):
    """the hyper-parameters as the ABI receives them (rounded to float32 first for the float32 entry point)"""
    return {k: float(NP[f64](v)) for k, v in HYPER.items()}


def call_adam(p, g, m, v, step, max_norm, f64, partials=None):
    """one irbfn_adam_clip_step[_f64] on device tensors, in place"""
    lib = _lib.load()
    h = _hyper(f64)
    partials = _nan((lib.irbfn_train_loss_partials(),), f64) if partials is None else partials
    fn = lib.irbfn_adam_clip_step_f64 if f64 else lib.irbfn_adam_clip_step
    st = fn(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), _ptr(step), h["lr"], h["b1"], h["b2"], h["eps"], float(NP[f64](max_norm)),
            _ptr(partials), _stream_ptr(torch))
    torch.cuda.synchronize()
    return st


def adam_state(n, seed, f64, step0):
    rng = np.random.default_rng(seed)
    ft = NP[f64]
    p, g = (rng.normal(size=n) * 0.01).astype(ft), (rng.normal(size=n) * 0.01).astype(ft)
    m, v = (rng.normal(size=n) * 0.1).astype(ft), (rng.uniform(0.5, 1.5, size=n) * 0.01).astype(ft)
    return [torch.from_numpy(a).cuda() for a in (p, g, m, v)] + [torch.tensor([step0], dtype=torch.int32, device="cuda")]


def check_adam(p, g, m, v, step, max_norm, f64, what, partials=None):
    """one call from the device's own state against the float64 statement"""
    h = _hyper(f64)
    p0, g0, m0, v0 = (t.cpu().numpy() for t in (p, g, m, v))
    t = int(step.item()) + 1
    mn = float(NP[f64](max_norm))
    ref = tu.adam_clip(*(a.astype(np.float64) for a in (p0, g0, m0, v0)), t, h["lr"], h["b1"], h["b2"], h["eps"], mn)
    assert call_adam(p, g, m, v, step, max_norm, f64, partials) == 0
    assert int(step.item()) == t
    got = [a.cpu().numpy() for a in (p, m, v)]
    if p0.size == 0:
        return
    upd, upd_ref = got[0].astype(np.float64) - p0, ref[0] - p0
    if f64:
        errs = [tu.rel64(upd, upd_ref, 1e-13 * np.nanmax(np.abs(ref[0]))), tu.rel64(got[1], ref[1], 1e-13 * np.nanmax(np.abs(ref[1]))),
                tu.rel64(got[2], ref[2], 1e-13 * np.nanmax(np.abs(ref[2])))]
    else:
        r32 = tu.adam_clip(p0, g0, m0, v0, t, h["lr"], h["b1"], h["b2"], h["eps"], mn)
        errs = [tu.ratio32(upd, upd_ref, r32[0].astype(np.float64) - p0, scale=h["lr"]), tu.ratio32(got[1], ref[1], r32[1]), tu.ratio32(got[2], ref[2], r32[2])]
    print(f"[train_step] {what} t={t} max_norm={max_norm}: err/bound update {errs[0]:.3g}, m {errs[1]:.3g}, v {errs[2]:.3g}")
    assert max(errs) <= 1.0, (what, t, errs)


ADAM_N = (0, 1, 255, 256, 257, 65536, 65537, 262144, 262145, 300001)


@pytest.mark.parametrize("f64", [False, True], ids=["adam_clip_kernel<float>", "adam_clip_kernel<double>"])
@pytest.mark.parametrize("n,step0", [(n, (0, 1, 999)[i % 3]) for i, n in enumerate(ADAM_N)])
def test_adam_clip_three_calls_from_a_running_state(gpu, n, step0, f64):
    """random m, positive v, a resumed count; n around the strides of sqnorm_partial_kernel (65 536) and adam_clip_kernel
    (262 144); max_norm 1 (clips from n of a few thousand), 1e-3 (always clips), 0 (never)."""
    p, g, m, v, step = adam_state(n, n + step0, f64, step0)
    for k, max_norm in enumerate((1.0, 1e-3, 0.0)):
        check_adam(p, g, m, v, step, max_norm, f64, f"adam n={n}")
        g.mul_(0.5).add_(torch.roll(g, 1) * 0.25 if n else g)
    assert int(step.item()) == step0 + 3


@pytest.mark.parametrize("f64", [False, True], ids=["adam_clip_kernel<float>", "adam_clip_kernel<double>"])
@pytest.mark.parametrize("n", [2, 70001])
def test_adam_clip_edges(gpu, n, f64):
    """g = [3, 4, 0, ...]: ||g|| = 5 exactly.  max_norm = 5 is "not less than", scale 5 / 5 = 1: bit-equal to no clipping, as are
    max_norm = 0 and -1; 4.999 clips; g = 0 gives no NaN."""
    def run(max_norm, gvec=None):
        p, g, m, v, step = adam_state(n, 5, f64, 3)
        g.zero_()
        if gvec is None:
            g[0], g[1] = 3.0, 4.0
        assert call_adam(p, g, m, v, step, max_norm, f64) == 0 and int(step.item()) == 4
        return [t.cpu().numpy() for t in (p, m, v)]
    free = run(0.0)
    for max_norm in (5.0, -1.0, 6.0):
        for a, b in zip(run(max_norm), free):
            assert np.array_equal(a, b), max_norm
    clipped = run(4.999)
    assert not np.array_equal(clipped[1], free[1])
    p, g, m, v, step = adam_state(n, 5, f64, 3)
    g.zero_()
    g[0], g[1] = 3.0, 4.0
    check_adam(p, g, m, v, step, 4.999, f64, f"adam edge n={n}")
    assert all(np.isfinite(a).all() for a in run(1.0, gvec="zero"))


@pytest.mark.parametrize("f64", [False, True], ids=["adam_clip_kernel<float>", "adam_clip_kernel<double>"])
def test_adam_clip_non_finite_gradients(gpu, f64):
    """optax's formula: under a positive max_norm a NaN anywhere in g makes the norm, the scale and every parameter NaN; a single
    +Inf makes the scale 0 (the other gradients vanish) and that one entry Inf * 0 = NaN."""
    n = 70001
    p, g, m, v, step = adam_state(n, 6, f64, 10)
    g[40000] = float("nan")
    assert call_adam(p, g, m, v, step, 1.0, f64) == 0
    assert bool(torch.isnan(p).all()) and int(step.item()) == 11
    p, g, m, v, step = adam_state(n, 6, f64, 10)
    g[40000] = float("inf")
    check_adam(p, g, m, v, step, 1.0, f64, "adam +Inf")          # non-finite reference entries are met exactly
    assert bool(torch.isnan(p[40000])) and int(torch.isnan(p).sum()) == 1 and int(torch.isnan(m).sum()) == 1


@pytest.mark.parametrize("f64", [False, True], ids=["sqnorm_partial_kernel<float>", "sqnorm_partial_kernel<double>"])
def test_adam_step_word_survives_the_seed_kernels_partials(gpu, f64):
    """train.py hands ONE partials buffer to both: a seed call at B = 262 401 fills all 1024 entries, the slot after the 256 norm
    partials -- where sqnorm_partial_kernel parks the incremented step count for adam_clip_kernel -- included.  The count still
    grows by exactly one, the bias correction uses the new count, and what the buffer held before (the seed partials, NaN,
    zeros) changes nothing."""
    lib = _lib.load()
    c = case("oneint", 2, 7, BIG, f64)
    n = 300001
    results = []
    for fill in ("seeds", "nan", "zeros"):
        partials = _nan((lib.irbfn_train_loss_partials(),), f64)
        if fill == "seeds":
            st, _, loss = call_seeds("oneint", c["x"], c["yp"], c["y"], 0.5, f64, partials=partials)
            assert st == 0 and np.isfinite(loss) and bool(torch.isfinite(partials).all())
        elif fill == "zeros":
            partials.zero_()
        p, g, m, v, step = adam_state(n, 8, f64, 999)
        check_adam(p, g, m, v, step, 1.0, f64, f"adam after {fill}", partials=partials)
        check_adam(p, g, m, v, step, 1.0, f64, f"adam after {fill}", partials=partials)
        assert int(step.item()) == 1001
        results.append([t.cpu().numpy() for t in (p, m, v)])
    for other in results[1:]:
        for a, b in zip(other, results[0]):
            assert np.array_equal(a, b)
    # a count of 0 -> 1, where one step more or less changes 1 - b1^t from 0.1 to 0.19
    p, g, m, v, step = adam_state(n, 9, f64, 0)
    check_adam(p, g, m, v, step, 1.0, f64, "adam first step n=300001")


@pytest.mark.parametrize("f64", [False, True], ids=["adam_clip_kernel<float>", "adam_clip_kernel<double>"])
def test_adam_blocks_that_start_late_use_the_parked_count(gpu, f64):
    """Block 0 of adam_clip_kernel stores the new count to step[0] while other blocks may not have started: every block takes
    the count from the word sqnorm_partial_kernel parked, never from step[0].  Matrix products on a second stream keep the
    device busy, so that the 1024 Adam blocks start in several waves; from a count of 0, one step too many turns the
    correction 1 - b1^t from 0.1 into 0.19.  Against a kernel that did read step[0] this test is probabilistic: it tells only
    when the products really delay some blocks (it did in the one recorded run, profiles/train_step_parity.txt).  With the
    kernel as it is the test is deterministic; the guarantee itself is the code and its comment above sqnorm_partial_kernel."""
    n = 300001
    side = torch.cuda.Stream()
    a = torch.randn(4096, 4096, device="cuda")
    b = torch.empty_like(a)
    for k in range(3):
        p, g, m, v, step = adam_state(n, 20 + k, f64, 0)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for _ in range(12):
                torch.mm(a, a, out=b)
        check_adam(p, g, m, v, step, 1.0, f64, f"adam beside a busy stream {k}")
        assert int(step.item()) == 1


# ------------------------------------------------------------------ softmax cross-entropy
def xent_case(B, R, labels, seed):
    rng = np.random.default_rng(seed)
    logits = rng.normal(size=(B, R))
    logits[::6] += 80.0                       # large but inside float32 expf's range (it overflows above 88.7) ...
    logits[1::6] -= 80.0                      # ... and above its underflow (normal down to -87.3): a max-shift is not needed yet
    logits[3::6] += 110.0                     # expf(110) = inf: without the shift by the row maximum the row's loss is inf
    logits[4::6] -= 110.0                     # expf(-110) = 0: without it the sum is 0 and its log -inf
    if B > 8:
        logits[7, : (R + 1) // 2] += 110.0    # both in one row: the small entries' softmax is exactly 0, their log-softmax -220
        logits[7, (R + 1) // 2:] -= 110.0
    logits[B // 2] = 1.25                     # a row of equal logits
    if labels == "onehot":
        lab = np.eye(R)[rng.integers(0, R, B)]
    else:
        lab = rng.uniform(0.0, 1.0, size=(B, R))
        if labels == "soft":
            lab /= lab.sum(axis=1, keepdims=True)
    return tu._f32(logits), tu._f32(lab)


def call_xent(logits, labels, accumulate, loss0=float("nan")):
    lib = _lib.load()
    B, R = logits.shape
    ld, bd = _dev(logits, False), _dev(labels, False)
    g, loss = _nan((B, R), False), torch.full((1,), loss0, device="cuda")
    partials = _nan((lib.irbfn_train_loss_partials(),), False)
    st = lib.irbfn_softmax_xent(_ptr(ld), _ptr(bd), _ptr(g), _ptr(loss), _ptr(partials), accumulate, B, R, _stream_ptr(torch))
    torch.cuda.synchronize()
    return st, g.cpu().numpy(), float(loss.item())


XENT = [(B, R) for R in (1, 2, 12, 500) for B in (1, 257)] + [(B, R) for R in (1, 2, 12) for B in (65536 + 3, 80000)]


@pytest.mark.parametrize("B,R,labels", [(B, R, ("onehot", "soft", "unnormalised")[i % 3]) for i, (B, R) in enumerate(XENT)]
                         + [(257, 12, k) for k in ("onehot", "soft", "unnormalised")])
def test_softmax_xent_kernel(gpu, B, R, labels):
    """irbfn_softmax_xent (softmax_xent_kernel + xent_final_kernel): the rows stride from B = 65 536 whatever R is, so R = 500 stays at the
    small batches.  accumulate = 0 overwrites a NaN loss; accumulate = 1 adds to 2.5; a repeat
    call is bit-equal."""
    logits, lab = xent_case(B, R, labels, seed=B + R)
    loss_ref, g_ref = tu.softmax_xent(logits, lab)
    loss32, g32 = tu.softmax_xent(logits.astype(np.float32), lab.astype(np.float32))
    st, g, loss = call_xent(logits, lab, 0)
    r_g, r_loss = tu.ratio32(g, g_ref, g32), tu.ratio32([loss], [loss_ref], [loss32])
    print(f"[train_step] softmax_xent_kernel B={B} R={R} {labels}: glogits err/bound {r_g:.3g}, loss err/bound {r_loss:.3g}")
    assert st == 0 and r_g <= 1.0 and r_loss <= 1.0
    st2, g2, loss2 = call_xent(logits, lab, 0)
    assert np.array_equal(g, g2) and loss == loss2
    st3, g3, loss3 = call_xent(logits, lab, 1, loss0=2.5)
    assert st3 == 0 and np.array_equal(g, g3) and loss3 == float(np.float32(2.5) + np.float32(loss))
