"""The float64 kernels (irbfn_amd/csrc/rbf_f64.hip) on their own: irbfn_f64_forward, irbfn_f64_vjp and irbfn_f64_vjp_x called
through the C ABI on guarded buffers, against the np.longdouble statement of tests/_f64_util.py, at the edges of their shapes and of
the gate -- the forward's output tiles of 16, the VJP's lane-per-centre padding, the slice rule at its caps and with slices behind the
batch, O = 16 and the refusal at O = 17, every D, nsplit = 0 / < D / = D, fewer and more rows of dimension_ranges than regions, ragged
range tables, the 64 KiB LDS limit of the gate table from both sides, B = 0, every refused argument, non-finite inputs and queries on
centres.  The cases are tests/_f64_util.py::TABLE.

Every call: x and gout carry NaN rows past B and the parameters NaN words behind their last element; out, gx and the four gradient
leaves are NaN-prefilled with GUARD NaN words behind their last element; the workspace is 0x5A-prefilled, handed over with exactly
irbfn_f64_workspace_bytes (which must be what the restated launch rules give) and has a tail behind it.  After the call the guards
and the tail are as they were; a refused call has written nothing at all.  Every successful call runs twice and is bit-identical.

The bound, on every finite element of the statement (tests/_f64_util.py): |got - ref| <= C64 2^-53 S + S_gamma + 1e-300; non-finite
elements exactly where the statement has them.  Each test prints its worst |err| / bound per operation."""
import ctypes as C

import numpy as np
import pytest

import _f64_util as fu
from irbfn_amd import _lib
from irbfn_amd.model import WCRBFNet, _stream_ptr

pytestmark = pytest.mark.gpu

GUARD, WS_TAIL = 64, 256
OK, BAD_ARG, UNSUPPORTED = 0, -1, -2
WORST = {op: 0.0 for op in fu.OPS}


# ------------------------------------------------------------------------------------------------ cards and nets
class Net:
    """A case's parameters on the device, NaN words behind each, and its card: WCRBFNet's own unless one built by hand is given."""

    def __init__(self, torch, case, card=None):
        self.case = case
        self.wc = WCRBFNet.from_config(case.cfg, use_float64=True)
        self.card = card if card is not None else self.wc._f64_card(torch)[0]
        p = case.params["params"]
        self.bufs, self.leaves = {}, {}
        for n, (a, b) in fu.LEAF_PATH.items():             # GUARD NaN words behind every parameter: a read past its end shows in the result
            v = np.ascontiguousarray(p[a][b])
            assert v.dtype == np.float64
            self.bufs[n] = torch.from_numpy(np.concatenate([v.ravel(), np.full(GUARD, np.nan)])).cuda()
            self.leaves[n] = self.bufs[n][:v.size]


def hand_card(torch, case, pad=0.0, n_ranges=None, null_tables=False, **fields):
    """An irbfn_f64_card built from the case's tables -> (card, the tensors it points to).  pad: the entries of lo / hi past a
    coordinate's own ranges; n_ranges: handed over as it is, with every row of dimension_ranges; fields: overrides."""
    ns, mr, lo, hi, delta, dr, nr = case.tables(pad=pad, n_ranges=n_ranges)
    tens = [torch.from_numpy(a).cuda() for a in (lo, hi, delta, dr if dr.size else np.zeros((1, 1), np.int32))]
    ptrs = [None] * 4 if null_tables else [t.data_ptr() for t in tens]
    card = _lib.F64Card(case.D, case.R, case.K, case.O, _lib.BASIS_ENUM[case.basis], ns, 0 if null_tables else mr, nr, *ptrs)
    for f, v in fields.items():
        setattr(card, f, v)
    return card, tens


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ------------------------------------------------------------------------------------------------ one guarded call
POINTERS = {"fwd": ("centers", "log_sigs", "kernel", "bias", "x", "out", "ws"),
            "vjp": ("centers", "log_sigs", "kernel", "x", "gout", "g_centers", "g_log_sigs", "g_kernel", "g_bias", "ws"),
            "vjpx": ("centers", "log_sigs", "kernel", "x", "gout", "gx", "ws")}


def run(torch, op, net, x=None, g=None, B=None, expect=OK, short=0, null=()):
    """One call of the ABI on guarded buffers -> {name: float64 array} (None where the call is refused, which must then have
    written nothing).  B: the batch handed over if it is not len(x); short: bytes taken off workspace_bytes; null: the names of
    pointer arguments (POINTERS) handed over as NULL."""
    lib, case = _lib.load(), net.case
    x = case.x if x is None else x
    g = case.g if g is None else g
    rows = x.shape[0]
    B = rows if B is None else B
    R, K, D, O = case.R, case.K, case.D, case.O
    shapes = {"fwd": {"out": (rows, O)}, "vjpx": {"gx": (rows, D)},
              "vjp": {"g_centers": (R, K, D), "g_log_sigs": (R, K), "g_kernel": (K, O), "g_bias": (O,)}}[op]
    xd = torch.from_numpy(np.vstack([x, np.full((GUARD, D), np.nan)])).cuda()
    gd = torch.from_numpy(np.vstack([g, np.full((GUARD, O), np.nan)])).cuda()
    outs = {n: torch.full((int(np.prod(s)) + GUARD,), float("nan"), dtype=torch.float64, device="cuda") for n, s in shapes.items()}
    need = int(lib.irbfn_f64_workspace_bytes(C.byref(net.card), B, 1 if op == "vjp" else 0))
    if need >= 0 and (net.card.D, net.card.R, net.card.K, net.card.O) == (D, R, K, O):
        plan = fu.f64_plan(R * K, B, D, R, O)
        assert need == plan["bytes_vjp" if op == "vjp" else "bytes_fwd"], (case.tag, op, need, plan)
    ws = torch.full((max(need, 4096) + WS_TAIL,), 0x5A, dtype=torch.uint8, device="cuda")
    ptr = {n: t.data_ptr() for n, t in net.leaves.items()}
    ptr.update(x=xd.data_ptr(), gout=gd.data_ptr(), ws=ws.data_ptr(), **{n: t.data_ptr() for n, t in outs.items()})
    for n in null:
        assert n in POINTERS[op]
        ptr[n] = None
    given = 0 if "ws" in null else max(need, 0) - short
    args = [ptr[n] for n in POINTERS[op][:-1]] + [B, ptr["ws"], given, _stream_ptr(torch)]
    fn = {"fwd": lib.irbfn_f64_forward, "vjp": lib.irbfn_f64_vjp, "vjpx": lib.irbfn_f64_vjp_x}[op]
    st = fn(C.byref(net.card), *args)
    torch.cuda.synchronize()
    return _after(torch, case, op, st, expect, outs, shapes, ws, max(need, 0) if st == OK else 0)


def _after(torch, case, op, st, expect, outs, shapes, ws, used):
    """The status is the expected one; the workspace behind `used` bytes is untouched; the guards are NaN, and so is everything
    where the call was refused."""
    assert st == expect, (case.tag, op, _lib.STATUS_NAMES.get(st, st), "expected", _lib.STATUS_NAMES[expect])
    assert bool((ws[used:] == 0x5A).all()), f"{case.tag} {op}: wrote behind the workspace it asked for"
    res = {}
    for n, s in shapes.items():
        size = int(np.prod(s))
        assert bool(torch.isnan(outs[n][size:]).all()), f"{case.tag} {op}: wrote behind the last element of {n}"
        if st != OK:
            assert bool(torch.isnan(outs[n]).all()), f"{case.tag} {op}: a refused call wrote into {n}"
        res[n[2:] if n.startswith("g_") else n] = outs[n][:size].cpu().numpy().reshape(s)      # the leaves under the parameters' names
    return res if st == OK else None


def run_twice(torch, op, net, **kw):
    got, again = run(torch, op, net, **kw), run(torch, op, net, **kw)
    for n in got:
        assert np.array_equal(_bits(got[n]), _bits(again[n])), f"{net.case.tag} {op} {n}: two runs differ in some bit"
    return got


def check(case, op, got):
    """The bound on every output of the operation; non-finite elements exactly where the statement has them."""
    ref, bad, line = fu.reference(case, op), [], []
    for name, (r, S, Sg) in ref.items():
        assert got[name].dtype == np.float64 and got[name].shape == r.shape
        worst = fu.ratio(got[name], r, S, Sg)
        WORST[op] = max(WORST[op], worst)
        line.append(f"{name} {worst:.3f}")
        if not fu.same_nonfinite(got[name], np.asarray(r, np.float64)):
            bad.append(f"{name}: non-finite elements differ from the statement's")
        if not worst <= 1.0:
            bad.append(f"{name}: |err| / bound {worst:.3f}")
    print(f"F64PARITY {case.tag:32s} {op:5s} " + "  ".join(line) + f"   (worst {op} so far {WORST[op]:.3f})")
    assert not bad, (case.tag, op, bad)
    return ref


def run_case(torch, tag, op, net=None):
    case = fu.Case(fu.BY_TAG[tag]) if net is None else net.case
    net = net or Net(torch, case)
    got = run_twice(torch, op, net)
    return case, net, got, check(case, op, got)


# ------------------------------------------------------------------------------------------------ the table, per operation
SLICE_TAGS = fu.tags("vjp", fu.SLICES)


@pytest.mark.parametrize("tag", fu.tags("fwd"))
def test_forward_cases(gpu, tag):
    run_case(gpu, tag, "fwd")


@pytest.mark.parametrize("tag", [t for t in fu.tags("vjp") if t not in SLICE_TAGS])
def test_vjp_cases(gpu, tag):
    run_case(gpu, tag, "vjp")


@pytest.mark.parametrize("tag", fu.tags("vjpx"))
def test_vjpx_cases(gpu, tag):
    run_case(gpu, tag, "vjpx")


@pytest.mark.parametrize("tag", SLICE_TAGS)
def test_vjp_slice_rule_at_its_caps(gpu, tag):
    """1024 slices of 64 queries; the cap of 1024 with 15 and with 8 slices behind the batch, which still have to write their zero
    slabs into a workspace that holds 0x5A; ceil(B / 64) below 4096 / groups."""
    case, _, _, _ = run_case(gpu, tag, "vjp")
    plan = case.plan()
    assert (plan["slices"], plan["per_slice"], plan["empty"]) == {"slices_b65536": (1024, 64, 0), "slices_b65537": (1024, 65, 15),
                                                                  "slices_b66000": (1024, 65, 8), "slices_n449": (10, 60, 0)}[tag]


# ------------------------------------------------------------------------------------------------ the gate's edges
def test_steep_gate_exact_zeros(gpu):
    """delta = 15: a region no query reaches has exactly 0 in its rows of d centers / d log_sigs, and a query that every region
    weighs 0 returns the bias itself."""
    torch = gpu
    case = fu.Case(fu.BY_TAG["steep"])
    g64 = fu.gate(case, np.float64, tanh_form=True)[0]
    if not ((g64[:, 3] == 0).all() and (g64[[7, 11]] == 0).all() and (g64[:, :3].max(0) > 0.9).all()):
        pytest.fail("test inputs, not the code under test: the exact zeros of the gate are not where the case wants them")
    net = Net(torch, case)
    _, _, grads, _ = run_case(torch, "steep", "vjp", net)
    assert (grads["centers"][3] == 0).all() and (grads["log_sigs"][3] == 0).all()
    assert (grads["centers"][:3] != 0).all() and (grads["log_sigs"][:3] != 0).all()
    _, _, fwd, _ = run_case(torch, "steep", "fwd", net)
    bias = case.params["params"]["linear"]["bias"]
    assert np.array_equal(fwd["out"][7], bias) and np.array_equal(fwd["out"][11], bias)
    _, _, gx, _ = run_case(torch, "steep", "vjpx", net)
    assert (gx["gx"][[7, 11]] == 0).all()


def test_regions_with_tiny_weights_are_held_to_their_own_scale(gpu):
    """Five of six regions weigh 1e-7 .. 1e-14: their gradients are out of sight of a bound relative to the leaf's largest element,
    and in sight of this one."""
    case, _, got, ref = run_case(gpu, "r6_tiny", "vjp")
    r, S, Sg = ref["centers"]
    assert float(np.abs(r[1:]).max()) < 1e-5 * float(np.abs(r[0]).max())
    assert (got["centers"][1:] != 0).any(axis=(1, 2)).all()
    assert float(fu.bound(S, Sg)[1:].max()) < 1e-12 * float(np.abs(r[0]).max())      # what the max-norm bound would have let pass


def test_regions_without_a_row_get_exact_zeros(gpu):
    case, _, got, _ = run_case(gpu, "r6_rows4", "vjp")
    assert (got["centers"][4:] == 0).all() and (got["log_sigs"][4:] == 0).all() and (got["centers"][:4] != 0).any(axis=(1, 2)).all()


@pytest.mark.parametrize("tag,kw", [("r4_rows6", dict(n_ranges=6)), ("r6_rows4", dict(pad=np.nan)), ("d3_o5_n63", dict(null_tables=True)),
                                    ("r2_nsplit0", dict(null_tables=True))])
def test_cards_built_by_hand_equal_the_class_cards_bit_for_bit(gpu, tag, kw):
    """n_ranges > R is clamped; the padding entries of lo / hi (NaN here) are never part of a result; a card without split
    coordinates needs no tables at all."""
    torch = gpu
    case = fu.Case(fu.BY_TAG[tag])
    card, keep = hand_card(torch, case, **kw)
    if "n_ranges" in kw:
        assert card.n_ranges == 6 > card.R == 4
    if "pad" in kw:
        assert bool(torch.isnan(keep[0]).any()) and bool(torch.isnan(keep[1]).any())
    if "null_tables" in kw:
        assert card.nsplit == 0 and card.lo_dev is None and card.dim_ranges_dev is None and card.n_ranges == case.R
    mine, theirs = Net(torch, case, card), Net(torch, case)
    for op in fu.OPS:
        a, b = run_twice(torch, op, mine), run_twice(torch, op, theirs)
        for n in a:
            assert np.array_equal(_bits(a[n]), _bits(b[n])), (tag, op, n)
        check(case, op, a)


def test_nsplit_0_regions_past_n_ranges_stay_zero(gpu):
    torch = gpu
    case = fu.Case(fu.BY_TAG["r2_nsplit0"])
    card, _ = hand_card(torch, case, null_tables=True, n_ranges=1)
    got = run_twice(torch, "vjp", Net(torch, case, card))
    assert (got["centers"][1] == 0).all() and (got["log_sigs"][1] == 0).all() and (got["centers"][0] != 0).all()


# ------------------------------------------------------------------------------------------------ the batch
_FULL = {}


@pytest.mark.parametrize("B", fu.BATCH_EDGES)
def test_batch_edges_and_rows_independent_of_the_batch(gpu, B):
    """One net, one draw: the bound at every B, and the forward's and the x-VJP's rows bit-identical to those of the B = 600 call."""
    torch = gpu
    if not _FULL:
        full = Net(torch, fu.Case(fu.BY_TAG["b600"]))
        _FULL.update(fwd=run(torch, "fwd", full)["out"], vjpx=run(torch, "vjpx", full)["gx"])
    net = None
    for op in fu.OPS:
        case, net, got, _ = run_case(torch, f"b{B}", op, net)
        if op != "vjp":
            name = "out" if op == "fwd" else "gx"
            assert np.array_equal(_bits(got[name]), _bits(_FULL[op][:B])), (B, op)
    assert case.plan()["slices"] == -(-B // 64)


def test_nan_query_changes_only_its_own_row(gpu):
    torch = gpu
    case = fu.Case(fu.BY_TAG["nonfinite_nan_x"])
    net = Net(torch, case)
    clean = case.x.copy()
    clean[23, 3] = 0.5
    for op, name in (("fwd", "out"), ("vjpx", "gx")):
        bad, good = run(torch, op, net)[name], run(torch, op, net, x=clean)[name]
        assert np.isnan(bad[23]).all() and np.isfinite(good).all()
        assert np.array_equal(_bits(np.delete(bad, 23, 0)), _bits(np.delete(good, 23, 0))), op


def test_b_0(gpu):
    """The forward and the x-VJP write nothing; the VJP, with NULL x / gout / workspace, writes exact zeros into all four leaves."""
    torch = gpu
    case = fu.Case(fu.BY_TAG["d2_o2_n33"])
    net = Net(torch, case)
    x0, g0 = np.zeros((0, case.D)), np.zeros((0, case.O))
    assert run(torch, "fwd", net, x=x0, g=g0)["out"].shape == (0, case.O)
    assert run(torch, "vjpx", net, x=x0, g=g0)["gx"].shape == (0, case.D)
    got = run(torch, "vjp", net, x=x0, g=g0, null=("x", "gout", "ws"))
    assert all((got[n] == 0).all() and not np.signbit(got[n]).any() for n in fu.LEAVES)
    full = run(torch, "fwd", net, B=0)                    # B = 0 with real buffers: still nothing written
    assert np.isnan(full["out"]).all()
    full = run(torch, "vjpx", net, B=0)
    assert np.isnan(full["gx"]).all()


# ------------------------------------------------------------------------------------------------ refusals
def test_vjp_refuses_17_outputs_and_the_other_two_do_not(gpu):
    torch = gpu
    case = fu.Case(fu.BY_TAG["d6_o17_n130"])
    net = Net(torch, case)
    assert run(torch, "vjp", net, expect=UNSUPPORTED) is None
    check(case, "fwd", run(torch, "fwd", net))
    check(case, "vjpx", run(torch, "vjpx", net))
    with pytest.raises(ValueError, match="out_features <= 16"):
        net.wc.vjp64(case.params, case.x, case.g)


def test_lds_limit_of_the_gate_table(gpu):
    """128 entries are exactly 64 KiB and run (forward and VJP, within the bound); 129 are refused by both with nothing written;
    the x-VJP has no such table."""
    torch = gpu
    at, over = fu.Case(fu.BY_TAG["lds_128"]), fu.Case(fu.BY_TAG["lds_129"])
    assert fu.gate_lds_bytes(*at.tables()[:2]) == fu.F64_LDS_LIMIT and fu.gate_lds_bytes(*over.tables()[:2]) == fu.F64_LDS_LIMIT + 512
    net = Net(torch, at)
    assert (net.card.nsplit, net.card.max_ranges) == (8, 16)
    for op in fu.OPS:
        run_case(torch, "lds_128", op, net)
    net = Net(torch, over)
    assert (net.card.nsplit, net.card.max_ranges) == (3, 43)
    assert run(torch, "fwd", net, expect=UNSUPPORTED) is None and run(torch, "vjp", net, expect=UNSUPPORTED) is None
    run_case(torch, "lds_129", "vjpx", net)


@pytest.mark.parametrize("op", ["fwd", "vjp"])              # irbfn_f64_vjp_x takes no workspace
def test_a_workspace_one_byte_short_is_refused(gpu, op):
    torch = gpu
    for tag in ("d2_o2_n33", "r65"):
        net = Net(torch, fu.Case(fu.BY_TAG[tag]))
        assert run(torch, op, net, short=1, expect=BAD_ARG) is None
        assert run(torch, op, net) is not None


BAD_CARDS = [("D", 0), ("D", 9), ("R", 0), ("K", 0), ("O", 0), ("nsplit", 9), ("nsplit", 3), ("basis", -1), ("basis", 13),
             ("max_ranges", 0), ("lo_dev", None), ("hi_dev", None), ("delta_dev", None), ("dim_ranges_dev", None), ("n_ranges", -1)]


@pytest.mark.parametrize("field,value", BAD_CARDS, ids=[f"{f}={v}" for f, v in BAD_CARDS])
def test_bad_cards_are_refused_before_any_launch(gpu, field, value):
    torch = gpu
    lib = _lib.load()
    case = fu.Case(fu.BY_TAG["d2_o2_n33"])                                     # D = 2, nsplit = 1: nsplit = 3 exceeds D
    good, keep = hand_card(torch, case)
    assert good.n_ranges == 1 and good.nsplit == 1 and good.D == 2
    for op in fu.OPS:
        assert run(torch, op, Net(torch, case, good)) is not None
    card, _ = hand_card(torch, case, **{field: value})
    assert getattr(card, field) == value
    for with_vjp in (0, 1):
        assert lib.irbfn_f64_workspace_bytes(C.byref(card), case.B, with_vjp) == BAD_ARG
    net = Net(torch, case, card)
    for op in fu.OPS:
        assert run(torch, op, net, expect=BAD_ARG) is None
        assert run(torch, op, net, B=0, expect=BAD_ARG) is None


def test_null_card_negative_batch_and_null_pointers_are_refused(gpu):
    torch = gpu
    lib = _lib.load()
    case = fu.Case(fu.BY_TAG["d2_o2_n33"])
    net = Net(torch, case)
    for with_vjp in (0, 1):
        assert lib.irbfn_f64_workspace_bytes(None, case.B, with_vjp) == BAD_ARG
        assert lib.irbfn_f64_workspace_bytes(C.byref(net.card), -1, with_vjp) == BAD_ARG
    for op in fu.OPS:
        assert run(torch, op, net, B=-1, expect=BAD_ARG) is None
        for name in (n for n in POINTERS[op] if (op, n) != ("vjpx", "ws")):      # the x-VJP takes no workspace: NULL is fine there
            assert run(torch, op, net, null=(name,), expect=BAD_ARG) is None, (op, name)
        assert run(torch, op, net) is not None


# ------------------------------------------------------------------------------------------------ through the class
def test_through_the_class(gpu):
    """A cuda tensor in gives cuda float64 out; vjp64(out=...) writes into the given leaves; a small batch after a large one on one
    net (the cached workspace) gives the bits of a fresh net."""
    torch = gpu
    case = fu.Case(fu.BY_TAG["b65"])
    big = fu.Case(fu.BY_TAG["b600"])
    used, fresh = WCRBFNet.from_config(case.cfg, use_float64=True), WCRBFNet.from_config(case.cfg, use_float64=True)
    xd, gd = torch.from_numpy(case.x).cuda(), torch.from_numpy(case.g).cuda()
    out = used.apply(case.params, xd)
    assert out.is_cuda and out.dtype == torch.float64 and tuple(out.shape) == (case.B, case.O)
    gx = used.vjp_x(case.params, xd, gd)
    assert gx.is_cuda and gx.dtype == torch.float64
    shapes = {"centers": (case.R, case.K, case.D), "log_sigs": (case.R, case.K), "kernel": (case.K, case.O), "bias": (case.O,)}

    def leaves():
        t = {n: torch.full(s, float("nan"), dtype=torch.float64, device="cuda") for n, s in shapes.items()}
        return t, {"params": {"rbf_list": {"centers": t["centers"], "log_sigs": t["log_sigs"]},
                              "linear": {"kernel": t["kernel"], "bias": t["bias"]}}}

    used.vjp64(big.params, torch.from_numpy(big.x).cuda(), torch.from_numpy(big.g).cuda())           # 10 slices, then 2
    ta, tree = leaves()
    ret = used.vjp64(case.params, xd, gd, out=tree)
    tb, tree_b = leaves()
    fresh.vjp64(case.params, xd, gd, out=tree_b)
    torch.cuda.synchronize()
    assert ret["params"]["rbf_list"]["centers"].data_ptr() == ta["centers"].data_ptr()
    got = {n: ta[n].cpu().numpy() for n in shapes}
    for n in shapes:
        assert np.array_equal(_bits(got[n]), _bits(tb[n].cpu().numpy())), n
    check(case, "vjp", got)
    check(case, "fwd", {"out": out.cpu().numpy()})
    check(case, "vjpx", {"gx": gx.cpu().numpy()})
    assert np.array_equal(_bits(fresh.apply(case.params, case.x)), _bits(out.cpu().numpy()))
