"""The np.longdouble statement, the float64 yardstick and the restated launch rules of tests/_f64_util.py, without a GPU: the
statement against the project's independent float64 oracle and torch.autograd of it under the element-wise bound the kernels are
held to (tests/test_gpu_f64_kernels.py), the yardstick's worst error over the whole table (which fixes the bound's coefficient), the
launch rules against values worked out by hand, and the conditions on the inputs that the cases are about."""
import numpy as np
import pytest

import _f64_util as fu
import _vjpx_util as vx
from oracle import irbfn_oracle as orc

D2_ONLY = ("gaussian", "gaussian_wide", "gaussian_wider", "inverse_quadratic", "inverse_multiquadric", "multiquadric", "quadratic")
INPUTS = "test inputs, not the code under test: "


def oracle_cfg(case):
    """The oracle has no card without split coordinates: a box on coordinate 0 that no query is near gives it gamma = 1 exactly."""
    if case.ns:
        return case.cfg
    return dict(case.cfg, activation_idx=[0], lower_bounds=[[-1e6]], upper_bounds=[[1e6]], delta=[1.0],
                dimension_ranges=[[0]] * len(case.cfg["dimension_ranges"]))


def _autograd(case):
    import torch
    p = orc.torch_params(case.params, requires_grad=True)
    out = orc.wcrbfnet_apply(oracle_cfg(case), p, torch.tensor(case.x, dtype=torch.float64))
    (out * torch.tensor(case.g, dtype=torch.float64)).sum().backward()
    return {n: p["params"][a][b].grad.numpy() for n, (a, b) in fu.LEAF_PATH.items()}


def _hold(case, what, got, ref, S, Sg, rows=None):
    """`got`, a float64 evaluation, meets the kernels' bound against the statement; its non-finite elements are the statement's."""
    if rows is not None:
        got, ref, S, Sg = got[rows], ref[rows], S[rows], Sg[rows]
    assert got.dtype == np.float64 and ref.dtype == fu.LD and got.shape == ref.shape
    assert fu.same_nonfinite(got, np.asarray(ref, np.float64)), (case.tag, what)
    fin = np.isfinite(ref)
    assert (S[fin] >= np.abs(ref[fin]) * (1 - 1e-15)).all(), (case.tag, what)
    worst = fu.ratio(got, ref, S, Sg)
    assert worst <= 1.0, (case.tag, what, worst)
    return worst


@pytest.mark.parametrize("tag", [s["tag"] for s in fu.TABLE if s["B"] <= 600])
def test_statement_agrees_with_the_oracle_and_autograd(tag):
    case = fu.Case(fu.BY_TAG[tag])
    cfg, line = oracle_cfg(case), []
    on_rows = [b for b, _ in case.on]
    if "fwd" in case.ops:
        line.append(("fwd", _hold(case, "fwd", orc.wcrbfnet_apply(cfg, case.params, case.x), *fu.reference(case, "fwd")["out"])))
    if "vjp" in case.ops:
        ref = fu.reference(case, "vjp")
        others = {}
        if case.on and case.basis in D2_ONLY:        # autograd differentiates sqrt at 0: NaN for a query on a centre, whatever the basis
            hand = orc.wcrbfnet_vjp(cfg, case.params, case.x, case.g)["params"]
            others["wcrbfnet_vjp"] = {n: hand[a][b] for n, (a, b) in fu.LEAF_PATH.items()}
        else:
            others["autograd"] = _autograd(case)
        for name, other in others.items():
            line.append((name, max(_hold(case, f"{name} {leaf}", other[leaf], *ref[leaf]) for leaf in fu.LEAVES)))
    if "vjpx" in case.ops:
        gx = vx.ref_gx(cfg, case.params, case.x, case.g)
        keep = np.ones(case.B, bool)
        keep[on_rows] = False                         # ref_gx goes through sqrt: NaN on a centre, where the statement has the kernels' finite convention
        assert np.isnan(gx[on_rows]).all()
        assert np.isfinite(np.asarray(fu.reference(case, "vjpx")["gx"][0], np.float64)[on_rows]).all()
        line.append(("ref_gx", _hold(case, "ref_gx", gx, *fu.reference(case, "vjpx")["gx"], rows=keep)))
    print(f"{tag:32s} " + "  ".join(f"{n} {w:.3f}" for n, w in line))


def test_yardstick_and_the_coefficient():
    """r64, the worst max(|y - ref| - S_gamma, 0) / (2^-53 S) of the float64 restatement over every case and operation of the table,
    printed per case with the name that sets it."""
    r64, who = 0.0, None
    for spec in fu.TABLE:
        case = fu.Case(spec)
        line = []
        for op in case.ops:
            ref, y = fu.reference(case, op), fu.yardstick(case, op)
            for name, (r, S, Sg) in ref.items():
                assert fu.same_nonfinite(y[name], np.asarray(r, np.float64)), (case.tag, op, name)
                need = fu.needed(y[name], r, S, Sg)
                line.append(f"{op}.{name} {need:.2f}")
                if need > r64:
                    r64, who = need, (case.tag, op, name)
        print(f"{case.tag:32s} " + "  ".join(line))
    print(f"r64 = {r64:.3f} set by {who}; R64 = {fu.R64}, C64 = {fu.C64}")
    assert r64 <= fu.R64 <= 1.5 * r64, "R64 in _f64_util.py is not what the yardstick gives"
    assert fu.C64 == 4 * fu.R64


def test_the_gate_term_of_the_bound_matters():
    """Without S_gamma the same yardstick is far outside C64 2^-53 S on the regions that weigh 1e-7 and less."""
    case = fu.Case(fu.BY_TAG["r6_tiny"])
    ref, y = fu.reference(case, "vjp"), fu.yardstick(case, "vjp")
    r, S, Sg = ref["centers"]
    assert fu.needed(y["centers"], r, S, 0 * Sg) > 1e3 * fu.C64 and fu.ratio(y["centers"], r, S, Sg) <= 1.0


HAND = [  # N, B, D, R, O -> slices, per_slice, Npad, empty, bytes_fwd, bytes_vjp
    (1, 1, 1, 1, 1, 1, 1, 64, 0, 256, 256 + 3 * 64 * 8),
    (3, 0, 3, 1, 2, 1, 0, 64, 1, 0, 6 * 64 * 8),
    (63, 65, 8, 1, 1, 2, 33, 64, 0, 768, 768 + 2 * 10 * 64 * 8),
    (64, 64, 3, 1, 5, 1, 64, 64, 0, 512, 512 + 9 * 64 * 8),
    (65, 129, 4, 1, 16, 3, 43, 128, 0, 1280, 1280 + 3 * 21 * 128 * 8),
    (130, 600, 7, 65, 10, 10, 60, 192, 0, 312064, 312064 + 10 * 18 * 192 * 8),
    (3, 65536, 3, 1, 2, 1024, 64, 64, 0, 524288, 524288 + 1024 * 6 * 64 * 8),
    (3, 65537, 3, 1, 2, 1024, 65, 64, 15, 524544, 524544 + 1024 * 6 * 64 * 8),
    (3, 66000, 3, 1, 2, 1024, 65, 64, 8, 528128, 528128 + 1024 * 6 * 64 * 8),
    (449, 600, 3, 1, 2, 10, 60, 512, 0, 4864, 4864 + 10 * 6 * 512 * 8),
    (449, 80000, 3, 1, 2, 512, 157, 512, 2, 640000, 640000 + 512 * 6 * 512 * 8),
]


@pytest.mark.parametrize("N,B,D,R,O,slices,per_slice,Npad,empty,bytes_fwd,bytes_vjp", HAND)
def test_launch_rules_by_hand(N, B, D, R, O, slices, per_slice, Npad, empty, bytes_fwd, bytes_vjp):
    p = fu.f64_plan(N, B, D, R, O)
    assert (p["slices"], p["per_slice"], p["Npad"], p["empty"], p["bytes_fwd"], p["bytes_vjp"]) == \
        (slices, per_slice, Npad, empty, bytes_fwd, bytes_vjp)


def test_slice_cases_are_at_the_caps():
    plans = {tag: fu.Case(fu.BY_TAG[tag]).plan() for tag in fu.tags("vjp", fu.SLICES)}
    assert [(p["slices"], p["per_slice"], p["empty"]) for p in plans.values()] == \
        [(1024, 64, 0), (1024, 65, 15), (1024, 65, 8), (10, 60, 0)], INPUTS + str(plans)
    assert fu.gate_lds_bytes(8, 16) == fu.F64_LDS_LIMIT and fu.gate_lds_bytes(3, 43) == fu.F64_LDS_LIMIT + 512
    for tag, (ns, mr) in (("lds_128", (8, 16)), ("lds_129", (3, 43))):
        assert fu.Case(fu.BY_TAG[tag]).tables()[:2] == (ns, mr), INPUTS + tag


def test_table_covers_the_shapes_the_issue_names():
    specs = {op: [s for s in fu.TABLE if op in s["ops"]] for op in fu.OPS}
    for op, want in (("fwd", {1, 2, 15, 16, 17, 32, 33}), ("vjp", {1, 2, 5, 15, 16}), ("vjpx", {1, 16, 17, 33})):
        assert want <= {s["O"] for s in specs[op]}, INPUTS + op
        assert {s["basis"] for s in specs[op]} == set(fu.BASES), INPUTS + op
        assert {s["D"] for s in specs[op]} == set(range(1, 9)), INPUTS + op
    cases = [fu.Case(s) for s in specs["vjp"] if s["B"] <= 600]
    assert {1, 33, 63, 64, 65, 130} <= {c.N for c in cases}
    assert {2, 63, 64, 65} <= {c.R for c in cases if c.kind == "regions"}
    assert {(c.ns == 0, c.R) for c in cases if c.ns == 0} == {(True, 1), (True, 2)}
    assert any(0 < c.ns < c.D for c in cases) and any(c.ns == c.D for c in cases)
    assert max(s["O"] for s in specs["vjp"]) == fu.F64_OT


def test_gate_cases_are_what_they_say():
    """The steep net's half-factors fill the three bands, one region and two queries are exactly 0 in float64; r6_tiny's regions
    weigh 1e-7 and less next to one that weighs 1; fewer rows than regions give exact zeros; more rows than regions are dropped."""
    steep = fu.Case(fu.BY_TAG["steep"])
    z = steep.half_z()
    for lo, hi, what in ((-18.0, -9.1, "where float32's gate is 0 and float64's is not"), (-np.inf, -20.0, "where float64's tanh is -1"),
                         (-0.5, 0.5, "near 0")):
        if not ((z > lo) & (z < hi)).sum() >= 10:
            pytest.fail(INPUTS + f"the steep gate has no half-factor {what}")
    assert (np.tanh(z[z < -20.0]) == -1.0).all() and ((np.tanh(z[(z > -18.0) & (z < -9.1)]) + 1) / 2 > 0).all()
    g64, _, _, _ = fu.gate(steep, np.float64, tanh_form=True)
    gld, dg, _, _ = fu.gate(steep)
    if not ((g64[:, 3] == 0).all() and (g64[[7, 11]] == 0).all() and (gld[:, :3].max(0) > 0.9).all() and (gld > 0).all()):
        pytest.fail(INPUTS + "the steep gate's exact zeros are not where the case wants them")
    assert (np.abs(g64 - gld) <= dg).all()                     # the float64 tanh form is within delta gamma of the statement's gate
    tiny = fu.Case(fu.BY_TAG["r6_tiny"])
    gam = np.asarray(fu.gate(tiny)[0], np.float64)
    if not ((gam[:, 0] > 0.99).all() and (gam[:, 1:] < 1e-6).all() and (gam[:, 1:] > 0).all() and gam[:, 1:].min() < 1e-13):
        pytest.fail(INPUTS + "r6_tiny's weights are not what the case is about")
    S = fu.reference(tiny, "vjp")["centers"][1]
    assert S[1:].max() < 1e-5 * S[0].max()                      # elements a bound relative to the largest element cannot see
    rows4, rows6 = fu.Case(fu.BY_TAG["r6_rows4"]), fu.Case(fu.BY_TAG["r4_rows6"])
    g4 = fu.gate(rows4)[0]
    assert (g4[:, 4:] == 0).all() and (g4[:, :4].max(0) > 0.5).all() and rows4.tables()[6] == 4 < rows4.R
    assert rows6.tables()[6] == 4 and rows6.tables(n_ranges=6)[5].shape == (6, 2) and rows6.R == 4
    ns, mr, lo, hi, _, _, _ = rows4.tables(pad=np.nan)          # 3 and 2 ranges: one padding entry per table
    assert (ns, mr) == (2, 3) and np.isnan(lo).sum() == 1 and np.isnan(hi).sum() == 1 and np.isnan(lo[1, 2])
    small = fu.Case(fu.BY_TAG["d3_o17_small_column"])
    out, S, _ = fu.reference(small, "fwd")["out"]
    W = small.params["params"]["linear"]["kernel"]
    assert np.abs(W[:, 16]).max() < 1e-8 and np.abs(W[:, :16]).min(1).max() > 1e-3


def test_non_finite_and_on_centre_cases_are_what_they_say():
    for tag in fu.tags("vjp", fu.NONFINITE):
        case = fu.Case(fu.BY_TAG[tag])
        bad_x, bad_g = ~np.isfinite(case.x), ~np.isfinite(case.g)
        want = {"nan_x": (1, 0), "nan_g": (0, 1), "inf_g": (0, 1)}[case.spec["poison"]]
        if (bad_x.sum(), bad_g.sum()) != want or (bad_x.any() and not bad_x[23, 3]) or case.ns > 3:
            pytest.fail(INPUTS + f"{tag}: the non-finite element is not where the case wants it")
        gx = np.asarray(fu.reference(case, "vjpx")["gx"][0], np.float64)
        row = {"nan_x": 23, "nan_g": 17, "inf_g": 40}[case.spec["poison"]]
        assert not np.isfinite(gx[row]).any() and np.isfinite(np.delete(gx, row, 0)).all(), tag
        ref = fu.reference(case, "vjp")
        if case.spec["poison"] == "nan_x":
            assert all(np.isnan(ref[n][0]).all() for n in ("centers", "log_sigs", "kernel")) and np.isfinite(ref["bias"][0]).all()
            out = np.asarray(fu.reference(case, "fwd")["out"][0], np.float64)
            assert np.isnan(out[23]).all() and np.isfinite(np.delete(out, 23, 0)).all()
        elif case.spec["poison"] == "nan_g":
            assert np.isnan(ref["kernel"][0][:, 1]).all() and np.isfinite(np.delete(ref["kernel"][0], 1, 1)).all()
        else:
            assert (ref["kernel"][0][:, 2] == np.inf).all() and ref["bias"][0][2] == np.inf and np.isinf(ref["centers"][0]).all()
    for tag in fu.tags("vjp", fu.ON_CENTRES + fu.ON_CENTRES_D):
        case = fu.Case(fu.BY_TAG[tag])
        cc = case.params["params"]["rbf_list"]["centers"]
        if not (len(case.on) == 3 and all((case.x[b] == cc[0, k]).all() for b, k in case.on)):
            pytest.fail(INPUTS + f"{tag}: the three queries are not centres")
        ref = fu.reference(case, "vjp")
        assert np.isfinite(ref["log_sigs"][0]).all() and np.isfinite(fu.reference(case, "vjpx")["gx"][0]).all()
        assert np.isnan(ref["centers"][0]).all() if case.basis in fu.D_BASES else np.isfinite(ref["centers"][0]).all()
