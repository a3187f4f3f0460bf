"""The chunked float64 reference, the float32 yardstick, the restated launch rules and the cases of tests/_k2m_util.py, without a
GPU: the centre chunks against the unchunked k2.vjp_reference / k2.vjp_float32 bit for bit and against torch.autograd of the
oracle, k2m_plan against rows worked out by hand, what TABLE claims to cover, the gates' preconditions (a gamma that is really
between 0 and 1, really read from the second range column, really an exact float32 zero), the non-finite cases' references, and
R32M -- the worst error of the plain float32 restatement over the whole table, which fixes the coefficient of the element-wise
bound of tests/test_gpu_k2m.py."""
import itertools

import numpy as np
import pytest

import _k2_util as k2
import _k2m_util as km
from test_k2_reference_cpu import _autograd

INPUTS = "test inputs, not the code under test: "


@pytest.mark.parametrize("tag", ["m_d5_o17_n33_gaussian_wider", "m_gate_column_ns3"])
def test_centre_chunks_change_no_bit(tag):
    """Seven centres a chunk (several chunks and a ragged last one) against the whole net in one piece: every sum runs over the
    queries of one centre, so no bit of any leaf may move, in float64 or in float32."""
    case = km.CaseM(km.BY_TAG[tag])
    assert case.K > 14 and case.K % 7
    ref, whole = km.reference(case, chunk=7), k2.vjp_reference(case.basis, case.params, case.x, case.g, case.gamma())
    yard, plain = km.yardstick(case, chunk=7), k2.vjp_float32(case.basis, case.params, case.x, case.g, case.gamma(np.float32))
    auto = _autograd(case)
    for leaf in k2.LEAVES:
        grad, S = ref[leaf]
        assert grad.dtype == np.float64 and grad.shape == S.shape == whole[leaf][0].shape
        assert np.array_equal(grad, whole[leaf][0]) and np.array_equal(S, whole[leaf][1]), (tag, leaf)
        assert yard[leaf].dtype == np.float32 and np.array_equal(yard[leaf], plain[leaf]), (tag, leaf)
        assert (S >= np.abs(grad)).all() and (np.abs(grad - auto[leaf]) <= 1e-11 * S).all(), (tag, leaf)
    default = case.reference()                                               # the chunk a test runs with
    assert all(np.array_equal(default[leaf][0], whole[leaf][0]) for leaf in k2.LEAVES)


# ------------------------------------------------------------------------------------------------ the launch rules
HAND = [  # N, B, O -> groups, S, tiles per wave, idle waves
    (1, 1, 17, 1, 1, 1, [1, 2, 3]), (33, 17, 32, 2, 1, 1, [2, 3]), (65, 257, 33, 3, 2, 3, [6, 7]), (100, 513, 64, 4, 3, 3, [11]),
    (17, 1021, 65, 2, 4, 4, []), (40, 70, 100, 3, 1, 2, [3]), (4096, 4096, 64, 128, 4, 16, []),
]


@pytest.mark.parametrize("N,B,O,groups,S,tpw,idle", HAND)
def test_k2m_plan_by_hand(N, B, O, groups, S, tpw, idle):
    p = km.k2m_plan(N, B, 5, O, "inverse_quadratic")
    assert (p["groups"], p["S"], p["tiles_per_wave"], p["idle_waves"]) == (groups, S, tpw, idle)
    OW = 32 if O <= 32 else 64 if O <= 64 else 128
    assert (p["OW"], p["CT"], p["grid"], p["block"], p["ntiles"]) == (OW, 2 if OW <= 64 else 1, groups * S, 256, -(-B // 16))
    assert p["name"] == f"rbf_vjp_mfma<D=7,OW={OW},BC=1,CT={p['CT']},QSB={S}>"
    assert 4 * S * tpw >= p["ntiles"] > (4 * S - len(idle) - 1) * tpw


def test_k2m_plan_slab_cap_and_paddings():
    case = km.CaseM(km.BY_TAG["m_slab_cap"])
    p = case.plan()
    assert (case.N, case.B, case.O, case.D) == (1000, 2305, 100, 8)
    assert (p["groups"], p["by_groups"], p["by_batch"], p["QSB"], p["S"]) == (63, 9, 10, 10, 9)      # ceil(512 / 63) caps, not the batch
    assert (p["ntiles"], p["tiles_per_wave"], p["idle_waves"]) == (145, 5, list(range(29, 36)))      # the ninth slab: waves 32 .. 35
    assert (p["OW"], p["OP"], p["grid"], p["name"]) == (128, 100, 567, "rbf_vjp_mfma<D=8,OW=128,BC=0,CT=1,QSB=9>")
    assert [km.k2m_plan(9, 70, D, 20, "gaussian")["DC"] for D in range(1, 9)] == [3, 3, 3, 4, 7, 7, 7, 8]
    assert [km.k2m_plan(9, 70, 3, O, "gaussian")["OW"] for O in (17, 32, 33, 64, 65, 100, 101, 128)] == [32, 32, 64, 64] + [128] * 4
    assert [km.k2m_plan(9, 70, 3, O, "gaussian")["OP"] for O in (17, 32, 33, 64, 65, 100, 101, 128)] == [32, 32, 64, 64, 100, 100, 128, 128]
    assert km.k2m_plan(4096, 80000, 8, 64, "gaussian")["S"] == 4 and km.k2m_plan(100, 80000, 8, 64, "gaussian")["S"] == 128
    # K2's layout caps: 6400 centres are 100 groups of 64, ceil(8192 / 400) = 21 slabs allocated
    assert (km.k2m_plan(6400, 80000, 8, 128, "gaussian")["QSB"], km.k2m_plan(6400, 80000, 8, 128, "gaussian")["S"]) == (21, 2)


# ------------------------------------------------------------------------------------------------ what the table covers
def test_table_covers_what_it_claims():
    S = km.SHAPES
    assert {s["D"] for s in S} == set(range(1, 9)) and {s["O"] for s in S} == {17, 32, 33, 64, 65, 100, 101, 128}
    assert {s["basis"] for s in S} == set(k2.FAST)
    for wide in ("gaussian_wide", "gaussian_wider"):
        assert len({km.vjpm_ow(s["O"]) for s in S if s["basis"] == wide}) >= 2
    for CW, ks in km.K_AROUND.items():
        assert {s["K"] for s in S if 16 * km.vjpm_ct(km.vjpm_ow(s["O"])) == CW} == set(ks), CW
    # every instance launch_vjp_mfma dispatches to: 4 padded D x 3 OW x 3 basis classes
    inst = {(k2.padded_D(s["D"]), km.vjpm_ow(s["O"]), k2.bclass(s["basis"])) for s in km.TABLE}
    assert inst == set(itertools.product((3, 4, 7, 8), (32, 64, 128), (0, 1, 2))) and len(inst) == 36
    assert any(s["ns"] == 0 for s in S) and any(0 < s["ns"] < s["D"] for s in S) and any(s["ns"] == s["D"] for s in S)
    assert all(s["gate"] == "mid" for s in S + km.BATCH + km.SLAB_CAP + km.REUSE + km.NONFINITE + km.ON_CENTRES)
    assert [(s["gate"], s["ns"]) for s in km.GATES] == [("column", 1), ("column", 3), ("sharp", 1), ("none", 1)]
    assert tuple(s["B"] for s in km.BATCH) == (1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 513, 1021) and len({s["net"] for s in km.BATCH}) == 1
    assert all(16 < s["O"] <= 128 and s["basis"] in k2.FAST and s["kind"] == "one" for s in km.TABLE)
    assert all(s["B"] * s["K"] * s["O"] <= 2.5e8 for s in km.TABLE)
    assert {s["poison"] for s in km.NONFINITE} == {"nan_g", "nan_x", "inf_g", "nan_xg"}
    assert all(s["O"] % 4 and s["B"] % 16 and s["ns"] < 4 for s in km.NONFINITE)     # x[23, 3] is ungated, x[23, 0] gated
    assert {s["basis"] for s in km.ON_CENTRES} == set(k2.FAST)
    batch = [km.CaseM(s) for s in km.BATCH]
    assert all(np.array_equal(c.x, batch[-1].x[:c.B]) and np.array_equal(c.g, batch[-1].g[:c.B]) for c in batch)
    assert all(np.array_equal(c.params["params"]["linear"]["kernel"], batch[-1].params["params"]["linear"]["kernel"]) for c in batch)


# ------------------------------------------------------------------------------------------------ the gates
def _drawn(spec):
    """The case on its net's whole drawn batch, unpoisoned: the batch rows take its first B queries."""
    return km.CaseM(dict(spec, B=spec.get("draw", spec["B"]), poison=None))


def test_gates_are_what_the_cases_are_about():
    for spec in km.TABLE:
        case = _drawn(spec)
        gam, gam32 = case.gamma()[:, 0], case.gamma(np.float32)[:, 0]
        assert case.cfg["dimension_ranges"] == ([] if case.gate == "none" else [case.cols]) and len(case.cfg["delta"]) == case.ns
        if case.gate == "none":
            if not ((gam == 0).all() and (gam32 == 0).all()):
                pytest.fail(INPUTS + f"{case.tag}: a card without a range row has a weight")
        elif case.ns == 0:
            if not ((gam == 1).all() and (gam32 == 1).all()):
                pytest.fail(INPUTS + f"{case.tag}: no gated coordinate, yet gamma is not 1")
        elif case.gate in ("mid", "column"):
            if not (gam.min() < 0.1 and gam.max() > 0.5 and (gam32 > 0).all()):
                pytest.fail(INPUTS + f"{case.tag}: gamma in [{gam.min():.3g}, {gam.max():.3g}] does not exercise the gate")
        if case.gate == "column":
            other = case.gamma_other_column()[:, 0]
            if not (case.cfg["dimension_ranges"][0].count(1) >= 1 and np.abs(other - gam).max() > 0.1):
                pytest.fail(INPUTS + f"{case.tag}: the other range column gives the same gamma")
            zero = km.tanh_gate(dict(case.cfg, dimension_ranges=[[0] * case.ns]), case.x)[:, 0]
            if not np.abs(zero - gam).max() > 0.1:
                pytest.fail(INPUTS + f"{case.tag}: range column 0 gives the same gamma")
        if case.gate == "sharp":
            if not (((gam32 == 0) & (gam > 0)).sum() >= 8 and (gam > 0.5).sum() >= 8):
                pytest.fail(INPUTS + f"{case.tag}: no query with an exact float32 zero beside a float64 weight, or none inside the box")
    cols = km.CaseM(km.BY_TAG["m_gate_column_ns3"])
    assert cols.cols == [1, 0, 1] and cols.cfg["lower_bounds"] == [[-9.0, 0.0], [0.0, -9.0], [-9.0, 0.0]]
    assert cols.cfg["upper_bounds"] == [[9.0, 0.8], [0.8, 9.0], [9.0, 0.8]]
    mid = km.CaseM(km.BY_TAG["m_d2_o32_n15_inverse_quadratic"])
    assert mid.cfg["lower_bounds"] == [[0.0]] * 2 and mid.cfg["upper_bounds"] == [[0.8]] * 2 and mid.cfg["delta"] == [3.0] * 2
    # one factor of the mid gate over the queries' range
    f = km.tanh_gate(dict(mid.cfg, activation_idx=[0], lower_bounds=[[0.0]], upper_bounds=[[0.8]], delta=[3.0], dimension_ranges=[[0]]),
                     np.linspace(-0.9, 1.5, 2401)[:, None])
    assert 0.0044 < f.min() < 0.0046 and 0.83 < f.max() < 0.85


def test_a_gate_change_leaves_the_draw_alone():
    for tag in ("m_d8_o32_n65_gaussian", "m_gate_column_ns3", "m_gate_sharp", "m_gate_none"):
        mine, plain = km.CaseM(km.BY_TAG[tag]), k2.Case(km.BY_TAG[tag])
        assert np.array_equal(mine.x, plain.x) and np.array_equal(mine.g, plain.g)
        for a, b in k2.LEAF_PATH.values():
            assert np.array_equal(mine.params["params"][a][b], plain.params["params"][a][b])


def test_the_ungated_card_weighs_nothing():
    ref = km.CaseM(km.BY_TAG["m_gate_none"]).reference()
    assert all((ref[leaf][0] == 0).all() and (ref[leaf][1] == 0).all() for leaf in ("centers", "log_sigs", "kernel"))
    assert (ref["bias"][0] != 0).all()


# ------------------------------------------------------------------------------------------------ the non-finite cases
@pytest.mark.parametrize("tag", [s["tag"] for s in km.NONFINITE])
def test_non_finite_references(tag):
    """The NaN and Inf of the float64 reference where tests/test_gpu_k2m.py asserts them, and the same ones in plain float32: no
    Inf of the reference stands on a factor that float32 would flush to 0 (0 x Inf = NaN there)."""
    case = km.CaseM(km.BY_TAG[tag])
    ref, yard = case.reference(), case.yardstick()
    g = {leaf: ref[leaf][0] for leaf in k2.LEAVES}
    assert all(k2.same_nonfinite(yard[leaf], g[leaf]) for leaf in k2.LEAVES)
    poison = case.spec["poison"]
    if poison == "nan_g":
        others = [o for o in range(case.O) if o != 1]
        assert np.isnan(case.g[17, 1]) and np.isnan(g["kernel"][:, 1]).all() and np.isnan(g["bias"][1])
        assert np.isfinite(g["kernel"][:, others]).all() and np.isfinite(g["bias"][others]).all()
        assert np.isnan(g["centers"]).all() and np.isnan(g["log_sigs"]).all()
    elif poison in ("nan_x", "nan_xg"):
        col = 3 if poison == "nan_x" else 0
        assert np.isnan(case.x[23, col]) and (col >= case.ns) == (poison == "nan_x")
        assert np.isnan(case.gamma()[23, 0]) == (poison == "nan_xg")
        assert np.isnan(g["centers"]).all() and np.isnan(g["log_sigs"]).all() and np.isnan(g["kernel"]).all()
        assert np.isfinite(g["bias"]).all()
    else:
        others = [o for o in range(case.O) if o != 2]
        assert case.g[40, 2] == np.inf and (g["kernel"][:, 2] == np.inf).all() and g["bias"][2] == np.inf
        assert np.isfinite(g["kernel"][:, others]).all() and np.isfinite(g["bias"][others]).all()
        assert np.isinf(g["centers"]).all() and np.isinf(g["log_sigs"]).all()
        # query 40 in float32: gamma, phi and the slope all far above the smallest normal number
        c, ls = case.params["params"]["rbf_list"]["centers"][0], case.params["params"]["rbf_list"]["log_sigs"][0]
        d2 = ((case.x[40][None] - c) ** 2).sum(-1, dtype=np.float32) * np.exp(-2 * ls)
        phi = k2.basis_and_slope(case.basis, d2)[0]
        assert phi.dtype == np.float32 and (case.gamma(np.float32)[40, 0] * phi * d2 > 2.0 ** -60).all()


def test_queries_on_centres_are_on_centres():
    for spec in km.ON_CENTRES:
        case = km.CaseM(spec)
        cc = case.params["params"]["rbf_list"]["centers"]
        assert all((case.x[b] == cc[0, k]).all() for b, k in ((5, 3), (20, 17), (case.B - 1, case.K - 1)))
        assert all(np.isfinite(v[0]).all() for v in case.reference().values())


# ------------------------------------------------------------------------------------------------ the coefficient
def test_yardstick_and_the_coefficient():
    """r32, the worst |err| / S of the plain float32 restatement over every case of the table, printed per case and leaf.  A case
    that needs more than 5e-5 S in plain float32 has the wrong inputs for its purpose."""
    r32, at = 0.0, None
    for spec in km.TABLE:
        case = km.CaseM(spec)
        ref, y = case.reference(), case.yardstick()
        line = []
        for leaf in k2.LEAVES:
            assert k2.same_nonfinite(y[leaf], ref[leaf][0]), (case.tag, leaf)
            es, _ = km.ratios_m(y[leaf], *ref[leaf])
            if es > 5e-5:
                pytest.fail(INPUTS + f"{case.tag} {leaf} needs {es:.2e} S in plain float32")
            line.append(f"{leaf} {es:.2e}")
            if es > r32:
                r32, at = es, (case.tag, leaf)
        print(f"{case.tag:36s} " + "  ".join(line))
    print(f"r32 = {r32:.3e} at {at}; R32M = {km.R32M:.3e}, C_M = {km.C_M:.3e}")
    assert km.R32M / 2 < r32 <= km.R32M, "R32M in _k2m_util.py is not what the yardstick gives"
    assert km.C_M == 4 * km.R32M and km.C_M <= 5e-5
