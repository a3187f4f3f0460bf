"""The float64 reference, the float32 yardstick and the restated layout rules of tests/_k2_util.py, without a GPU: the reference
against the oracle's hand VJP and against torch.autograd of the oracle's forward, the yardstick's worst error over the whole table
(which fixes the coefficient of the element-wise bound of tests/test_gpu_k2.py), and the layout rules against values worked out
by hand."""
import numpy as np
import pytest

import _k2_util as k2
from oracle import irbfn_oracle as orc

BY_TAG = {s["tag"]: s for s in k2.TABLE}
D2_ONLY = ("gaussian", "gaussian_wide", "gaussian_wider", "inverse_quadratic", "inverse_multiquadric", "multiquadric", "quadratic")


def _autograd(case):
    """torch.autograd of the oracle's forward in float64: the cotangent g of `out` -> the four stage leaves."""
    import torch
    p = orc.torch_params(case.params, requires_grad=True)
    x, g = torch.tensor(case.x, dtype=torch.float64), torch.tensor(case.g, dtype=torch.float64)
    if case.cluster:
        pc = case.params["params"]["cluster"]
        p["params"]["cluster"] = {n: torch.tensor(pc[n], dtype=torch.float64) for n in ("kernel", "bias")}
        out, _ = orc.cluster_wcrbfnet_apply({"basis_func": case.basis}, p, x)
    else:
        out = orc.wcrbfnet_apply(case.cfg, p, x)
    (out * g).sum().backward()
    return {n: p["params"][a][b].grad.numpy() for n, (a, b) in k2.LEAF_PATH.items()}


@pytest.mark.parametrize("tag", ["d2_o2_n33", "d5_o5_n65", "d7_o8", "d3_o10", "wide_d7_o100", "r2", "r65", "r130", "r6_rows4", "r6_tiny",
                                 "clu_d5_o3_r7", "clu_d3_o5_r1", "b5_r4", "on_centres_inverse_quadratic"])
def test_reference_agrees_with_the_oracle_and_autograd(tag):
    case = k2.Case(BY_TAG[tag])
    ref = case.reference()
    others = {}
    # autograd differentiates sqrt at 0: NaN for a query on a centre.  r6_tiny: tanh(z) + 1 in float64 fixes a weight of 4e-8 to
    # 1e-16 / 4e-8 only, and torch's tanh and NumPy's differ in the last bit there -- the NumPy oracle alone is compared
    if not tag.startswith("on_centres") and tag != "r6_tiny":
        others["autograd"] = _autograd(case)
    if not case.cluster and case.basis in D2_ONLY:
        hand = orc.wcrbfnet_vjp(case.cfg, case.params, case.x, case.g)["params"]
        others["wcrbfnet_vjp"] = {n: hand[a][b] for n, (a, b) in k2.LEAF_PATH.items()}
    assert others
    for leaf in k2.LEAVES:
        grad, S = ref[leaf]
        assert grad.dtype == np.float64 and grad.shape == S.shape == case.params["params"][k2.LEAF_PATH[leaf][0]][k2.LEAF_PATH[leaf][1]].shape
        assert (S >= np.abs(grad)).all(), (tag, leaf)
        for name, other in others.items():
            worst = float((np.abs(grad - other[leaf]) / (S + 1e-300)).max())
            assert (np.abs(grad - other[leaf]) <= 1e-11 * S).all(), (tag, leaf, name, worst)


@pytest.mark.parametrize("tag", [s["tag"] for s in k2.ON_CENTRES_D])
def test_reference_has_autograds_non_finite_elements_on_centres(tag):
    """A basis in d itself with a query on every centre: NaN in d centers, a finite d log_sigs (the width does not go through the
    sqrt) -- the reference element for element where torch.autograd of the oracle's forward has them, the finite ones to 1e-11 S."""
    case = k2.Case(BY_TAG[tag])
    ref, auto = case.reference(), _autograd(case)
    assert np.isnan(auto["centers"]).all() and np.isfinite(auto["log_sigs"]).all()
    for leaf in k2.LEAVES:
        grad, S = ref[leaf]
        assert k2.same_nonfinite(grad, auto[leaf]), (tag, leaf)
        fin = np.isfinite(grad)
        assert (np.abs(grad[fin] - auto[leaf][fin]) <= 1e-11 * S[fin]).all(), (tag, leaf)


def test_regions_without_a_range_and_tiny_weights_are_what_the_cases_say():
    case = k2.Case(BY_TAG["r6_rows4"])
    ref = case.reference()
    assert (case.gamma()[:, 4:] == 0).all() and (case.gamma()[:, :4].max(axis=0) > 0.5).all()
    assert (ref["centers"][0][4:] == 0).all() and (ref["log_sigs"][0][4:] == 0).all() and (ref["centers"][1][4:] == 0).all()
    tiny = k2.Case(BY_TAG["r6_tiny"])
    gam = tiny.gamma()
    assert (gam[:, 0] > 0.99).all() and (gam[:, 1:] < 1e-6).all() and (gam[:, 1:] > 0).all()
    assert (tiny.gamma(np.float32)[:, 1:] > 0).all()             # none of them below float32's exact zero of the gate
    S = tiny.reference()["centers"][1]
    assert S[1:].max() < 1e-5 * S[0].max()                       # elements the max-norm bound cannot see


def test_yardstick_and_the_coefficient():
    """r32, the worst |err| / S of the float32 restatement over every case of the table: printed per case and leaf (the
    `yardstick` columns of profiles/k2_parity.txt come from the same function).  A case that needs more than 5e-5 S in plain
    float32 has the wrong inputs for its purpose."""
    r32 = 0.0
    for spec in k2.TABLE:
        case = k2.Case(spec)
        ref, y = case.reference(), case.yardstick()
        line = []
        for leaf in k2.LEAVES:
            assert k2.same_nonfinite(y[leaf], ref[leaf][0]), (case.tag, leaf)
            es, em = k2.ratios(y[leaf], *ref[leaf])
            if es > 5e-5:
                pytest.fail(f"test inputs, not the code under test: {case.tag} {leaf} needs {es:.2e} S in plain float32")
            line.append(f"{leaf} {es:.2e}")
            r32 = max(r32, es)
        print(f"{case.tag:32s} " + "  ".join(line))
    print(f"r32 = {r32:.3e}; R32 = {k2.R32:.3e}, C_S = {k2.C_S:.3e}")
    assert r32 <= 1.25e-5
    assert k2.R32 / 2 < r32 <= k2.R32, "R32 in _k2_util.py is not what the yardstick gives"
    assert k2.C_S == 4 * k2.R32 and k2.C_S <= 5e-5


HAND = [  # N, B -> groups, QSB, per_wave, bias_blocks
    (33, 1, 1, 1, 1, 1), (33, 5, 1, 1, 2, 1), (33, 255, 1, 1, 64, 4), (33, 256, 1, 1, 64, 4), (33, 257, 1, 2, 33, 5),
    (33, 16383, 1, 64, 64, 256), (33, 16384, 1, 64, 64, 256),
    (64, 1, 1, 1, 1, 1), (64, 5, 1, 1, 2, 1), (64, 255, 1, 1, 64, 4), (64, 256, 1, 1, 64, 4), (64, 257, 1, 2, 33, 5),
    (64, 16383, 1, 64, 64, 256), (64, 16384, 1, 64, 64, 256),
    (65, 1, 2, 1, 1, 1), (65, 5, 2, 1, 2, 1), (65, 255, 2, 1, 64, 4), (65, 256, 2, 1, 64, 4), (65, 257, 2, 2, 33, 5),
    (65, 16383, 2, 64, 64, 256), (65, 16384, 2, 64, 64, 256),
]


@pytest.mark.parametrize("N,B,groups,QSB,per_wave,bias_blocks", HAND)
def test_layout_rules_by_hand(N, B, groups, QSB, per_wave, bias_blocks):
    p = k2.k2_plan(N, B, 7, 10, "gaussian", False)
    assert (p["groups"], p["QSB"], p["per_wave"], p["bias_blocks"]) == (groups, QSB, per_wave, bias_blocks)
    assert p["grid"] == groups * QSB and p["name"] == "rbf_vjp_kernel<D=7,OP=10,BC=0,GATED=0>" and p["lds"] == 4 * 18 * 65 * 4


def test_layout_lds_and_names_by_hand():
    assert k2.k2_plan(130, 300, 8, 64, "gaussian", False)["lds"] == 75920
    assert k2.k2_plan(50, 300, 7, 100, "gaussian", False)["lds"] == 112320
    assert k2.k2_plan(130, 300, 8, 128, "gaussian", False)["lds"] == 142480
    assert k2.k2_plan(650, 600, 8, 4, "matern52", True)["name"] == "rbf_vjp_kernel<D=8,OP=4,BC=3,GATED=1>"
    assert k2.k2_plan(1, 70, 1, 1, "inverse_multiquadric", False)["name"] == "rbf_vjp_kernel<D=3,OP=2,BC=2,GATED=0>"
    assert k2.k2_plan(65, 600, 5, 5, "inverse_quadratic", True)["name"] == "rbf_vjp_kernel<D=7,OP=5,BC=1,GATED=1>"
    # many centre groups: the slab count comes from the 8192 waves, not from the batch
    p = k2.k2_plan(64 * 100, 100000, 7, 10, "gaussian", False)
    assert (p["groups"], p["QSB"], p["per_wave"], p["grid"]) == (100, 21, 1191, 2100)
