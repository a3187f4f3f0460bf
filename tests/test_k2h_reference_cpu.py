"""The chunked float64 reference, the restated operand pairs and launch rules and the yardsticks of tests/_k2h_util.py, without a
GPU: the reference against the unchunked one and torch.autograd of the oracle, the NumPy restatement of f16_split.h at the ends of
its documented range, k2h_plan against values worked out by hand, and R_H -- the worst error of the float32 restatement with K2h's
operand pairs over the whole table, which fixes the coefficient of the element-wise bound of tests/test_gpu_k2h.py."""
import numpy as np
import pytest

import _k2_util as k2
import _k2h_util as kh
from test_k2_reference_cpu import _autograd


@pytest.mark.parametrize("tag", ["h_d5_o5_n31", "h_d7_o8_n33", "h_wcols_spread"])
def test_chunked_reference_is_the_reference(tag):
    case = kh.CaseH(kh.BY_TAG[tag])
    assert case.B > 8 * kh.CHUNK and case.B % kh.CHUNK                      # several chunks and a ragged last one
    ref = case.reference()
    whole = k2.vjp_reference(case.basis, case.params, case.x, case.g, case.gamma())
    auto = _autograd(case)
    for leaf in k2.LEAVES:
        grad, S = ref[leaf]
        assert grad.dtype == np.float64 and grad.shape == S.shape == whole[leaf][0].shape
        assert (S >= np.abs(grad)).all(), (tag, leaf)
        assert (np.abs(S - whole[leaf][1]) <= 1e-13 * S).all(), (tag, leaf)
        for name, other in (("unchunked", whole[leaf][0]), ("autograd", auto[leaf])):
            worst = float((np.abs(grad - other) / (S + 1e-300)).max())
            assert (np.abs(grad - other) <= 1e-11 * S).all(), (tag, leaf, name, worst)


def test_plain_yardstick_in_chunks_is_the_k2_yardstick():
    """The same float32 operations in the same order as k2.vjp_float32: only the matrix product g W^T may round differently
    between a chunk's rows and the whole batch's (BLAS), which moves hbar by an ulp."""
    case = kh.CaseH(kh.BY_TAG["h_d5_o5_n31"])
    mine, theirs = case.yardstick(), k2.vjp_float32(case.basis, case.params, case.x, case.g, case.gamma(np.float32))
    ref = case.reference()
    assert np.array_equal(mine["bias"], theirs["bias"]) and np.array_equal(mine["kernel"], theirs["kernel"])
    for leaf in ("centers", "log_sigs"):
        assert (np.abs(mine[leaf].astype(np.float64) - theirs[leaf]) <= 2.0 ** -22 * ref[leaf][1]).all(), leaf


def test_a_card_without_a_range_row_weighs_nothing():
    case = kh.CaseH(kh.BY_TAG["h_norange"])
    assert (case.gamma() == 0).all() and (case.gamma(np.float32) == 0).all()
    ref = case.reference()
    assert all((ref[leaf][0] == 0).all() and (ref[leaf][1] == 0).all() for leaf in ("centers", "log_sigs", "kernel"))
    assert (ref["bias"][0] != 0).all()


def test_operand_range_cases_are_what_they_say():
    w = kh.CaseH(kh.BY_TAG["h_wcols_spread"])
    W = w.params["params"]["linear"]["kernel"]
    so = kh.pow2_above(np.abs(W).max(axis=0))
    assert so.max() / so.min() >= 2.0 ** 19 and so.argmin() == 0 and (w.g[:, 1:] == 0).all() and (w.g[:, 0] != 0).all()
    g = kh.CaseH(kh.BY_TAG["h_grows_spread"])
    rows = np.abs(g.g).max(axis=1)
    assert rows.max() / rows.min() >= 2.0 ** 18
    # within 2^-29 of each scale: the documented range of a pair
    assert np.abs(g.g)[g.g != 0].min() >= 2.0 ** -29 * kh.pow2_above(np.abs(g.g).max())
    z = kh.CaseH(kh.BY_TAG["h_zero_col"])
    assert (z.params["params"]["linear"]["kernel"][:, 1] == 0).all() and kh.pow2_above(np.float32(0)) == 1
    o = kh.CaseH(kh.BY_TAG["h_outside"])
    gam = o.gamma()
    assert (gam[::3] == 0).all() and (o.gamma(np.float32)[::3] == 0).all() and (gam[1::3] > 0).all()
    assert np.isfinite(((o.x[:, None, :] - o.params["params"]["rbf_list"]["centers"][0][None]) ** 2).sum(-1, dtype=np.float32)).all()
    for p in kh.NONFINITE:
        n = kh.CaseH(p)
        assert (np.abs(np.nan_to_num(n.g, nan=0.0, posinf=0.0)).max(axis=0) >= 2).all()     # every column holds a |g| >= 2


def test_shapes_cover_what_they_claim():
    """The table holds every D, both ends of every output padding, the centre counts around the
    tile, block and group, the five bases and the three kinds of gate."""
    S = kh.SHAPES
    assert {s["D"] for s in S} == set(range(1, 9)) and {s["O"] for s in S} == {1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 16}
    assert {s["K"] for s in S} == {1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130}
    assert {s["basis"] for s in S} == {"gaussian", "gaussian_wide", "gaussian_wider", "inverse_quadratic", "inverse_multiquadric"}
    assert any(s["ns"] == 0 for s in S) and any(0 < s["ns"] < s["D"] for s in S) and any(s["ns"] == s["D"] for s in S)
    assert all(s["B"] > 2048 for s in S) and len({s["B"] % 32 for s in S}) >= 8


# ------------------------------------------------------------------------------------------------ f16_split.h restated
def _back(hi, lo):
    with np.errstate(invalid="ignore"):
        return hi.astype(np.float64) + lo.astype(np.float64) / 2048.0


def test_static_pair_over_its_documented_range():
    """hi + 2^-11 lo reproduces 2^15 v to 2^-21 relative for 2^-14 <= |2^15 v| < 2^15."""
    rng = np.random.default_rng(0)
    for e in range(-14, 15):
        w = rng.uniform(1.0, 2.0, size=2048) * 2.0 ** e * rng.choice([-1, 1], size=2048)
        w[0], w[1] = 2.0 ** e, -(2.0 ** e)
        v = (w / 32768.0).astype(np.float32)
        hi, lo = kh.split_static(v)
        assert np.isfinite(hi.astype(np.float32)).all() and np.isfinite(lo.astype(np.float32)).all()
        rel = np.abs(_back(hi, lo) - v.astype(np.float64) * 32768.0) / np.abs(v.astype(np.float64) * 32768.0)
        assert rel.max() <= 2.0 ** -21, (e, rel.max())


def test_static_pair_at_and_beyond_the_scale():
    hi, lo = kh.split_static(np.array([1.0, -1.0], np.float32))              # |v| = 1: 2^15, no overflow
    assert (hi.astype(np.float32) == [32768.0, -32768.0]).all() and (lo == 0).all()
    hi, lo = kh.split_static(np.array([2.0, -2.0], np.float32))              # 2 x scale: 2^16 is no f16 number
    assert np.isinf(hi).all() and np.isinf(lo).all() and (np.sign(hi.astype(np.float32)) == -np.sign(lo.astype(np.float32))).all()
    assert np.isnan(_back(hi, lo)).all()                                     # Inf - Inf: the precondition |v| <= 1 is a real one


def test_cotangent_pair_of_non_finite_elements():
    v = np.array([0.25, np.nan, np.inf, -np.inf], np.float32)
    hi, lo = kh.split_cotangent(v)
    sh, sl = kh.split_static(v[:1])
    assert hi[0] == sh[0] and lo[0] == sl[0] and np.isnan(hi[1]) and np.isnan(lo[1])
    assert (hi[2:].astype(np.float32) == [65504.0, -65504.0]).all() and (lo[2:].astype(np.float32) == [np.inf, -np.inf]).all()
    w = np.array([[0.5, -0.5]], np.float32)                                  # x a weight of either sign: the infinity keeps the product's
    wh, wl = kh.split_static(w)
    with np.errstate(invalid="ignore"):
        prod = kh.pair_product(hi[2:, None], lo[2:, None], wh, wl)
    assert np.array_equal(prod, np.array([[np.inf, -np.inf], [-np.inf, np.inf]], np.float32))


def test_phi_pair_over_its_documented_range():
    rng = np.random.default_rng(1)
    for e in range(-14, 15):                                                  # P = 2^14 phi, phi <= 1
        P = (rng.uniform(1.0, 2.0, size=2048) * 2.0 ** e).astype(np.float32)
        P[0] = 2.0 ** e
        P = np.minimum(P, np.float32(16384.0))
        hi, lo = kh.split_phi(P)
        assert (hi.astype(np.float32) <= P).all() and (lo.astype(np.float32) >= 0).all()          # truncated: the residual is >= 0
        assert ((hi.view(np.uint16) & 0x3FF) == (P.view(np.uint32) >> 13 & 0x3FF)).all()          # the top 11 bits, as they are
        rel = np.abs(_back(hi, lo) - P.astype(np.float64)) / P
        assert rel.max() <= 2.0 ** -21, (e, rel.max())
    assert kh.f16_rtz(np.float32(65519.0)) == np.float16(65504) and kh.f16_rtz(np.float32(1e9)) == np.float16(65504)
    assert kh.f16_rtz(np.float32(-1.0009766 - 1e-4)) == np.float16(-1.0009766) and np.isnan(kh.f16_rtz(np.float32(np.nan)))


# ------------------------------------------------------------------------------------------------ the launch rules
HAND = [  # N, B -> S, bpw, waves without a block, blocks of the last working wave
    (1, 2048, 8, 2, 0, 2), (33, 2049, 9, 2, 3, 1), (100, 2304, 9, 2, 0, 2), (100, 2305, 10, 2, 3, 1), (3072, 4352, 16, 3, 18, 1),
    (1000, 8333, 33, 2, 1, 1),
]


@pytest.mark.parametrize("N,B,S,bpw,empty,last", HAND)
def test_k2h_plan_by_hand(N, B, S, bpw, empty, last):
    """2305 queries are 73 blocks = 36 waves of two and one of one, 8333 are 261 = 130 and one: their last working wave holds one
    block as well, as the rule gives it."""
    p = kh.k2h_plan(N, B, 3, 5, "gaussian")
    assert (p["S"], p["bpw"], p["empty_waves"], p["last_wave_blocks"]) == (S, bpw, empty, last)
    assert p["grid"] == (-(-N // 32), S) and (p["DC"], p["OP"], p["RFQ"], p["BC"]) == (3, 5, 4, 0)
    assert 4 * S * bpw >= p["nqb"] > (4 * S - empty - 1) * bpw


def test_k2h_plan_caps_and_paddings():
    p = kh.k2h_plan(3072, 4352, 3, 5, "gaussian")
    assert p["q"] == 16 and p["QSB"] == 17                                    # K2h's own rule caps, not the layout's slabs
    p = kh.k2h_plan(100, 2305, 3, 5, "gaussian")
    assert p["q"] == 19 and p["QSB"] == 10                                    # the layout's slabs cap
    assert kh.k2h_plan(100, 2049, 3, 5, "gaussian")["last_block_queries"] == 1
    assert [kh.k2h_plan(9, 2048, D, 2, "gaussian")["RFQ"] for D in range(1, 9)] == [4, 4, 4, 8, 8, 8, 8, 12]
    assert [kh.k2h_plan(9, 2048, 3, O, "gaussian")["OP"] for O in (1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 16)] == [2, 2, 4, 4, 5, 8, 8, 10, 10, 16, 16]
    for B in kh.BIG_EDGES:
        p = kh.k2h_plan(3072, B, 3, 5, "gaussian_wide")
        assert (p["S"], p["bpw"], p["empty_waves"]) == (16, 3, 18) and p["last_wave_blocks"] == (1 if B == 4352 else 2)


# ------------------------------------------------------------------------------------------------ the coefficient
def test_yardstick_h_and_the_coefficient():
    """r_h, the worst |err| / S of the float32 restatement with K2h's operand pairs over every case of the table, beside the plain
    float32 yardstick's: printed per case and leaf.  A case that needs more than 5e-5 S in either has the wrong inputs."""
    r_h = r32 = 0.0
    for spec in kh.TABLE:
        case = kh.CaseH(spec)
        ref, yh, y = case.reference(), case.yardstick_h(), case.yardstick()
        line = []
        for leaf in k2.LEAVES:
            assert kh.same_nonfinite(yh[leaf], ref[leaf][0]) and kh.same_nonfinite(y[leaf], ref[leaf][0]), (case.tag, leaf)
            eh, e32 = kh.ratios_h(yh[leaf], *ref[leaf])[0], kh.ratios_h(y[leaf], *ref[leaf])[0]
            if max(eh, e32) > 5e-5:
                pytest.fail(f"test inputs, not the code under test: {case.tag} {leaf} needs {eh:.2e} S with the pairs, {e32:.2e} S in plain float32")
            line.append(f"{leaf} {eh:.2e} ({e32:.2e})")
            r_h, r32 = max(r_h, eh), max(r32, e32)
        print(f"{case.tag:24s} " + "  ".join(line))
    print(f"r_h = {r_h:.3e} (plain float32: {r32:.3e}); R_H = {kh.R_H:.3e}, C_H = {kh.C_H:.3e}")
    assert kh.R_H / 2 < r_h <= kh.R_H, "R_H in _k2h_util.py is not what the yardstick gives"
    assert kh.C_H == 4 * kh.R_H and kh.C_H <= 5e-5
    assert r_h <= 2 * r32, "the operand pairs cost more than a factor 2 over plain float32: say in the summary which operand does it"
