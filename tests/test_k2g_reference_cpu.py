"""The launch rules, the operand restatement, the floor and the coefficient of tests/_k2g_util.py, without a GPU: k2g_plan against
values worked out by hand from vjp_layout, vjpg_slices, plan_vjp and launch_vjp_gram_mode; the precondition that K2g and K2h run
with the same number of slabs where tests/test_gpu_k2g.py tells them apart by their bits; the box of the expansion restated from
gram_header; what the cases claim about themselves; R_G -- the worst error of the float32 restatement with K2g's operand treatment
beyond the documented floor A -- which fixes the coefficient of the element-wise bound; the condition that A stays below C_G S on
four elements of five, so that the floor cannot hide a failure; and the sweep over the spread of the weight columns that says where
hbar's operand scheme stops being float32-grade."""
import functools

import numpy as np
import pytest

import _k2_util as k2
import _k2h_util as kh
import _k2g_util as kg


# ------------------------------------------------------------------------------------------------ the launch rules
#        B      N     O   S  bpb  working  empty  blocks of the last working slice  queries of the last block
HAND = [(2048, 100, 5, 8, 8, 8, 0, 8, 32),
        (2049, 100, 5, 9, 8, 9, 0, 1, 1),
        (2080, 100, 5, 9, 8, 9, 0, 1, 32),
        (2081, 100, 5, 9, 8, 9, 0, 2, 1),
        (2113, 100, 5, 9, 8, 9, 0, 3, 1),
        (2145, 100, 5, 9, 8, 9, 0, 4, 1),
        (2305, 100, 5, 10, 8, 10, 0, 1, 1),
        (16384, 100, 5, 64, 8, 64, 0, 8, 32),
        (16385, 100, 5, 64, 9, 57, 7, 9, 1),
        (11777, 2049, 10, 47, 8, 47, 0, 1, 1),
        (11777, 2049, 11, 46, 9, 41, 5, 9, 1)]


@pytest.mark.parametrize("B,N,O,S,bpb,working,empty,last,lastq", HAND)
def test_k2g_plan_by_hand(B, N, O, S, bpb, working, empty, last, lastq):
    """2145 queries are 68 blocks: eight slices of 8 and one of 4, whose stage(0 + 3) is the first reuse of ring slot 0.  16385 are
    513 blocks in slices of 9: 57 slices hold them, 7 of the 64 find nothing.  N = 2049: 65 chunks, 17 blocks of centres, the last
    with one active wave; 369 query blocks: O = 10 asks for 61 slices, more than eight blocks a slice allow (47 = the slabs allocated);
    O = 11 asks for 46, which leaves 41 slices of 9 with work and five without."""
    p = kg.k2g_plan(N, B, 3, O, "gaussian")
    assert (p["S"], p["bpb"], p["working"], p["empty"], p["last_slice_blocks"], p["last_block_queries"]) == (S, bpb, working, empty, last, lastq)
    assert p["grid"] == (-(-N // 128), S) and p["OC"] == (O <= 10) and S * bpb >= p["nqb"] > (working - 1) * bpb
    assert p["bias_blocks"] == (256 if B >= 16384 else -(-B // 64))
    if N == 2049:
        assert p["gb"] == 17 and p["idle_waves"] == 3 and p["q"] == (47 if O == 10 else 46) and p["nqb"] == 369 and p["QSB"] == 47
    else:
        assert p["gb"] == 1 and p["idle_waves"] == 0 and p["nchunks"] == 4


def test_k2g_plan_modes_paddings_and_idle_waves():
    assert [kg.k2g_plan(N, 2049, 3, 5, "gaussian")["idle_waves"] for N in (15, 16, 17, 31, 32, 33, 96, 97, 127, 128, 129, 130)] == \
        [3, 3, 3, 3, 3, 2, 1, 0, 0, 0, 3, 3]
    assert [kg.k2g_plan(N, 2049, 3, 5, "gaussian")["gb"] for N in (128, 129)] == [1, 2]
    assert [kg.k2g_plan(40, 2049, D, 5, "gaussian")["DC"] for D in range(1, 9)] == [3, 3, 3, 4, 7, 7, 7, 8]
    for mode, pieces in ((1, 10), (2, 7)):                      # the frozen modes: other resident rounds, the same slices here
        for B in kg.FROZEN_EDGES:
            p, full = kg.k2g_plan(100, B, 3, 5, "gaussian", mode), kg.k2g_plan(100, B, 3, 5, "gaussian")
            assert (p["S"], p["bpb"], p["last_slice_blocks"]) == (full["S"], full["bpb"], full["last_slice_blocks"]) and p["pieces"] == pieces
    assert kg.k2g_plan(100, 2145, 3, 5, "gaussian")["last_slice_blocks"] == 4 and kg.k2g_plan(100, 2049, 3, 5, "gaussian")["pieces"] == 12


def test_k2g_and_k2h_run_with_the_same_slabs_where_the_bits_tell_them_apart():
    """Behind a raised flag launch_vjp_f16 runs with K2g's S.  A forced K2H call has the same bits only where its own rule gives the
    same S: every case of the table below 16384 queries with at most 130 centres."""
    n = 0
    for spec in kg.TABLE + kh.RANGES:
        if spec["B"] < 16384 and spec["K"] <= 130:
            a = kg.k2g_plan(spec["K"], spec["B"], spec["D"], spec["O"], spec["basis"])
            assert a["S"] == kh.k2h_plan(spec["K"], spec["B"], spec["D"], spec["O"], spec["basis"])["S"], spec["tag"]
            n += 1
    assert n >= len(kg.TABLE) - 4
    assert kg.k2g_plan(40, 4352, 5, 11, "gaussian")["S"] == kh.k2h_plan(40, 4352, 5, 11, "gaussian")["S"] == 17      # the reuse test's first call


# ------------------------------------------------------------------------------------------------ the cases
def test_table_covers_what_it_claims():
    S = kg.SHAPES
    assert {s["D"] for s in S} == set(range(1, 9)) and {s["O"] for s in S} == {1, 2, 5, 9, 10, 11, 15, 16}
    assert {s["K"] for s in S} | {kg.ONE_CENTRE["K"]} == {1, 15, 16, 17, 31, 32, 33, 96, 97, 127, 128, 129, 130}
    assert {s["basis"] for s in S} == {"gaussian", "gaussian_wide", "gaussian_wider", "inverse_quadratic", "inverse_multiquadric"}
    assert any(s["ns"] == 0 for s in S) and any(0 < s["ns"] < s["D"] for s in S) and any(s["ns"] == s["D"] for s in S)
    assert 12 <= len(S) + 1 <= 14 and all(s["B"] > 2048 for s in S) and len({s["B"] % 32 for s in S}) >= 8
    # every compiled (DC, BC, OC) instance: twelve rows cannot hold 24 instances, so the count runs over the whole table
    inst = {(k2.padded_D(s["D"]), k2.bclass(s["basis"]), s["O"] <= 10) for s in kg.TABLE}
    assert inst == {(dc, bc, oc) for dc in (3, 4, 7, 8) for bc in (0, 1, 2) for oc in (True, False)}
    assert len({s["tag"] for s in kg.TABLE}) == len(kg.TABLE) and not set(kg.BY_TAG) & set(kh.BY_TAG)


def test_the_box_of_the_expansion_and_the_cases_inside_it():
    """Every query of every case lies inside the box (|x'_i| < 0.999 * 2^ex), so K2g computes; one centre has no box at all."""
    for spec in kg.TABLE:
        case = kg.CaseG(spec)
        r, lim = kg.box_limit(case.params["params"]["rbf_list"]["centers"][0])
        assert lim == np.float32(1.998), spec["tag"]                      # centres in [-1, 1.6]: half width < 1.3, 1.25 x that < 2
        fin = np.isfinite(case.x).all(axis=1)
        assert (np.abs(case.x[fin] - r[None]) < 0.9 * lim).all(), spec["tag"]
    one = kg.CaseG(kg.ONE_CENTRE)
    assert kg.header(one.params["params"]["rbf_list"]["centers"][0])[2] == 0.0


def test_range_cases_are_what_they_say():
    far = kg.CaseG(kg.BY_TAG["g_far"])
    rl = far.params["params"]["rbf_list"]
    d = np.sqrt(((far.x[:, None, :].astype(np.float64) - rl["centers"][0][None]) ** 2).sum(-1)) / np.exp(rl["log_sigs"][0].astype(np.float64))[None]
    assert 6.0 <= d.min() and d.max() <= 8.0
    assert np.exp(-d.min() ** 2) < 2.0 ** -24 / 1e4                        # phi far below what an ungained pair resolves
    assert (far.gamma() > 0.5).all()
    for tag in ("g_wcols_gauss", "g_wcols_iq", "g_wcols_imq"):
        w = kg.CaseG(kg.BY_TAG[tag])
        so = kh.pow2_above(np.abs(w.params["params"]["linear"]["kernel"]).max(axis=0))
        assert so.max() / so.min() >= 2.0 ** 19 and so.argmin() == 0 and (w.g[:, 1:] == 0).all() and (w.g[:, 0] != 0).all()
    assert {k2.bclass(kg.BY_TAG[t]["basis"]) for t in ("g_wcols_gauss", "g_wcols_iq", "g_wcols_imq")} == {0, 1, 2}
    g = kg.CaseG(kg.BY_TAG["g_grows_spread"])
    rows = np.abs(g.g).max(axis=1)
    assert rows.max() / rows.min() >= 2.0 ** 18


def test_plain_pair_is_short_by_less_than_the_subnormal_grid():
    """split_pair_plain: hi + lo <= p, short by less than 2^-24 absolute below 2^-4 and by 2^-21 relative above."""
    rng = np.random.default_rng(2)
    for e in range(-40, 15):
        p = (rng.uniform(1.0, 2.0, size=1024) * 2.0 ** e).astype(np.float32)
        hi, lo = kg.split_plain(p)
        back = hi.astype(np.float64) + lo.astype(np.float64)
        assert (back <= p).all() and (p - back < max(2.0 ** -24, 2.0 ** -21 * 2.0 ** (e + 1))).all(), e
    hi, lo = kg.split_plain(np.float32([0.0, 2.0 ** -30]))
    assert (hi == 0).all() and (lo == 0).all()


# ------------------------------------------------------------------------------------------------ the coefficient
@functools.lru_cache(maxsize=None)
def _measured():
    """Per case of the yardsticked table: {leaf: (worst (|err| - A)+ / S, share of the elements with S > 0 where A >= C_G S,
    max-norm ratio)} of yardstick_g against the float64 reference."""
    out = {}
    for spec in kg.YARDSTICKED:
        case = kg.CaseG(spec)
        ref, y, A = case.reference(), case.yardstick_g(), case.floor()
        row = {}
        for leaf in k2.LEAVES:
            r, S = ref[leaf]
            assert kg.same_nonfinite(y[leaf], r), (case.tag, leaf)
            es, em = kg.ratios_g(y[leaf], r, S, A[leaf])
            pos = S > 0
            row[leaf] = (es, float((A[leaf][pos] >= kg.C_G * S[pos]).mean()) if pos.any() else 0.0, em)
        out[case.tag] = row
        print(f"{case.tag:18s} " + "  ".join(f"{leaf} {v[0]:.2e} (A over the line {v[1]:.2f}, max-norm {v[2]:.3f})" for leaf, v in row.items()))
    return out


def test_yardstick_g_and_the_coefficient():
    m = _measured()
    r_g, where = max((v[0], f"{tag} {leaf}") for tag, row in m.items() for leaf, v in row.items())
    print(f"r_g = {r_g:.3e} at {where}; R_G = {kg.R_G:.3e} ({kg.R_G_CASE}), C_G = {kg.C_G:.3e}")
    assert kg.R_G / 2 < r_g <= kg.R_G, "R_G in _k2g_util.py is not what the yardstick gives"
    assert where == kg.R_G_CASE
    assert kg.C_G == 4 * kg.R_G and kg.C_G <= 5e-5
    assert kg.R_G <= 3 * kh.R_H, "K2g's operand treatment costs more than a factor 3 over K2h's: say in the summary which operand does it"


def test_yardstick_g_is_inside_the_bounds_the_kernel_is_held_to():
    for tag, row in _measured().items():
        for leaf, (es, _, em) in row.items():
            assert es <= kg.C_G / 4 and em <= 1.0, (tag, leaf, es, em)


def test_the_floor_cannot_hide_a_failure():
    """Outside the operand-range group: A < C_G S on at least 80 % of the elements of every leaf that have a scale at all (a region
    without a range row has none: there the GPU test asserts exact zeros)."""
    for tag, row in _measured().items():
        if tag in kg.RANGE_TAGS:
            continue
        for leaf, (_, share, _) in row.items():
            assert share <= 0.2, (tag, leaf, share)
    A = kg.CaseG(kg.BY_TAG["g_b2049"]).floor()
    assert (A["bias"] == 0).all() and all((A[leaf] > 0).all() for leaf in ("centers", "log_sigs", "kernel"))


def test_the_scale_of_the_largest_cotangent_times_column_is_what_the_wcols_cases_need():
    """The restatement with hbar's scale as it was, s_g max_o s_o (kg.RANGE_NOTE), misses the project's max-norm bound on K2h's own
    wcols case by the factor the kernel missed it by on the GPU (7.05); with the scale of the largest operand present it is
    float32-grade again."""
    case = kg.CaseG(kh.BY_TAG["h_wcols_spread"])
    r, S = case.reference()["centers"]
    norm = k2.MAXNORM_REL * np.abs(r).max() + k2.MAXNORM_ABS
    now = np.abs(case.yardstick_g()["centers"].astype(np.float64) - r)
    case.before_fix = True
    was = np.abs(case.yardstick_g()["centers"].astype(np.float64) - r)
    print(f"h_wcols_spread d centers max-norm ratio: s_g max s_o {was.max() / norm:.3f}, largest operand present {now.max() / norm:.3f}")
    assert 6.5 < was.max() / norm < 7.5 and now.max() / norm < 0.05 and (now / (S + 1e-300)).max() <= kg.R_G


def test_column_spread_sweep():
    """Where hbar's operand scheme stops being float32-grade: yardstick_g on the wcols nets with the weight columns over 2^-s .. 2^s,
    the cotangent in the smallest column alone.  Printed per basis class: worst |err| / S and max-norm ratio of d centers.  Whatever
    the spread, the restatement must stay inside the project's max-norm bound -- K2h does on the same inputs."""
    bad = []
    for tag in ("g_wcols_gauss", "g_wcols_iq", "g_wcols_imq"):
        base = dict(kg.BY_TAG[tag], wcols=False)
        for s in range(0, 11):
            case = kg.CaseG(dict(base, tag=f"{tag}_s{s}", net=tag, wspread=s))
            ref, y = case.reference(), case.yardstick_g()
            r, S = ref["centers"]
            err = np.abs(y["centers"].astype(np.float64) - r)
            es, em = float((err / (S + 1e-300)).max()), float(err.max() / (k2.MAXNORM_REL * np.abs(r).max() + k2.MAXNORM_ABS))
            print(f"K2GSPREAD {case.basis:22s} columns 2^+-{s:<2d} d centers |err| / S {es:.2e}  max-norm ratio {em:.3f}")
            if em > 1.0:
                bad.append((case.basis, s, em))
    assert not bad, bad
