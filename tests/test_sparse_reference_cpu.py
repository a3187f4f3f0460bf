"""tests/_sparse_util.py without a GPU: its references against the oracle, its restated host rules of rbf_sparse.hip against values
worked out by hand, the conditions on the inputs that make each case of its table exercise the edge it names, and the float32
yardstick's worst error over the table, which fixes the coefficient of the element-wise bound of tests/test_gpu_sparse_edges.py."""
import json
import os

import numpy as np
import pytest

import _k2_util as k2
import _sparse_util as su
from oracle import c_oracle as co
from oracle import irbfn_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_CARDS = {}


def card(tag):
    if tag not in _CARDS:
        _CARDS[tag] = su.Card(su.BY_TAG[tag])
    return _CARDS[tag]


def fixture_cfg(run):
    with open(os.path.join(GOLDEN, f"ckpt_{run}.json")) as f:
        return json.load(f)


def max_live(cfg, x=None):
    """Brute force: the largest number of live regions over x (gated coordinates suffice) and a dense sample."""
    n = int(su.live(cfg, su.dense_sample(cfg)).sum(axis=1).max())
    return n if x is None else max(n, int(su.live(cfg, x).sum(axis=1).max()))


# ------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("tag", ["cap96", "e32_nr87", "perm", "repeated_rows"])
def test_references_agree_with_the_oracle_where_no_factor_lies_between_the_two_zeros(tag):
    c = card(tag)
    assert not su.between_the_zeros(c.cfg, c.x), "test inputs: a factor is 0 for the kernels and not in float64"
    ref, scale = c.forward_reference()
    p64, x64 = orc.cast_params(c.params, np.float64), c.x.astype(np.float64)
    out = orc.wcrbfnet_apply(c.cfg, p64, x64)
    assert (np.abs(ref - out) <= 1e-11 * scale).all() and (scale >= np.abs(ref)).all()
    from test_gpu_gram import _terms_scale
    assert np.allclose(scale, _terms_scale(c.cfg, p64, x64), rtol=1e-12, atol=0)
    hand = co.wcrbf_vjp(c.cfg, c.params, c.x, c.g, np.float64)["params"]
    for leaf, (grad, S) in c.reference().items():
        other = hand[k2.LEAF_PATH[leaf][0]][k2.LEAF_PATH[leaf][1]]
        assert grad.shape == other.shape and (np.abs(grad - other) <= 1e-11 * S).all(), (tag, leaf)


def test_the_gate_has_exact_zeros_where_the_oracle_has_1e_minus_17():
    c = card("long_b10000")
    gam, orc_gam = c.gamma(), k2.tanh_gate(c.cfg, c.x)
    far = ~c.live()
    assert far.any() and (gam[far] == 0).all() and (orc_gam[far] > 0).any() and orc_gam[far].max() < 1e-7
    assert np.array_equal(gam[~far], orc_gam[~far])
    assert np.array_equal(c.live(), k2.tanh_gate(c.cfg, c.x, np.float32) != 0) or su.between_the_zeros(c.cfg, c.x)


# ------------------------------------------------------------------------------------------------ host rules
def test_host_rules_on_the_two_fixture_cards_by_hand():
    """dnmpc_128regions: ranges per gated coordinate 1, 2, 4, 4, 1, 2, 2 -> E = 16; non-zero together 1, 2, 3, 2, 1, 2, 2 (the four
    ranges of coordinate 2 are 1.8 wide with a margin of 0.901: the widened intervals of ranges j - 1 and j + 1 meet inside range
    j) -> cap = 48; DESIGN.md: 3.6 of 128 regions live.  Its worst case of 32 is that of queries off the centre lines of those
    ranges: on a strip 0.002 wide around one, three ranges of coordinate 2 are live in float32 and the brute force finds the 48.
    The 12-region Frenet card: E = 12, cap = its 12 regions, 5.7 live -> not preferred."""
    cfg = fixture_cfg("dnmpc_128regions")
    s = su.setup(cfg)
    assert (s["ok"], s["E"], s["cap"], s["nr"], s["OPS"]) == (True, 16, 48, 128, 10) and round(s["mean"], 1) == 3.6
    assert s["RS"] == 10 * 8 + 4                                           # K EW = 80: 20 slots, made odd
    assert max_live(cfg) == 48
    rng = np.random.default_rng(0)
    lo, hi = [min(v) for v in cfg["lower_bounds"]], [max(v) for v in cfg["upper_bounds"]]
    assert su.live(cfg, rng.uniform(lo, hi, size=(20000, 7)).astype(np.float32)).sum(axis=1).max() == 32
    assert su.sparse_preferred(cfg, 65) and not su.sparse_preferred(cfg, 64)
    assert su.vjp_eligible(cfg) and su.vjp_lds_fits(cfg)
    assert [su.vjp_slices(cfg, B) for B in (1, 5000, 20000, 80000)] == [8, 8, 8, 8]
    assert su.k1r_launch(cfg, 513) == {"kernel": "rbf_fwd_sparse<D=7,OP=10,BC=1,ROLL=0,GC=0>", "grid": 3, "block": 256}
    assert su.k1r_launch(cfg, 70001, roll=True)["kernel"] == "rbf_fwd_sparse<D=7,OP=10,BC=1,ROLL=1,GC=1>"
    cfg = fixture_cfg("dnmpc_12regions_frenet_l1_bigdata")
    s = su.setup(cfg)
    assert (s["ok"], s["E"], s["cap"], s["nr"], s["OPS"]) == (True, 12, 12, 12, 2) and round(s["mean"], 1) == 5.7
    assert not su.sparse_preferred(cfg, 5000) and su.vjp_slices(cfg, 5000) == 64
    assert su.k1r_launch(cfg, 65)["kernel"] == "rbf_fwd_sparse<D=8,OP=2,BC=0,ROLL=0,GC=0>"


def test_small_rules_by_hand():
    assert [su.sparse_ops(O) for O in (1, 2, 3, 5, 6, 10, 11, 16, 17)] == [2, 2, 5, 5, 10, 10, 16, 16, -1]
    assert su.slice_bounds(10000, 8)[0] == (0, 1250) and su.slice_bounds(3, 64)[20:23] == [(0, 0), (0, 1), (1, 1)]
    assert sum(b - a for a, b in su.slice_bounds(777, 64)) == 777
    im = su.img_layout(128, 84, 16, 10)                 # 256 + 128 + 64 + 160 dwords -> 768; 128 x 84 = 10752 -> 43 KB of centres
    assert im == {"small": 768, "total": 768 + 10752}
    # one region per combination: the 4 x 4 unit grid; two ranges live per coordinate
    s = su.setup(card("b257").cfg)
    assert (s["E"], s["cap"], s["RS"]) == (8, 4, 12)     # K EW = 12: three slots, odd already
    assert su.vjp_slices(card("b257").cfg, 257) == 64    # 16 regions: 64 slices for 1024 waves


def test_limits_from_both_sides():
    for fits, over in su.LIMIT_PAIRS:
        a, b = su.setup(su.cfg_only(su.LIMIT_BY_TAG[fits])), su.setup(su.cfg_only(su.LIMIT_BY_TAG[over]))
        assert a["ok"] and not b["ok"], (fits, over)
    a = su.setup(su.cfg_only(su.LIMIT_BY_TAG["lim_e32"]))
    b = su.setup(su.cfg_only(su.LIMIT_BY_TAG["lim_e33"]))
    assert (a["E"], b["E"]) == (32, 33)
    a, b = (su.setup(su.cfg_only(su.LIMIT_BY_TAG[t])) for t in ("lim_cap96", "lim_cap100"))
    assert (a["cap"], b["cap"]) == (96, 100)
    a, b = (su.setup(su.cfg_only(su.LIMIT_BY_TAG[t])) for t in ("lim_nr1024", "lim_nr1025"))
    assert (a["nr"], b["nr"]) == (1024, 1025) and a["E"] <= 32
    (f150, o150), (f60, o60) = su.lds_limit_specs()
    a, b = su.setup(su.cfg_only(f150)), su.setup(su.cfg_only(o150))
    assert a["ok"] and not b["ok"] and a["lds"] <= 150 * 1024 < b["lds"] and o150["K"] == f150["K"] + 1
    assert su.vjp_eligible(su.cfg_only(f60)) and not su.vjp_eligible(su.cfg_only(o60)) and su.setup(su.cfg_only(o60))["ok"]
    assert f60["K"] * 25 * 4 <= 60 * 1024 < o60["K"] * 25 * 4 and su.setup(su.cfg_only(f60))["ok"]


# ------------------------------------------------------------------------------------------------ every case is what it claims
@pytest.mark.parametrize("tag", [s["tag"] for s in su.TABLE])
def test_no_query_has_more_live_regions_than_the_restated_capacity(tag):
    c = card(tag)
    s = su.setup(c.cfg)
    assert s["ok"], (tag, s)
    worst = max_live(c.cfg, c.x)
    assert worst <= s["cap"], (tag, worst, s["cap"])
    if tag in ("cap96", "e32_nr87", "repeated_rows", "perm"):
        assert int(c.live().sum(axis=1).max()) == s["cap"] == s["nr"], (tag, worst, s)


def test_repeated_rows_are_live_together():
    """Rows 2 and 4, 1 and 5 of the card name the same ranges: four combinations, six regions; at (0.7, 0.7) every one of them has
    a float32 gamma between 3e-4 and 3e-3."""
    c = card("repeated_rows")
    s = su.setup(c.cfg)
    assert len(set(su.rows_of(c.cfg))) == 4 and (s["cap"], s["nr"]) == (6, 6)
    assert np.allclose(c.x[0, :2], 0.7) and c.live().all()
    g0 = k2.tanh_gate(c.cfg, c.x[:1], np.float32)[0]
    assert ((g0 > 3e-4) & (g0 < 3e-3)).all(), g0
    # per coordinate (2.401 + 2.051) / 3 = 1.484 ranges live on average; squared, times 6 rows / 4 combinations
    assert abs(s["mean"] - 1.484 ** 2 * 1.5) < 0.01


def test_long_lists_and_empty_regions():
    c = card("long_b10000")
    Lr, SL = c.live().sum(axis=0), su.vjp_slices(c.cfg, c.B)
    box = c.spec["box"]
    longest = max(b - a for a, b in su.slice_bounds(int(Lr[box]), SL))
    assert SL == 8 and Lr[box] == c.B and longest == 1250 > 1024 and longest % 64 != 0 and longest > 2 * su.WAVE * su.VP
    assert (Lr == 0).sum() >= 100 and ((Lr > 0) & (Lr < c.B)).sum() >= 3 and any(int(n) % 64 for n in Lr)
    assert any((card(t).live().sum(axis=0) == 0).any() for t in ("nr257", "nr1024_e32"))
    c = card("long_d7_o10_b5000")
    Lr, SL = c.live().sum(axis=0), su.vjp_slices(c.cfg, c.B)
    assert SL == 8 and Lr[c.spec["box"]] == c.B and su.slice_bounds(c.B, SL)[0] == (0, 625) and 625 > su.WAVE * su.VP
    assert c.D == k2.padded_D(c.D) and c.O == k2.padded_O(c.O)           # the whole-row branch of sp_load_row


def test_batch_edges_share_one_net_and_cover_the_search_steps():
    nblk = {B: -(-B // su.NT) for B in (1, 255, 256, 257, 513, 1025)}
    assert nblk == {1: 1, 255: 1, 256: 1, 257: 2, 513: 3, 1025: 5}
    big = card("b1025")
    for B in nblk:
        c = card(f"b{B}")
        assert np.array_equal(c.x, big.x[:B]) and np.array_equal(c.g, big.g[:B])
        assert all(np.array_equal(c.params["params"][a][b], big.params["params"][a][b]) for a, b in k2.LEAF_PATH.values())
    assert big.live().sum(axis=0).min() > 0


def test_the_empty_middle_block():
    c = card("empty_middle")
    h = c.live()[:, 0]
    assert c.B == 3 * su.NT and h[:su.NT].any() and not h[su.NT:2 * su.NT].any() and h[2 * su.NT:].any()
    assert c.live()[su.NT:2 * su.NT].any(axis=0).sum() >= 2               # block 1 is not empty, only row 0's part of it


def test_e32_every_factor_live_and_a_partial_last_word():
    c = card("e32_nr87")
    s = su.setup(c.cfg)
    assert s["E"] == 32 and s["nr"] == 87 and s["nr"] % 32 != 0
    assert all(f[1].all() for f in su._factors(c.cfg, c.x))                # all 32 factors of every query are non-zero
    c = card("nr1024_e32")
    assert su.setup(c.cfg)["E"] == 32 and su.setup(c.cfg)["cap"] == 8 and c.live().sum(axis=1).max() <= 8


def test_margin_neighbours_have_different_hit_sets():
    c = card("margin")
    nb = su.margin_neighbours(c.cfg)
    assert len(nb) == 2 * 2 * 3 and c.n_margin == 2 * len(nb)
    h = c.live()
    for i, (d, dead, alive) in enumerate(nb):
        assert np.nextafter(np.float32(dead), np.float32(alive)) == np.float32(alive)
        assert c.x[2 * i, d] == np.float32(dead) and c.x[2 * i + 1, d] == np.float32(alive)
        a, b = h[2 * i], h[2 * i + 1]
        assert (b & ~a).any() and not (a & ~b).any(), (i, d, dead, alive)  # the neighbour inside has more live regions
    assert h[:c.n_margin].sum(axis=1).max() <= su.setup(c.cfg)["cap"]


def test_region_counts_and_tail_regions():
    for n in (2, 31, 32, 33, 63, 64, 65, 255, 256, 257):
        s = su.setup(card(f"nr{n}").cfg)
        assert s["nr"] == n and s["E"] <= 24
    c = card("nr12_of_16")
    assert c.R == 16 and su.setup(c.cfg)["nr"] == 12 and (c.gamma()[:, 12:] == 0).all()
    ref = c.reference()
    assert (ref["centers"][1][12:] == 0).all() and (ref["centers"][1][:12].max(axis=(1, 2)) > 0).all()


def test_instances_cover_every_shape_the_issue_names():
    inst = [su.cfg_only(s) for s in su.INSTANCES]
    assert {c["in_features"] for c in inst} == set(range(1, 9))
    assert {len(c["activation_idx"]) for c in inst} == set(range(1, 9))
    assert {c["out_features"] for c in inst} == {1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 16}
    assert {c["basis_func"] for c in inst} == set(k2.FAST)
    assert {c["num_kernels"] for c in inst} == {1, 2, 3, 4, 5, 9}
    assert any(len(c["activation_idx"]) < c["in_features"] for c in inst) and any(len(c["activation_idx"]) == c["in_features"] for c in inst)
    assert all(su.vjp_eligible(c) and su.vjp_lds_fits(c) for c in inst)
    assert all(su.setup(su.cfg_only(s))["ok"] and not su.vjp_eligible(su.cfg_only(s)) for s in su.GENERIC)


# ------------------------------------------------------------------------------------------------ the coefficient
def test_yardstick_and_the_coefficient():
    """r32, the worst |err| / S of the float32 restatement (_k2_util.vjp_float32 with the kernels' gamma) over the VJP cases."""
    r32 = 0.0
    for spec in su.VJP_CASES:
        c = card(spec["tag"])
        ref, y = c.reference(), c.yardstick()
        line = []
        for leaf in su.LEAVES:
            assert k2.same_nonfinite(y[leaf], ref[leaf][0]), (c.tag, leaf)
            es, _ = su.ratios(y[leaf], *ref[leaf])
            if es > 5e-5:
                pytest.fail(f"test inputs, not the code under test: {c.tag} {leaf} needs {es:.2e} S in plain float32")
            line.append(f"{leaf} {es:.2e}")
            r32 = max(r32, es)
        print(f"{c.tag:24s} " + "  ".join(line))
    print(f"r32 = {r32:.3e}; R32 = {su.R32:.3e}, C_S = {su.C_S:.3e}")
    assert su.R32 / 2 < r32 <= su.R32, "R32 in _sparse_util.py is not what the yardstick gives"
    assert su.C_S == 4 * su.R32 and su.C_S <= 5e-5
