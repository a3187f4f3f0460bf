"""Helpers of tests/test_k2h_reference_cpu.py and tests/test_gpu_k2h.py: the f16 matrix-core parameter VJP K2h
(`rbf_vjp_f16mfma<DC, BC, 2>` with its pre-pass `vjp_pack_blocks_kernel`, irbfn_amd/csrc/rbf_vjp_f16.hip) on its own.  NumPy only.
Built on tests/_k2_util.py: the cases, the float64 formulas, the gate and the bounds' ratios are that file's.

k2h_plan(...)       vjp_layout's slab cap, vjph_slices, plan_vjp's min(slabs, QSB) and launch_vjp_f16's blocks per wave restated.
CaseH               a single-region k2.Case with the inputs the K2h cases are about (operand ranges, a card without a range row).
reference(case)     k2.vjp_reference in query chunks, the float64 chunks added: the same sums, without [B, N, D] in one piece.
yardstick(case)     the float32 restatement with the queries added one after the other (k2.vjp_float32, in chunks that carry the sum).
yardstick_h(case)   the same with the operands of the two GEMM-shaped pieces as K2h hands them to the matrix cores, restated from
                    the text of f16_split.h: weights over their column's power-of-two scale and cotangents over the batch's as
                    split_static pairs, 2^14 phi as a split_phi pair, the products accumulated as A1 + 2^-11 A2 in float32 without
                    lo x lo.  Its worst |err| / S over TABLE is R_H.

Bounds of tests/test_gpu_k2h.py, on every leaf of every case:
  max|got - ref| <= 5e-5 max|ref| + 1e-7     the project's own, unchanged;
  |got - ref|    <= C_H * S + 1e-30          element-wise, C_H = 4 * R_H (the factor 4 as in tests/_k2_util.py: the kernel's other
                                             summation order and its v_exp_f32); C_H may not exceed 5e-5."""
import numpy as np

import _k2_util as k2
from _k2_util import (LEAVES, LEAF_PATH, Case, _cdiv, basis_and_slope, padded_D, padded_O, ratios, same_nonfinite,  # noqa: F401
                      tanh_gate, vjp_reference)

# worst |err| / S of yardstick_h() over TABLE: 3.30e-7 (h_grows_spread, centers; the plain float32 yardstick of the same table:
# 3.77e-7), recorded as the second two-digit figure above it: 3.297e-7 sits so close under 3.3e-7 that a float32 np.exp which differs
# in the last bit between CPUs could cross it.  tests/test_k2h_reference_cpu.py::test_yardstick_h_and_the_coefficient recomputes it.
R_H = 3.4e-7
C_H = 4 * R_H
CHUNK = 256
K_PHI, K_W, K_LO = np.float32(2.0 ** 14), np.float32(2.0 ** 15), np.float32(2.0 ** 11)


def rfq(DC):
    return 4 if DC <= 3 else 8 if DC <= 7 else 12


def k2h_plan(N, B, D, O, basis):
    """The launch of a K2h call (B >= 2048): blocks of 4 waves x 2 tiles of 16 centres, S query slices of 4 waves; a wave works on
    bpw consecutive 32-query blocks.  S: enough slices for 6144 waves (vjph_slices), at least 4 blocks of queries each, never more
    than the slabs K2's layout allocated (vjp_layout's QSB)."""
    groups = _cdiv(N, 64)
    QSB = min(_cdiv(8192, 4 * groups), _cdiv(B, 256))
    gh, nqb = _cdiv(N, 32), _cdiv(B, 32)
    q = _cdiv(6144, 4 * gh)
    if 4 * q > nqb:
        q = _cdiv(nqb, 4)
    S = min(q, QSB)
    bpw = _cdiv(nqb, 4 * S)
    working = _cdiv(nqb, bpw)
    DC = padded_D(D)
    return {"S": S, "grid": (gh, S), "bpw": bpw, "empty_waves": 4 * S - working, "last_wave_blocks": nqb - (working - 1) * bpw,
            "last_block_queries": B - 32 * (nqb - 1), "nqb": nqb, "QSB": QSB, "q": q, "DC": DC, "OP": padded_O(O), "RFQ": rfq(DC),
            "BC": k2.bclass(basis)}


# ------------------------------------------------------------------------------------------------ f16_split.h in NumPy
def f16_rtz(a):
    """float32 -> float16 rounded toward zero (v_cvt_pkrtz_f16_f32)."""
    a = np.asarray(a, np.float32)
    with np.errstate(over="ignore"):
        h = a.astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(a)
    return np.where(over, np.nextafter(h, np.float16(0)), h)


def split_static(v):
    """split_static_f16: a factor v, |v| <= 1 -> (hi, lo) with 2^15 v = hi + 2^-11 lo; hi rounded to nearest."""
    w = np.asarray(v, np.float32) * K_W
    with np.errstate(over="ignore", invalid="ignore"):
        hi = w.astype(np.float16)
        lo = ((w - hi.astype(np.float32)) * K_LO).astype(np.float16)
    return hi, lo


def split_cotangent(v):
    """split_cotangent_f16: split_static for the finite elements (the batch scale is taken from them alone) and for NaN, which
    becomes (NaN, NaN); +-Inf becomes (+-65504, +-Inf), so that A1 stays finite and A2 carries the infinity with the product's sign."""
    v = np.asarray(v, np.float32)
    hi, lo = split_static(v)
    inf = np.isinf(v)
    return np.where(inf, np.copysign(np.float16(65504), v).astype(np.float16), hi), np.where(inf, v.astype(np.float16), lo)


def split_phi(P):
    """split_pair_f16<3>: P = 2^14 phi >= 0 -> hi = its top 11 bits, lo = 2^11 (P - hi), both converted toward zero."""
    P = np.ascontiguousarray(P, np.float32)
    h = (P.view(np.uint32) & np.uint32(0xFFFFE000)).view(np.float32)
    return f16_rtz(h), f16_rtz((P - h) * K_LO)


def pow2_above(mx):
    """The power of two above mx (frexp: mx = f 2^e, f in [0.5, 1) -> 2^e); 1 for zero."""
    mx = np.asarray(mx, np.float32)
    _, e = np.frexp(mx)
    return np.where(mx > 0, np.ldexp(np.float32(1), e), np.float32(1)).astype(np.float32)


def pair_product(ah, al, bh, bl):
    """A1 + 2^-11 A2 of the pairs a [m, k], b [k, n] in float32: A1 = ah bh, A2 = al bh + ah bl (f16 x f16 is exact in float32)."""
    f = np.float32
    ah, al, bh, bl = (np.asarray(t, f) for t in (ah, al, bh, bl))
    return (ah @ bh + (al @ bh + ah @ bl) / K_LO).astype(f)


# ------------------------------------------------------------------------------------------------ the cases
class CaseH(Case):
    """A k2.Case of kind "one" (a single region) plus, by key of the spec:
    norange      the card has no row in dimension_ranges: the region's weight is 0 for every query;
    wcols        the weight columns scaled by powers of two spaced over 2^-10 .. 2^10, the cotangent non-zero in the smallest alone
                 (|g| >= 2^-6 there and in `grows`: no operand below 2^-29 of its scale, the documented range of a pair);
    grows        the cotangent rows scaled by powers of two spaced over 2^-10 .. 2^10;
    zero_col     weight column 1 is zero;  zero_kernel: every weight;  zero_g: every cotangent;
    outside      every third query's first (gated) coordinate 1e3 above the box."""

    def __init__(self, spec):
        super().__init__(spec)
        assert self.kind == "one" and self.R == 1
        W = self.params["params"]["linear"]["kernel"]
        if spec.get("norange"):
            self.cfg["dimension_ranges"] = []
        if spec.get("wcols"):
            e = np.round(np.linspace(-10, 10, self.O)).astype(int)
            W *= np.ldexp(np.float32(1), e)[None, :]
            self.g[:] = np.copysign(np.maximum(np.abs(self.g), np.float32(2.0 ** -6)), self.g)      # 2^-20 g / s_g >= 2^-29
            self.g[:, 1:] = 0.0
        if spec.get("grows"):
            e = np.round(np.linspace(-10, 10, self.B)).astype(int)
            self.g[:] = np.copysign(np.maximum(np.abs(self.g), np.float32(2.0 ** -6)), self.g)      # every |g| >= 2^-29 s_g
            self.g *= np.ldexp(np.float32(1), np.random.default_rng(self.B).permutation(e))[:, None]
        if spec.get("zero_col"):
            W[:, 1] = 0.0
        if spec.get("zero_kernel"):
            W[:] = 0.0
        if spec.get("zero_g"):
            self.g[:] = 0.0
        if spec.get("outside"):
            assert self.ns >= 1
            self.x[::3, 0] += np.float32(1.0e3)

    def plan(self):
        return k2h_plan(self.N, self.B, self.D, self.O, self.basis)

    def reference(self):
        return reference(self)

    def yardstick(self):
        return yardstick(self)

    def yardstick_h(self):
        return yardstick(self, split=True)


def reference(case, chunk=CHUNK):
    """k2.vjp_reference over query chunks -> {leaf: (grad, S)}; float64 sums of the chunks."""
    gamma = case.gamma()
    acc = None
    for a in range(0, case.B, chunk):
        part = vjp_reference(case.basis, case.params, case.x[a:a + chunk], case.g[a:a + chunk], gamma[a:a + chunk])
        acc = part if acc is None else {leaf: (acc[leaf][0] + part[leaf][0], acc[leaf][1] + part[leaf][1]) for leaf in LEAVES}
    return acc


def yardstick(case, split=False, chunk=CHUNK):
    """The four formulas in float32, every sum over the queries sequential (np.cumsum, the chunks carry it) -> {leaf: grad}.
    split: hbar = g W^T and d kernel = (gamma phi)^T g through the (hi, lo) pairs of f16_split.h --
      hbar      (g[q,o] s_o / s_h) x (W[k,o] / s_o)           s_o = pow2_above(max_k |W[k,o]|), s_g = pow2_above(max FINITE |g|),
      d kernel  (gamma_q g[q,o] / s_g) x (2^14 phi[q,k])      s_h = s_g max_o s_o
    -- the weights by split_static, the cotangents by split_cotangent, 2^14 phi by split_phi, A1 + 2^-11 A2 in float32.  Everything else as in the plain one."""
    f = np.float32
    p = case.params["params"]
    c, ls, W = (np.asarray(p[a][b], f) for a, b in (LEAF_PATH["centers"], LEAF_PATH["log_sigs"], LEAF_PATH["kernel"]))
    assert c.shape[0] == 1
    gamma = case.gamma(f)
    K, D, O = case.K, case.D, case.O
    s2 = np.exp(-2 * ls)[None]
    with np.errstate(all="ignore"):
        if split:
            so = pow2_above(np.abs(W).max(axis=0))
            fin = np.abs(case.g)[np.isfinite(case.g)]
            sg = pow2_above(fin.max() if fin.size else f(0))
            sh = f(sg * so.max())
            wh, wl = split_static(W / so[None, :])
        tot = {"centers": np.zeros((1, 1, K, D), f), "log_sigs": np.zeros((1, 1, K), f), "bias": np.zeros((1, O), f)}
        kern = np.zeros((K, O), f) if not split else None
        A1, A2 = (np.zeros((1, K, O), f), np.zeros((1, K, O), f)) if split else (None, None)
        seq = lambda carry, a: np.cumsum(np.concatenate([carry, a]), axis=0, dtype=f)[-1:]
        for a in range(0, case.B, chunk):
            x, g, gm = case.x[a:a + chunk], case.g[a:a + chunk], gamma[a:a + chunk]
            diff = x[:, None, None, :] - c[None]
            r2 = (diff * diff).sum(-1)
            d2 = r2 * s2
            phi, dphi = basis_and_slope(case.basis, d2)
            if split:
                gh, gl = split_cotangent(g * (so / sh)[None, :])
                hbar = pair_product(gh, gl, wh.T, wl.T) * f(sh / (K_W * K_W))
            else:
                hbar = g @ W.T
            t = hbar[:, None, :] * gm[:, :, None] * dphi
            tot["centers"] = seq(tot["centers"], (t * s2)[..., None] * -2 * diff)
            tot["log_sigs"] = seq(tot["log_sigs"], t * (-2 * d2))
            tot["bias"] = seq(tot["bias"], g)
            if split:
                th, tl = split_cotangent(gm[:, :1] * g / sg)                   # [b, O]
                ph, pl = split_phi(phi[:, 0, :] * K_PHI)                     # [b, K]
                th, tl, ph, pl = (t_.astype(f) for t_ in (th, tl, ph, pl))
                A1 = seq(A1, ph[:, :, None] * th[:, None, :])
                A2 = seq(A2, pl[:, :, None] * th[:, None, :] + ph[:, :, None] * tl[:, None, :])
            else:
                h = gm[:, :, None] * phi                                     # [b, 1, K]
                kern = seq(kern[None], h[:, 0, :, None] * g[:, None, :])[0]
        if split:
            kern = ((A1[0] + A2[0] / K_LO) * f(sg / (K_PHI * K_W))).astype(f)
    out = {"centers": tot["centers"][0], "log_sigs": tot["log_sigs"][0], "kernel": kern, "bias": tot["bias"][0]}
    assert all(v.dtype == f for v in out.values())
    return out


_one = k2._one
B0 = 2048
# Every D from 1 to 8 (DC = 3, 3, 3, 4, 7, 7, 7, 8; RFQ = 4, 4, 4, 8, 8, 8, 8, 12), O at both ends of the compiled paddings
# 2, 4, 5, 8, 10, 16, centre counts around the 16-centre tile, the 32-centre block and the 64-centre group, the five eligible
# bases, no / some / all coordinates gated.  The ragged tails leave the last block 1, 5, 13, ... queries.
SHAPES = [
    _one("h_d1_o1_n1", 1, 1, 1, "gaussian", B0 + 1, ns=1),
    _one("h_d2_o2_n15", 2, 2, 15, "inverse_quadratic", B0 + 5, ns=1),
    _one("h_d3_o3_n16", 3, 3, 16, "inverse_multiquadric", B0 + 13),
    _one("h_d4_o4_n17", 4, 4, 17, "gaussian_wide", B0 + 31, ns=4),
    _one("h_d5_o5_n31", 5, 5, 31, "gaussian_wider", B0 + 33, ns=2),
    _one("h_d6_o6_n32", 6, 6, 32, "gaussian", B0 + 47),
    _one("h_d7_o8_n33", 7, 8, 33, "inverse_quadratic", B0 + 63, ns=7),
    _one("h_d8_o9_n63", 8, 9, 63, "inverse_multiquadric", B0 + 64, ns=3),
    _one("h_d3_o10_n64", 3, 10, 64, "gaussian_wide", B0 + 65, ns=3),
    _one("h_d4_o11_n65", 4, 11, 65, "inverse_quadratic", B0 + 17),
    _one("h_d8_o16_n130", 8, 16, 130, "gaussian", B0 + 29, ns=1),
    _one("h_d7_o5_n130", 7, 5, 130, "inverse_multiquadric", B0 + 2, ns=2),
]
NORANGE = [_one("h_norange", 4, 5, 40, "gaussian_wide", B0 + 9, ns=2, norange=True)]
BATCH_EDGES = (2048, 2049, 2079, 2080, 2081, 2304, 2305, 4097)
BATCH = [_one(f"h_b{B}", 3, 5, 100, "gaussian", B, net="h_batch", draw=4097) for B in BATCH_EDGES]
BIG_EDGES = (4352, 4353)
BIG = [_one(f"h_n3072_b{B}", 3, 5, 3072, "gaussian_wide", B, net="h_big", draw=4353) for B in BIG_EDGES]
REUSE = [_one("h_reuse_b2049", 4, 10, 150, "gaussian", 2049, net="h_reuse", draw=4352)]
RANGES = [
    _one("h_wcols_spread", 5, 8, 70, "gaussian_wide", B0 + 11, ns=1, wcols=True),
    _one("h_grows_spread", 5, 8, 70, "inverse_quadratic", B0 + 11, grows=True),
    _one("h_zero_col", 3, 4, 40, "gaussian", B0 + 3, zero_col=True),
    _one("h_zero_kernel", 3, 4, 40, "inverse_multiquadric", B0 + 3, zero_kernel=True),
    _one("h_zero_g", 4, 5, 40, "gaussian_wide", B0 + 3, ns=1, zero_g=True),
    _one("h_on_centres", 3, 5, 40, "inverse_quadratic", B0 + 7, ns=1, on_centres=True),
    _one("h_outside", 4, 3, 50, "inverse_quadratic", B0 + 21, ns=2, outside=True),
]
SCALING = [_one("h_scale_d3", 3, 5, 100, "gaussian_wide", B0 + 19, ns=1), _one("h_scale_d8", 8, 16, 70, "inverse_quadratic", B0 + 40)]
NONFINITE = [_one(f"h_nonfinite_{p}", 5, 3, 70, "gaussian_wide", B0 + 27, ns=2, net="h_nonfinite", poison=p)
             for p in ("nan_g", "inf_g", "nan_x")]
TABLE = SHAPES + NORANGE + BATCH + BIG + REUSE + RANGES + SCALING + NONFINITE
BY_TAG = {s["tag"]: s for s in TABLE}


def ratios_h(got, ref, S):
    """k2.ratios with the absolute term of the element-wise bound read against C_H: (worst |err| / S, max-norm ratio)."""
    fin = np.isfinite(ref)
    if not fin.any():
        return 0.0, 0.0
    err = np.abs(np.asarray(got, np.float64)[fin] - ref[fin])
    if not np.isfinite(err).all():
        return float("inf"), float("inf")
    return (float((err / (S[fin] + k2.ATOL_S / C_H)).max()),
            float(err.max() / (k2.MAXNORM_REL * np.abs(ref[fin]).max() + k2.MAXNORM_ABS)))
