"""Helpers of tests/test_k2g_reference_cpu.py and tests/test_gpu_k2g.py: the Gram-expansion parameter VJP K2g
(`rbf_vjp_f16gram<DC, BC, OC, MODE>` with its pre-pass `vjp_pack_blocks_gram_kernel`, irbfn_amd/csrc/rbf_vjp_gram.hip) on its own.
NumPy only.  Built on tests/_k2_util.py and tests/_k2h_util.py: the cases, the float64 formulas, the gate, the chunked reference, the
(hi, lo) splits and K2h's launch rules are those files'.

k2g_plan(...)        vjp_layout's slab cap, vjpg_slices, plan_vjp's min(slices, QSB) and launch_vjp_gram_mode's blocks per slice.
header(c)            the origin and the exponent of the expansion's box as gram_header (pack_all.hip) takes them from the centres:
                     a query is representable where |x_i - r_i| < 0.999 * 2^ex in every coordinate (gram_query_parts).
CaseG                a kh.CaseH plus the case whose queries lie 6 - 8 widths from every centre (`far`).
yardstick_g(case)    the float32 restatement of kh.yardstick with the operands of ALL four GEMM-shaped pieces as K2g hands them to
                     the matrix cores (restated from the text of rbf_vjp_gram.hip):
                       hbar      (gamma_q g[q,o] s_o / s_h 2^-expA) x (W[k,o] / s_o 2^-expB) as split_static pairs; O <= 10: the
                                 three products hi x hi + (2^-5 lo) x (2^-6 hi) + (2^-5 hi) x (2^-6 lo) in one sum, the scaled
                                 copies rounded to f16; else hi x hi + 2^-11 (lo x hi + hi x lo); then 2^-(ET - expA - expB)
                       P, tts    P = PS phi (PS = 1, 2^14, 2^7) and tts = hb P^p through split_pair_plain: hi converted toward
                                 zero, lo = P - hi converted toward zero as it is (no gain)
                       g, x'     gamma_q g / s_g and (x - r) 2^-ex, with a column of ones, as split_static pairs (2^11 on lo)
                       d centers -2 / sigma^2 KT (dC xs - c' stt),  d log_sigs -2 / sigma^2 KT sum tts v / scale
                     The distances stay plain float32: the expansion claims to cancel exactly.
floor(case)          A, the absolute floor K2g documents, in float64 from the inputs alone (below).

Bounds of tests/test_gpu_k2g.py, on every leaf of every case:
  max|got - ref| <= 5e-5 max|ref| + 1e-7     the project's own, unchanged;
  |got - ref|    <= C_G * S + A + 1e-30      element-wise, C_G = 4 * R_G, R_G the worst (|err| - A)+ / S of yardstick_g over TABLE
                                             (the factor 4 as in tests/_k2_util.py); C_G may not exceed 5e-5.

The floor A.  rbf_vjp_gram.hip documents three absolute accuracies; each becomes a term, the sums over the queries of the batch:
  (1) split_pair_plain: "lo < 2^-10 |p| falls into the f16 subnormals for |p| < 2^-4 and is then good to 2^-25 ABSOLUTE only".
      Both conversions go toward zero on the subnormal grid of 2^-24, so a value is short by less than 2^-24.  P = PS phi is the
      operand of d kernel:  A[kernel][k,o] = 2^-24 / PS * sum_q gamma_q |g[q,o]|   (PS = 1 for the gaussians, whose basis value is
      taken as phi itself; 2^14 for the inverse quadratic, 2^7 for the inverse multiquadric: 2^-14 resp. 2^-7 of the gaussians').
  (2) hbar's operands: "a (hi, lo) pair then keeps 2^-36 ABSOLUTE against operands of size 2^-2": lo = 2^11 (w - hi) lies on the
      grid of 2^-24 once w is below 2^-14, half a step of it is 2^-36 of the operand.  For O <= 10 the cross terms' operands are
      copies scaled by 2^-5 (cotangent side) and 2^-6 (weight side) and rounded to f16 again: half a step of 2^-24 on a copy that
      stands for 2^-6 resp. 2^-5 of its value is 2^-31 resp. 2^-30 of the operand; EPS_OC = 2^-30 is taken for both sides.
      With a = 2^15 gamma g s_o / s_h 2^-expA and b = 2^15 W / s_o 2^-expB the product's error in units of hbar is
          eh[q,k] = eps * sum_o ( gamma_q |g[q,o]| s_o 2^(expB - 15)  +  [gamma_q g[q,o] != 0] |W[k,o]| s_h / s_o 2^(expA - 15) )
      (a zero operand is exact).  The second term is relative to s_h, the power of two above the largest |g[q,o]| s_o of the batch:
      see RANGE_NOTE for what it was.
  (3) carried through tt = gamma hbar dphi/dd2:  A[centers][k,i] = sum_q eh |dphi| 2 / sigma^2 |x_i - c_ki|,
      A[log_sigs][k] = sum_q eh |dphi| 2 d2;  and tts itself goes through split_pair_plain into the dC products, short by less than
      2^-24 of tts = tt / KT:  A[centers][k,i] += 2^-24 |KT| 2 / sigma^2 sum_q [gamma_q != 0] (|x'_qi| + |c'_ki|).  d log_sigs is
      summed on the VALU from tts in float32 and has no such term.
  A[bias] = 0."""
import numpy as np

import _k2_util as k2
import _k2h_util as kh
from _k2_util import LEAVES, LEAF_PATH, _cdiv, padded_D, padded_O, same_nonfinite  # noqa: F401
from _k2h_util import CHUNK, f16_rtz, pow2_above, split_static

F = np.float32
LOG2E = F(1.4426950408889634)
EPS_PAIR, EPS_OC = 2.0 ** -36, 2.0 ** -30
OC_MAX = 10                                   # kVgOC: up to this many outputs hbar is ONE 16x16x32 MFMA


# ------------------------------------------------------------------------------------------------ the launch
def basis_consts(basis):
    """(BC, expA, expB, ET, PS, a) of a basis: vg_exp_a / vg_exp_b, ET and PS of vg_body; a = the gaussian's gscale."""
    bc = k2.bclass(basis)
    return (bc, 9 if bc == 0 else 16, 10 if bc == 0 else 17, (19, 47, 40)[bc], (1.0, 2.0 ** 14, 2.0 ** 7)[bc], k2.GAUSS_A.get(basis, 0.0))


def k2g_plan(N, B, D, O, basis, mode=0):
    """The launch of a K2g call (B >= 2048): blocks of 4 waves = 4 chunks of 32 centres, S query slices of bpb 32-query blocks that
    the 4 waves walk together through a ring of three LDS slots.  S: one resident round of blocks (vjpg_slices), at least 8 query
    blocks a slice, never more than the slabs K2's layout allocated (vjp_layout's QSB).  mode: 0 all leaves, 1 no centres, 2 linear."""
    OC = O <= OC_MAX
    waves = {0: 4 if OC else 3, 1: 5 if OC else 4, 2: 6}[mode]              # vg_waves
    nqb = _cdiv(B, 32)
    QSB = min(_cdiv(8192, 4 * _cdiv(N, 64)), _cdiv(B, 256))
    nchunks = _cdiv(N, 32)
    gb = _cdiv(nchunks, 4)
    resident = (1024 if OC else 768) if mode == 0 else 256 * waves
    q = min(_cdiv(resident, gb), 64)
    if 8 * q > nqb:
        q = _cdiv(nqb, 8)
    S = min(max(q, 1), QSB)
    bpb = _cdiv(nqb, S)
    working = _cdiv(nqb, bpb)
    return {"S": S, "bpb": bpb, "grid": (gb, S), "nqb": nqb, "QSB": QSB, "q": q, "gb": gb, "nchunks": nchunks,
            "idle_waves": 4 * gb - nchunks, "working": working, "empty": S - working, "last_slice_blocks": nqb - (working - 1) * bpb,
            "last_block_queries": B - 32 * (nqb - 1), "OC": OC, "DC": padded_D(D), "OP": padded_O(O), "BC": k2.bclass(basis),
            "bias_blocks": _cdiv(B, 64) if B < 16384 else 256, "pieces": {0: 12, 1: 10, 2: 7}[mode]}


def header(c):
    """gram_header (pack_all.hip) for centres c[K, D] -> (r, ex, hwm): the origin is the midpoint of the centres' box, hwm its largest
    half width, and |x'_i| < 2^ex with 2^ex above 1.25 hwm.  hwm = 0 (one centre): the pack's verdict is `does not fit`."""
    c = np.asarray(c, F)
    mx, mn = c.max(axis=0), (-c).max(axis=0)
    r = (F(0.5) * mx - F(0.5) * mn).astype(F)
    hw = (np.maximum(mx - r, r + mn) * F(1.0000005)).astype(F)
    hwm = float(hw.max())
    ex = int(np.frexp(1.25 * hwm * 1.0000002)[1]) if hwm > 0 else -40
    return r, ex, hwm


def box_limit(c):
    """(r, lim): a query is inside the expansion's box where |fl(x_i - r_i)| < lim in every coordinate (xlim of gram_query_parts)."""
    r, ex, _ = header(c)
    return r, F(np.ldexp(F(1), ex) * F(0.999))


def split_plain(p):
    """split_pair_plain: hi = p converted toward zero, lo = p - hi (exact) converted toward zero as it is."""
    p = np.asarray(p, F)
    hi = f16_rtz(p)
    return hi, f16_rtz(p - hi.astype(F))


# ------------------------------------------------------------------------------------------------ the cases
class CaseG(kh.CaseH):
    """A kh.CaseH plus, by key of the spec:
    wider    added to every log_sig (a case redrawn with wider widths: the condition on A of tests/test_k2g_reference_cpu.py);
    wspread  s: kh.CaseH's `wcols` with the weight columns over 2^-s .. 2^s instead of 2^-10 .. 2^10 (the sweep of the CPU test);
    far      the centres in two small clusters at opposite corners of their cube, one width for all, every query near the midpoint:
             6 - 8 widths from EVERY centre and well inside the box.  The gaussian's phi lies between e^-64 and e^-36, far below the
             2^-24 an ungained pair resolves: d kernel and d centers come out as the floor allows, d log_sigs in float32."""

    def __init__(self, spec):
        super().__init__(spec)
        rl = self.params["params"]["rbf_list"]
        if spec.get("wider"):
            rl["log_sigs"] += F(spec["wider"])
        if spec.get("wspread") is not None:
            e = np.round(np.linspace(-spec["wspread"], spec["wspread"], self.O)).astype(int)
            self.params["params"]["linear"]["kernel"] *= np.ldexp(F(1), e)[None, :]
            self.g[:] = np.copysign(np.maximum(np.abs(self.g), F(2.0 ** -6)), self.g)
            self.g[:, 1:] = 0.0
        if spec.get("far"):
            rng = np.random.default_rng(self.K)
            corner = np.where(np.arange(self.K)[:, None] % 2 == 0, -1.0, 1.6)
            rl["centers"][0] = (corner + np.sign(-corner) * rng.uniform(0, 0.1, size=(self.K, self.D))).astype(F)
            self.x[:] = (0.3 + rng.uniform(-0.08, 0.08, size=self.x.shape)).astype(F)
            rl["log_sigs"][:] = F(np.log(1.25 * np.sqrt(self.D) / 7.0))               # about the distance midpoint - cluster, over 7

    def plan(self, mode=0):
        return k2g_plan(self.N, self.B, self.D, self.O, self.basis, mode)

    def yardstick_g(self):
        return yardstick_g(self)

    def floor(self):
        return floor(self)


def _operand_scales(case, W):
    """(s_o[O], s_g, s_h): the weight columns' powers of two, the power of two above the largest finite |g| and hbar's scale, the
    power of two above the largest finite |g[q,o]| s_o (before_fix: s_g max_o s_o, RANGE_NOTE)."""
    so = pow2_above(np.abs(W).max(axis=0))
    fin = np.abs(case.g)[np.isfinite(case.g)]
    sg = pow2_above(fin.max() if fin.size else F(0))
    if getattr(case, "before_fix", False):
        return so, F(sg), F(sg * so.max())
    with np.errstate(all="ignore"):
        v = np.abs(case.g * so[None, :])
    v = v[np.isfinite(case.g)]
    return so, F(sg), F(pow2_above(v.max() if v.size else F(0)))


def yardstick_g(case, chunk=CHUNK):
    """The four formulas in float32 with K2g's operand treatment (module docstring) -> {leaf: grad}; every sum over the queries
    sequential, the chunks carry it."""
    f = F
    p = case.params["params"]
    c, ls, W = (np.asarray(p[a][b], f) for a, b in (LEAF_PATH["centers"], LEAF_PATH["log_sigs"], LEAF_PATH["kernel"]))
    assert c.shape[0] == 1
    c, ls = c[0], ls[0]
    K, D, O = case.K, case.D, case.O
    bc, expA, expB, ET, PS, ag = basis_consts(case.basis)
    PS, OC = f(PS), O <= OC_MAX
    r, ex, hwm = header(c)
    assert hwm > 0, "one centre: K2g refuses the net, there is nothing to restate"
    gamma = case.gamma(f)[:, 0]
    s2 = np.exp(-2 * ls).astype(f)                                   # [K] 1 / sigma^2
    so, sg, sh = _operand_scales(case, W)
    seq = lambda carry, a: np.cumsum(np.concatenate([carry, a]), axis=0, dtype=f)[-1:]
    h16 = lambda a: np.asarray(a, f).astype(np.float16).astype(f)
    with np.errstate(all="ignore"):
        wh, wl = (t.astype(f) for t in split_static((W / so[None, :]) * f(2.0 ** -expB)))              # [K, O]
        if OC:
            wx_h, wx_l = h16(wh * f(2.0 ** -6)), h16(wl * f(2.0 ** -6))
        cE = f(2.0 ** -(ET - expA - expB))
        const = f(-ag) / PS if bc == 0 else (f(-1) / (PS * PS) if bc == 1 else f(-0.5) / (PS * PS * PS))
        KT = f(f(sh * f(2.0 ** -30)) * f(2.0 ** ET) * const)
        alpha = (f(-ag) * LOG2E * s2).astype(f)                      # the gaussian's record scale
        gls = np.zeros((1, K), f)
        dW, dW2, dWl = (np.zeros((1, K, O), f) for _ in range(3))
        dC, dC2, dCl = (np.zeros((1, K, D + 1), f) for _ in range(3))
        bias = np.zeros((1, O), f)
        for a0 in range(0, case.B, chunk):
            x, g, gm = case.x[a0:a0 + chunk], case.g[a0:a0 + chunk], gamma[a0:a0 + chunk]
            ah, al = (t.astype(f) for t in split_static(gm[:, None] * g * (so / sh)[None, :] * f(2.0 ** -expA)))
            if OC:
                hb = ah @ wh.T + h16(al * f(2.0 ** -5)) @ wx_h.T + h16(ah * f(2.0 ** -5)) @ wx_l.T
            else:
                hb = (al @ wh.T + ah @ wl.T) * f(2.0 ** -11) + ah @ wh.T
            hb = (hb * cE).astype(f)                                 # [b, K]
            diff = x[:, None, :] - c[None]
            r2 = (diff * diff).sum(-1)
            if bc == 0:
                v = r2 * alpha[None]
                P = np.exp2(v)
                pw = P
            else:
                v = r2 * s2[None]
                P = PS / (1 + v) if bc == 1 else PS / np.sqrt(1 + v)
                pw = P * P if bc == 1 else P * P * P
            tts = (hb * pw).astype(f)
            gls = seq(gls, tts * v)
            th, tl = (t.astype(f) for t in split_static(gm[:, None] * g / sg))                        # [b, O]
            ph, pl = (t.astype(f) for t in split_plain(P))                                            # [b, K]
            dW = seq(dW, ph[:, :, None] * th[:, None, :])
            dW2 = seq(dW2, pl[:, :, None] * th[:, None, :])
            dWl = seq(dWl, ph[:, :, None] * tl[:, None, :])
            xp = np.concatenate([(x - r[None]) * f(2.0 ** -ex), np.ones((x.shape[0], 1), f)], axis=1)
            xh, xl = (t.astype(f) for t in split_static(xp))                                          # [b, D + 1]
            sh_, sl_ = (t.astype(f) for t in split_plain(tts))
            dC = seq(dC, sh_[:, :, None] * xh[:, None, :])
            dC2 = seq(dC2, sl_[:, :, None] * xh[:, None, :])
            dCl = seq(dCl, sh_[:, :, None] * xl[:, None, :])
            bias = seq(bias, g)
        kern = ((dWl[0] * f(2.0 ** -11) + (dW[0] + dW2[0])) * f(sg / (PS * kh.K_W))).astype(f)
        dv = (dCl[0] * f(2.0 ** -11) + (dC[0] + dC2[0])).astype(f)
        st = dv[:, D] * f(2.0 ** -15)
        cen = (f(-2) * s2[:, None] * KT * (dv[:, :D] * f(2.0 ** (ex - 15)) - (c - r[None]) * st[:, None])).astype(f)
        lsg = (f(-2) * s2 * KT * gls[0] / (alpha if bc == 0 else s2)).astype(f)
    out = {"centers": cen[None], "log_sigs": lsg[None], "kernel": kern, "bias": bias[0]}
    assert all(v_.dtype == f for v_ in out.values())
    return out


def floor(case, chunk=CHUNK):
    """A of the module docstring -> {leaf: float64 array}."""
    p = case.params["params"]
    c, ls, W = (np.asarray(p[a][b], np.float64) for a, b in (LEAF_PATH["centers"], LEAF_PATH["log_sigs"], LEAF_PATH["kernel"]))
    c, ls = c[0], ls[0]
    K, D, O = case.K, case.D, case.O
    bc, expA, expB, ET, PS, ag = basis_consts(case.basis)
    eps = EPS_OC if O <= OC_MAX else EPS_PAIR
    r, ex, hwm = header(c)
    r = r.astype(np.float64)
    so, sg, sh = (np.asarray(t, np.float64) for t in _operand_scales(case, np.asarray(W, F)))
    const = ag / PS if bc == 0 else (1 / PS ** 2 if bc == 1 else 0.5 / PS ** 3)
    KT = float(sh) * 2.0 ** (ET - 30) * const
    s2 = np.exp(-2 * ls)
    gamma = case.gamma()[:, 0]
    A = {"centers": np.zeros((1, K, D)), "log_sigs": np.zeros((1, K)), "kernel": np.zeros((K, O)), "bias": np.zeros(O)}
    with np.errstate(all="ignore"):
        wterm = np.abs(W) * (float(sh) / so)[None, :] * 2.0 ** (expA - 15)                   # [K, O]
        for a0 in range(0, case.B, chunk):
            x, gm = case.x[a0:a0 + chunk].astype(np.float64), gamma[a0:a0 + chunk]
            g = np.nan_to_num(case.g[a0:a0 + chunk].astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0)
            gg = gm[:, None] * np.abs(g)                                                      # [b, O]
            eh = eps * ((gg * so[None, :]).sum(1)[:, None] * 2.0 ** (expB - 15) + (gg != 0).astype(np.float64) @ wterm.T)
            diff = x[:, None, :] - c[None]
            d2 = (diff * diff).sum(-1) * s2[None]
            _, dphi = k2.basis_and_slope(case.basis, d2)
            t = eh * np.abs(dphi)                                                             # [b, K]
            A["centers"][0] += np.nan_to_num(((t * s2[None])[..., None] * 2 * np.abs(diff)).sum(0))
            A["log_sigs"][0] += np.nan_to_num((t * 2 * d2).sum(0))
            live = (gm != 0).astype(np.float64)
            A["centers"][0] += 2.0 ** -24 * abs(KT) * 2 * s2[:, None] * ((live[:, None] * np.abs(np.nan_to_num(x - r[None]))).sum(0)[None, :] +
                                                                         live.sum() * np.abs(c - r[None]))
            A["kernel"] += (2.0 ** -24 / PS) * gg.sum(0)[None, :]
    return A


# ------------------------------------------------------------------------------------------------ the table
_one = k2._one
B0 = 2048
# Every D from 1 to 8 (DC = 3, 3, 3, 4, 7, 7, 7, 8), O in {1, 2, 5, 9, 10, 11, 15, 16} (hbar as one MFMA up to 10, as two from 11),
# centre counts around the 16-centre tile, the 32-centre chunk and the 128-centre block (N = 15: one tile and three idle waves;
# 33: a second wave with one centre; 97, 127: a ragged fourth wave; 129, 130: a second block with three idle waves), the five
# eligible bases, no / some / all coordinates gated.  N = 1 is ONE_CENTRE: a single centre has no box (header: hwm = 0), the
# pack's verdict rejects it and K2g refuses the net -- tests/test_gpu_k2g.py asserts the refusal instead of a result.
# g_d8_o16_n97 is drawn with widths wider by 0.5: as drawn, A reached C_G S on a third of d kernel's elements.
SHAPES = [
    _one("g_d1_o1_n15", 1, 1, 15, "gaussian", B0 + 1, ns=1),
    _one("g_d2_o2_n16", 2, 2, 16, "inverse_quadratic", B0 + 5, ns=1),
    _one("g_d3_o11_n17", 3, 11, 17, "inverse_multiquadric", B0 + 13),
    _one("g_d4_o5_n31", 4, 5, 31, "gaussian_wide", B0 + 31, ns=4),
    _one("g_d5_o9_n32", 5, 9, 32, "gaussian_wider", B0 + 33, ns=2),
    _one("g_d6_o15_n33", 6, 15, 33, "inverse_quadratic", B0 + 47),
    _one("g_d7_o10_n96", 7, 10, 96, "inverse_multiquadric", B0 + 63, ns=7),
    _one("g_d8_o16_n97", 8, 16, 97, "gaussian", B0 + 64, ns=3, wider=0.5),
    _one("g_d8_o10_n127", 8, 10, 127, "inverse_quadratic", B0 + 65),
    _one("g_d4_o11_n128", 4, 11, 128, "inverse_quadratic", B0 + 17, ns=1),
    _one("g_d4_o2_n129", 4, 2, 129, "inverse_multiquadric", B0 + 29, ns=2),
    _one("g_d8_o15_n130", 8, 15, 130, "inverse_multiquadric", B0 + 2, ns=8),
]
ONE_CENTRE = _one("g_d1_o1_n1", 1, 1, 1, "gaussian", B0 + 1, ns=1)
NORANGE = [_one("g_norange", 4, 11, 40, "gaussian_wide", B0 + 9, ns=2, norange=True)]
BATCH_EDGES = (2048, 2049, 2080, 2081, 2113, 2145, 2305, 16384, 16385)
BATCH = [_one(f"g_b{B}", 3, 5, 100, "gaussian", B, net="g_batch", draw=16385) for B in BATCH_EDGES]
FROZEN_EDGES = (2049, 2145)
LARGE = [_one(f"g_n2049_o{O}", 3, O, 2049, "inverse_quadratic", 11777, net=f"g_large_o{O}") for O in (10, 11)]
REUSE = [_one("g_reuse_b2049", 5, 11, 150, "gaussian", 2049, net="g_reuse", draw=4352)]
RANGES = [
    _one("g_wcols_gauss", 8, 8, 70, "gaussian_wide", B0 + 11, ns=1, wcols=True),
    _one("g_wcols_iq", 4, 8, 70, "inverse_quadratic", B0 + 11, ns=1, wcols=True),
    _one("g_wcols_imq", 3, 8, 70, "inverse_multiquadric", B0 + 11, ns=1, wcols=True),
    _one("g_grows_spread", 5, 16, 70, "inverse_multiquadric", B0 + 11, grows=True),
    _one("g_zero_col", 6, 4, 40, "inverse_quadratic", B0 + 3, zero_col=True),
    _one("g_zero_kernel", 4, 12, 40, "inverse_multiquadric", B0 + 3, zero_kernel=True),
    _one("g_zero_g", 8, 11, 40, "inverse_quadratic", B0 + 3, ns=1, zero_g=True),
    _one("g_on_centres", 8, 5, 40, "inverse_multiquadric", B0 + 7, ns=1, on_centres=True),
    _one("g_far", 3, 11, 40, "gaussian", B0 + 7, ns=1, far=True),
]
SCALING = [_one("g_scale_d3", 3, 5, 100, "gaussian_wide", B0 + 19, ns=1), _one("g_scale_d8", 8, 16, 70, "inverse_quadratic", B0 + 40)]
# the base of the hand-over cases (tests/test_gpu_k2g.py changes single rows of x and g): B = 2049, the last block holds one query;
# coordinates 0 and 1 gated, 2 and 3 not
HANDOVER = [_one("g_hand", 4, 3, 50, "inverse_quadratic", B0 + 1, ns=2)]
NONFINITE = [_one(f"g_nonfinite_{p}", 5, 3, 70, "gaussian_wide", B0 + 27, ns=2, net="g_nonfinite", poison=p) for p in ("nan_g", "inf_g", "nan_x")]
RING = [_one("g_ring", 3, 5, 40, "gaussian", B0 + 1, ns=1)]
TABLE = SHAPES + NORANGE + BATCH + LARGE + REUSE + RANGES + SCALING + HANDOVER + RING
BY_TAG = {s["tag"]: s for s in TABLE + NONFINITE + [ONE_CENTRE]}
RANGE_TAGS = {s["tag"] for s in RANGES}
YARDSTICKED = [s for s in TABLE if s not in LARGE]            # the large pair: reference only, no yardstick

# worst (|err| - A)+ / S of yardstick_g() over YARDSTICKED: 9.83e-7 (g_far, log_sigs: exponents of -36 .. -64 in float32; the plain
# float32 yardstick of that case: 1.1e-6; next g_grows_spread, centers: 8.9e-7), recorded as the second two-digit figure above it:
# a float32 np.exp2 that differs in the last bit between CPUs could cross 9.9e-7.
# tests/test_k2g_reference_cpu.py::test_yardstick_g_and_the_coefficient recomputes it.
R_G = 1.0e-6
R_G_CASE = "g_far log_sigs"
C_G = 4 * R_G


# The finding these tests were written around.  Until this file existed s_h was s_g max_o s_o, which is not the size of the largest
# operand present: with the cotangent in a weight column 2^20 below the widest (kh.CaseH's wcols, inside K2h's documented range,
# K2h at 1.4e-6 S) every cotangent-side operand sat 2^-20 lower in the f16 subnormals.  The restatement with that rule
# (case.before_fix = True) and the kernel on an MI355X agreed to three digits -- max-norm ratio of d centers, bound 1:
#     h_wcols_spread  yardstick 7.050  kernel 7.049     g_wcols_gauss  5.403 / 5.401
#     g_wcols_iq      91.923 / 91.924 (d log_sigs 13.3)  g_wcols_imq    57.571 / 57.570 (d log_sigs 43.6)
# i.e. up to 4.6e-3 of max|d centers|; the issue's NumPy model (1.2e-5 resp. 1.1e-3 of max|hbar|) was right.  The sweep of the CPU
# test under the old rule crossed the bound at column spreads of 2^+-9 (gaussians) and 2^+-7 (the other bases).  K2g now takes s_h
# from the largest operand that is there; the wcols cases are the regression tests, profiles/k2g_parity.txt has both runs.
RANGE_NOTE = "s_h = pow2_above(max finite |g[q,o]| s_o); before: s_g * max_o s_o"


def ratios_g(got, ref, S, A):
    """(worst (|err| - A)+ / S with the absolute term read against C_G, max-norm ratio) over the finite elements of ref."""
    fin = np.isfinite(ref)
    if not fin.any():
        return 0.0, 0.0
    err = np.abs(np.asarray(got, np.float64)[fin] - ref[fin])
    if not np.isfinite(err).all():
        return float("inf"), float("inf")
    over = np.maximum(err - A[fin], 0.0)
    return float((over / (S[fin] + k2.ATOL_S / C_G)).max()), float(err.max() / (k2.MAXNORM_REL * np.abs(ref[fin]).max() + k2.MAXNORM_ABS))
