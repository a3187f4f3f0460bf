"""Helpers of tests/test_k2m_reference_cpu.py and tests/test_gpu_k2m.py: the f32 matrix-core parameter VJP K2m
(`rbf_vjp_mfma<D, OW, BC, CT>` with its pre-pass `vjpm_pack_kernel`, irbfn_amd/csrc/rbf_vjp_mfma.hip) on its own.  NumPy only.
Built on tests/_k2_util.py: the cases' draws, the float64 formulas, the gate and the bounds' ratios are that file's.

k2m_plan(...)       vjpm_ow, vjpm_ct, vjpm_groups, vjpm_slices, the cap of vjp_layout / plan_vjp (never more slabs than K2's layout
                    allocated) and launch_vjp_mfma's tiles per wave restated, so that a test states the launch it expects.
CaseM               a single-region k2.Case whose gate is replaced after the draw (x, g and the parameters stay what k2.Case drew):
                    gate="mid"     lower 0.0, upper 0.8, delta 3.0 on every gated coordinate: the box lies inside the queries' range
                                   [-0.9, 1.5], one factor runs from 0.0045 to 0.84 over it;
                    gate="column"  two range columns per gated coordinate, the box (0.0, 0.8) in the column that dimension_ranges
                                   names and (-9, 9) in the other; `cols` gives the column per coordinate (default: all 1), so
                                   max_ranges = 2 and the index read from dim_ranges is not 0 everywhere;
                    gate="sharp"   as mid with delta 20: a query left or right of the box has a float32 gamma of exactly 0
                                   (z < -13 ln 2, k2.tanh_gate's float32 form) where float64 keeps about 1e-16;
                    gate="none"    dimension_ranges = []: no region has a range row, gamma is 0 for every query.
                    A row with ns = 0 has no gated coordinate: its gamma is 1 whatever the key says.
                    poison="nan_xg" (beside k2.Case's three): a NaN in a GATED coordinate, x[23, 0].
reference(case)     k2.vjp_reference in centre chunks -> {leaf: (grad, S)}.  Every sum runs over the queries of one centre, so the
yardstick(case)     chunks change no bit of d centers, d log_sigs and d kernel; d bias is taken once.  yardstick: k2.vjp_float32
                    in the same chunks, without the [B, 1, K, O] intermediate in one piece.

Bounds of tests/test_gpu_k2m.py, on every leaf of every case:
  max|got - ref| <= 5e-5 max|ref| + 1e-7     the project's own, unchanged;
  |got - ref|    <= C_M * S + 1e-30          element-wise, C_M = 4 * R32M (the factor 4 as in tests/_k2_util.py: the kernel's other
                                             summation order and its v_exp_f32); C_M may not exceed 5e-5."""
import numpy as np

import _k2_util as k2
from _k2_util import LEAVES, LEAF_PATH, Case, _cdiv, bclass, padded_D, padded_O, same_nonfinite, tanh_gate  # noqa: F401

# worst |err| / S of yardstick() over TABLE: 1.45e-6 (m_b1, centers: one query, so an element is one term, and hbar = g . W[k, :]
# of 20 outputs cancels to a fortieth of its largest term for the worst of the 40 centres; the next is m_b1's log_sigs, then
# m_slab_cap's kernel with 8.0e-7), rounded up to two digits; np.exp in float32 may differ in the last bit between CPUs.
# tests/test_k2m_reference_cpu.py::test_yardstick_and_the_coefficient recomputes it.
R32M = 1.5e-6
C_M = 4 * R32M
ELEMENTS = 1 << 22           # of the [B, 1, chunk, O] intermediate of one yardstick chunk


def vjpm_ow(O):
    return 32 if O <= 32 else 64 if O <= 64 else 128


def vjpm_ct(OW):
    return 2 if OW <= 64 else 1


def k2m_plan(N, B, D, O, basis):
    """The launch of a forced K2m call: blocks of 4 waves, every wave on the same CT tiles of 16 centres, S query slabs of 4 waves; a
    wave walks tiles_per_wave consecutive 16-query tiles.  S: about 512 blocks (vjpm_slices), at least 16 tiles per slab, never more
    than the slabs K2's layout allocated (vjp_layout's QSB)."""
    OW = vjpm_ow(O)
    CT = vjpm_ct(OW)
    groups = _cdiv(N, 16 * CT)
    QSB = min(_cdiv(8192, 4 * _cdiv(N, 64)), _cdiv(B, 256), 4096)
    ntiles = _cdiv(B, 16)
    by_groups, by_batch = _cdiv(512, groups), _cdiv(ntiles, 16)
    S = max(1, min(by_groups, by_batch, QSB))
    tpw = _cdiv(ntiles, 4 * S)
    DC, BC = padded_D(D), bclass(basis)
    return {"OW": OW, "CT": CT, "CW": 16 * CT, "DC": DC, "BC": BC, "OP": padded_O(O), "groups": groups, "S": S, "grid": groups * S,
            "block": 256, "ntiles": ntiles, "tiles_per_wave": tpw, "idle_waves": [w for w in range(4 * S) if w * tpw >= ntiles],
            "by_groups": by_groups, "by_batch": by_batch, "QSB": QSB,
            "name": f"rbf_vjp_mfma<D={DC},OW={OW},BC={BC},CT={CT},QSB={S}>"}


# ------------------------------------------------------------------------------------------------ the cases
BOX_LO, BOX_HI, FAR = 0.0, 0.8, 9.0
DELTA = {"mid": 3.0, "column": 3.0, "sharp": 20.0, "none": 3.0}


class CaseM(Case):
    """A k2.Case of kind "one" with the gate its spec names (this file's docstring)."""

    def __init__(self, spec):
        super().__init__(spec)
        assert self.kind == "one" and self.R == 1 and self.basis in k2.FAST
        self.gate = spec.get("gate", "mid")
        ns = self.ns
        self.cols = list(spec.get("cols", [1] * ns)) if self.gate == "column" else [0] * ns
        assert len(self.cols) == ns
        if self.gate == "column":       # the box in the column that is read, (-FAR, FAR) in the other
            self.cfg.update(lower_bounds=[[-FAR, BOX_LO] if c else [BOX_LO, -FAR] for c in self.cols],
                            upper_bounds=[[FAR, BOX_HI] if c else [BOX_HI, FAR] for c in self.cols], dimension_ranges=[self.cols])
        else:
            self.cfg.update(lower_bounds=[[BOX_LO]] * ns, upper_bounds=[[BOX_HI]] * ns,
                            dimension_ranges=[] if self.gate == "none" else [[0] * ns])
        self.cfg["delta"] = [DELTA[self.gate]] * ns
        if spec.get("poison") == "nan_xg":
            assert ns >= 1
            self.x[23, 0] = np.nan       # a gated coordinate

    def gamma_other_column(self, dtype=np.float64):
        """gamma with the other range column of every gated coordinate: what a pack that ignores dim_ranges would store."""
        return tanh_gate(dict(self.cfg, dimension_ranges=[[1 - c for c in self.cols]]), self.x, dtype)

    def plan(self):
        return k2m_plan(self.N, self.B, self.D, self.O, self.basis)

    def reference(self):
        return reference(self)

    def yardstick(self):
        return yardstick(self)


def _centre_chunks(case, chunk):
    p = case.params["params"]
    c, ls, W = (p[a][b] for a, b in (LEAF_PATH["centers"], LEAF_PATH["log_sigs"], LEAF_PATH["kernel"]))
    for a in range(0, case.K, chunk):
        yield {"params": {"rbf_list": {"centers": c[:, a:a + chunk], "log_sigs": ls[:, a:a + chunk]},
                          "linear": {"kernel": W[a:a + chunk], "bias": p["linear"]["bias"]}}}


def _chunk_of(case, chunk):
    return max(1, ELEMENTS // (case.B * case.O)) if chunk is None else chunk


def reference(case, chunk=None):
    """k2.vjp_reference over centre chunks -> {leaf: (grad, S)}."""
    gamma = case.gamma()
    parts = [k2.vjp_reference(case.basis, sub, case.x, case.g, gamma) for sub in _centre_chunks(case, _chunk_of(case, chunk))]
    out = {leaf: tuple(np.concatenate([p[leaf][i] for p in parts], axis=ax) for i in (0, 1))
           for leaf, ax in (("centers", 1), ("log_sigs", 1), ("kernel", 0))}
    out["bias"] = parts[0]["bias"]
    return out


def yardstick(case, chunk=None):
    """k2.vjp_float32 over centre chunks -> {leaf: grad}."""
    gamma = case.gamma(np.float32)
    parts = [k2.vjp_float32(case.basis, sub, case.x, case.g, gamma) for sub in _centre_chunks(case, _chunk_of(case, chunk))]
    out = {leaf: np.concatenate([p[leaf] for p in parts], axis=ax) for leaf, ax in (("centers", 1), ("log_sigs", 1), ("kernel", 0))}
    out["bias"] = parts[0]["bias"]
    return out


def _m(D, O, K, basis, B, ns, **kw):
    return k2._one(kw.pop("tag", f"m_d{D}_o{O}_n{K}_{basis}"), D, O, K, basis, B, ns=ns, gate=kw.pop("gate", "mid"), **kw)


# Every compiled instance (DC in 3, 4, 7, 8) x (OW in 32, 64, 128) x (BC in 0, 1, 2) once; every real D from 1 to 8; O at both
# ends of each OW and of OP = 100 under OW = 128; the five fast bases, gaussian_wide and gaussian_wider at three OW each; K around
# the centre tile CW = 16 CT (32 for OW <= 64, 16 for OW = 128) and K2's 64-centre Npad; ns = 0, 0 < ns < D and ns = D.
SHAPES = [
    # OW = 32
    _m(1, 17, 1, "gaussian", 70, 1), _m(2, 32, 15, "inverse_quadratic", 300, 2), _m(3, 17, 16, "inverse_multiquadric", 100, 0),
    _m(4, 32, 17, "gaussian_wide", 131, 1), _m(4, 17, 31, "inverse_quadratic", 77, 0), _m(4, 32, 32, "inverse_multiquadric", 301, 2),
    _m(5, 17, 33, "gaussian_wider", 257, 2), _m(6, 32, 63, "inverse_quadratic", 90, 1), _m(7, 17, 64, "inverse_multiquadric", 113, 1),
    _m(8, 32, 65, "gaussian", 270, 2), _m(8, 17, 1, "inverse_quadratic", 95, 1), _m(8, 32, 15, "inverse_multiquadric", 65, 0),
    # OW = 64
    _m(3, 33, 16, "gaussian_wide", 290, 2), _m(1, 64, 17, "inverse_quadratic", 81, 1), _m(2, 33, 31, "inverse_multiquadric", 99, 1),
    _m(4, 64, 32, "gaussian_wider", 120, 1), _m(4, 33, 33, "inverse_quadratic", 310, 2), _m(4, 64, 63, "inverse_multiquadric", 75, 1),
    _m(6, 33, 64, "gaussian", 67, 0), _m(7, 64, 65, "inverse_quadratic", 333, 2), _m(5, 33, 1, "inverse_multiquadric", 83, 1),
    _m(8, 64, 15, "gaussian_wide", 141, 1), _m(8, 33, 16, "inverse_quadratic", 71, 0), _m(8, 64, 17, "inverse_multiquadric", 299, 2),
    # OW = 128
    _m(2, 65, 1, "gaussian_wider", 285, 2), _m(3, 100, 15, "inverse_quadratic", 79, 1), _m(1, 101, 16, "inverse_multiquadric", 91, 1),
    _m(4, 128, 17, "gaussian", 101, 1), _m(4, 65, 33, "inverse_quadratic", 277, 2), _m(4, 100, 1, "inverse_multiquadric", 69, 0),
    _m(7, 101, 15, "gaussian_wide", 303, 2), _m(5, 128, 16, "inverse_quadratic", 87, 1), _m(6, 65, 17, "inverse_multiquadric", 93, 1),
    _m(8, 100, 33, "gaussian_wider", 119, 1), _m(8, 101, 1, "inverse_quadratic", 73, 1), _m(8, 128, 15, "inverse_multiquadric", 311, 2),
]
K_AROUND = {32: (1, 15, 16, 17, 31, 32, 33, 63, 64, 65), 16: (1, 15, 16, 17, 33)}       # by CW
GATES = [
    _m(4, 40, 40, "gaussian", 200, 1, tag="m_gate_column_ns1", gate="column"),
    _m(5, 70, 20, "inverse_quadratic", 600, 3, tag="m_gate_column_ns3", gate="column", cols=[1, 0, 1]),
    _m(3, 20, 30, "inverse_multiquadric", 200, 1, tag="m_gate_sharp", gate="sharp"),
    _m(3, 24, 20, "gaussian_wide", 100, 1, tag="m_gate_none", gate="none"),
]
BATCH_EDGES = (1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 513, 1021)
BATCH = [_m(3, 20, 40, "gaussian", B, 1, tag=f"m_b{B}", net="m_batch", draw=1021) for B in BATCH_EDGES]
# 63 centre groups: S = 9 slabs from ceil(512 / 63) where the batch would allow 10; 145 tiles, 5 per wave: waves 29 .. 35 idle
SLAB_CAP = [_m(8, 100, 1000, "gaussian", 2305, 1, tag="m_slab_cap")]
REUSE = [_m(4, 33, 150, "gaussian", 65, 1, tag="m_reuse_b65", net="m_reuse", draw=4096),
         _m(4, 33, 150, "gaussian", 300, 1, tag="m_reuse_b300", net="m_reuse", draw=4096)]
# O = 18 is no multiple of 4 and B = 130 none of 16: the zero padding of g and W and the zero tail records share MFMAs with the poison
NONFINITE = [_m(5, 18, 70, "gaussian_wide", 130, 2, tag=f"m_nonfinite_{p}", net="m_nonfinite", poison=p)
             for p in ("nan_g", "nan_x", "inf_g", "nan_xg")]
ON_CENTRES = [_m(3, 20, 40, b, 67, 1, tag=f"m_on_centres_{b}", on_centres=True) for b in k2.FAST]
TABLE = SHAPES + GATES + BATCH + SLAB_CAP + REUSE + NONFINITE + ON_CENTRES
BY_TAG = {s["tag"]: s for s in TABLE}
assert len(BY_TAG) == len(TABLE)


def ratios_m(got, ref, S):
    """k2.ratios with the absolute term of the element-wise bound read against C_M: (worst |err| / S, max-norm ratio)."""
    fin = np.isfinite(ref)
    if not fin.any():
        return 0.0, 0.0
    err = np.abs(np.asarray(got, np.float64)[fin] - ref[fin])
    if not np.isfinite(err).all():
        return float("inf"), float("inf")
    return (float((err / (S[fin] + k2.ATOL_S / C_M)).max()),
            float(err.max() / (k2.MAXNORM_REL * np.abs(ref[fin]).max() + k2.MAXNORM_ABS)))
