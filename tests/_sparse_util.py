"""Helpers of tests/test_sparse_reference_cpu.py and tests/test_gpu_sparse_edges.py: the region-sparse kernels K1r / K2r
(irbfn_amd/csrc/rbf_sparse.hip) at their list and shape edges.  NumPy only: nothing here needs a GPU.

Card(spec)        a tanh-gated net from range edges per gated coordinate (they may overlap), delta per coordinate and a list of
                  rows of dimension_ranges; parameters drawn as tests/_k2_util.py::Case draws them (the gated coordinates of a
                  region's centres inside its box), queries and cotangents; one seed per net.
setup(...) ...    the host rules of rbf_sparse.hip restated (sparse_setup, sparse_ops, sparse_preferred, sparse_vjp_eligible,
                  sparse_vjp_lds_fits, sparse_vjp_slices, the slice bounds, K1r's launch), so that a test states what it expects.
gamma(cfg, x)     the gate the sparse kernels implement: the float64 gamma of _k2_util.tanh_gate with a half factor set to 0
                  exactly where the kernels' float32 delta * (x - lo) (or delta * (hi - x)) is below -9.0109133f.  A subtraction,
                  then a multiplication: no FMA can form, NumPy float32 gives the kernels' number.  Without it a region that no
                  query reaches has S = 1e-17 in the reference where the kernels have an exact 0.
live(cfg, x)      the float32 hit set per query under the same rule (NaN counts as a hit, as in the kernels).
forward_reference / Card.reference   float64 forward with its scale sum|gamma phi W| + |bias|; _k2_util.vjp_reference with that gamma.

Bounds of tests/test_gpu_sparse_edges.py:
  forward   |sparse - ref| <= 1e-5 |ref| + 3e-6 scale and |sparse - dense| <= 2e-6 scale + 1e-7 |ref| element-wise
            (tests/test_gpu_sparse.py); generic bases max|err| <= 2e-5 max|ref|;
  VJP       on every leaf element |err| <= C_S S + 1e-30, C_S = 4 * R32 (the margin of tests/test_gpu_k2.py, for the same reason:
            a butterfly, chunks, slices and a slab tree instead of one sequential sum, plus v_exp_f32), and the max-norm bound
            max|err| <= 5e-5 max|ref| + 1e-7."""
import collections
import zlib

import numpy as np

import _k2_util as k2
from oracle import irbfn_oracle as orc

LEAVES, LEAF_PATH = k2.LEAVES, k2.LEAF_PATH
Z32 = np.float32(9.0109133)                 # kGateSatZ (rbf_forward.h)
NT, WAVE, VP = 256, 64, 8                   # kSpNT, kWave, kSpVP
MAX_E, MAX_CAP, MAX_REGIONS, MAX_LDS, MAX_SPLIT = 32, 96, 1024, 150 * 1024, 8
WP, PART_PITCH = 16, 20                     # kSpWP, kSpPartPitch

# worst |err| / S of _k2_util.vjp_float32 with gamma() over the VJP cases of TABLE: 2.76e-6 (b1, centers), rounded up to two digits.  tests/test_sparse_reference_cpu.py::test_yardstick_and_the_coefficient recomputes it.
R32 = 2.8e-6
C_S = 4 * R32
MAXNORM_REL, MAXNORM_ABS, ATOL_S = 5e-5, 1e-7, 1e-30


def _cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ host rules, restated
def sparse_ops(O):
    return 2 if O <= 2 else 5 if O <= 5 else 10 if O <= 10 else 16 if O <= 16 else -1


def img_layout(nr, RS, E, K):
    """sp_img_layout, in dwords."""
    o = nr * 2
    o = (o + 3) & ~3
    o += (nr + 31) & ~31
    o += E * 4
    o += K * WP
    small = (o + 255) & ~255
    return {"small": small, "total": small + ((nr * RS + 255) & ~255)}


def fwd_lds_dwords(img, nr, E, cap, wide):
    """sp_lds_layout(...).total."""
    o = img + E * NT + 9 * NT
    o = (o + 3) & ~3
    o += PART_PITCH * NT + ((nr + 31) >> 5) * NT
    o += (cap * NT * (2 if wide else 1) + 3) // 4 + (cap * NT + 3) // 4
    return o + NT // 64 + 1


def rows_of(cfg):
    ns = len(cfg["activation_idx"])
    return [tuple(r[:ns]) for r in cfg["dimension_ranges"][:cfg["num_regions"]]]


def setup(cfg):
    """sparse_setup -> dict(ok, E, cap, mean, RS, OPS, lds).  cap: per gated coordinate the largest number of ranges that are
    non-zero together (intervals widened by 1e-4 of the margin and 1e-6 of their size), their product times the largest number of
    rows that share one combination of ranges, at most nr.  mean: the expected number of live regions of a query uniform over the
    card's span, scaled by rows per distinct combination."""
    ns, rows = len(cfg["activation_idx"]), rows_of(cfg)
    nr, R, K = len(rows), cfg["num_regions"], cfg["num_kernels"]
    out = {"ok": False, "E": 0, "cap": 0, "mean": 0.0, "nr": nr}
    if R < 2 or nr < 2 or ns < 1 or ns > MAX_SPLIT or nr > MAX_REGIONS:
        return out
    OPS = sparse_ops(cfg["out_features"])
    if OPS < 0:
        return out
    E, cap, mean = 0, 1.0, 1.0
    for d in range(ns):
        dl = float(np.float32(cfg["delta"][d]))
        if not (dl > 0 and np.isfinite(dl)):
            return out
        used = sorted({r[d] for r in rows})
        marg = float(Z32) / dl * (1.0 + 1e-4)
        ab = [(float(np.float32(cfg["lower_bounds"][d][j])), float(np.float32(cfg["upper_bounds"][d][j]))) for j in used]
        ev = []
        for a, b in ab:
            tiny = 1e-6 * (abs(a) + abs(b) + 1.0)
            ev += [(a - marg - tiny, +1), (b + marg + tiny, -1)]
        E += len(used)
        ev.sort(key=lambda e: (e[0], -e[1]))                     # openings first: closed intervals
        cur = best = 0
        for _, s in ev:
            cur += s
            best = max(best, cur)
        L, U = min(a for a, _ in ab), max(b for _, b in ab)
        covered = sum(max(0.0, min(U, b + marg) - max(L, a - marg)) for a, b in ab)
        cap *= best
        mean *= max(1.0, covered / (U - L)) if U > L else float(len(used))
    out["E"] = E
    if E > MAX_E:
        return out
    combos = collections.Counter(rows)
    cap = min(cap * max(combos.values()), float(nr))
    mean = min(mean * (nr / len(combos)), float(nr))
    out.update(cap=int(cap), mean=float(np.float32(mean)))
    if cap > MAX_CAP:
        return out
    DC = k2.padded_D(cfg["in_features"])
    EW = (DC + 1 + 3) & ~3
    RS = K * EW
    if ((RS // 4) & 1) == 0:
        RS += 4                                                  # an odd number of 16-byte slots per region
    im = img_layout(nr, RS, E, K)
    lds = fwd_lds_dwords(im["total"], nr, E, int(cap), nr > 256) * 4
    out.update(RS=RS, OPS=OPS, lds=lds, small=im["small"])
    out["ok"] = lds <= MAX_LDS
    return out


def sparse_preferred(cfg, B):
    s = setup(cfg)
    return bool(s["ok"] and B > 64 and np.float32(s["mean"]) <= np.float32(0.25) * np.float32(s["nr"]))


def vjp_eligible(cfg):
    s = setup(cfg)
    DC, OP = k2.padded_D(cfg["in_features"]), k2.padded_O(cfg["out_features"])
    return bool(s["ok"] and cfg["basis_func"] in k2.FAST and OP <= 16 and cfg["num_kernels"] * (DC + 1 + OP) * 4 <= 60 * 1024)


def vjp_lds_fits(cfg):
    s = setup(cfg)
    nr, nr64, NW = s["nr"], (s["nr"] + 63) & ~63, NT // WAVE
    return (s["small"] + s["E"] * NT + 9 * NT + ((nr + 31) // 32) * NT + 3 * NW * nr64 + nr64 + NW + 8) * 4 <= MAX_LDS


def vjp_slices(cfg, B):
    s = setup(cfg)
    per_region = float(B) * float(np.float32(s["mean"])) / s["nr"]
    sl = int(per_region / (WAVE * VP) + 0.999)
    while sl * s["nr"] < 1024 and sl < 64:
        sl += 1
    return min(max(sl, 1), 64)


def slice_bounds(Lr, SL):
    return [(Lr * sl // SL, Lr * (sl + 1) // SL) for sl in range(SL)]


def k1r_launch(cfg, B, roll=False, n_cu=256):
    grid = _cdiv(B, NT)
    return {"kernel": f"rbf_fwd_sparse<D={k2.padded_D(cfg['in_features'])},OP={sparse_ops(cfg['out_features'])},"
                      f"BC={k2.bclass(cfg['basis_func'])},ROLL={int(roll)},GC={int(grid > n_cu)}>", "grid": grid, "block": NT}


# ------------------------------------------------------------------------------------------------ the gate of the sparse kernels
def _factors(cfg, x):
    """Per gated coordinate ([B, ranges] float64 factor with the kernels' exact zeros, [B, ranges] bool: float32 factor != 0)."""
    x64, x32, f32 = np.asarray(x, np.float64), np.asarray(x, np.float32), np.float32
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(len(cfg["activation_idx"])):
            lo, hi, dl = np.asarray(cfg["lower_bounds"][d]), np.asarray(cfg["upper_bounds"][d]), cfg["delta"][d]
            zl = f32(dl) * (x32[:, d, None] - lo.astype(f32)[None])
            zh = f32(dl) * (hi.astype(f32)[None] - x32[:, d, None])
            assert zl.dtype == f32 and zh.dtype == f32
            fl = np.where(zl < -Z32, 0.0, (np.tanh(dl * (x64[:, d, None] - lo[None])) + 1) / 2)
            fh = np.where(zh < -Z32, 0.0, (np.tanh(dl * (hi[None] - x64[:, d, None])) + 1) / 2)
            out.append((fl * fh, ~((zl < -Z32) | (zh < -Z32))))
    return out


def gamma(cfg, x):
    fac, rows = _factors(cfg, x), rows_of(cfg)
    g = np.zeros((len(x), cfg["num_regions"]))
    for r, row in enumerate(rows):
        cur = np.ones(len(x))
        for d, j in enumerate(row):
            cur = cur * fac[d][0][:, j]
        g[:, r] = cur
    return g


def live(cfg, x):
    """[B, R] bool: the regions whose float32 factors are all non-zero."""
    fac, rows = _factors(cfg, x), rows_of(cfg)
    h = np.zeros((len(x), cfg["num_regions"]), bool)
    for r, row in enumerate(rows):
        cur = np.ones(len(x), bool)
        for d, j in enumerate(row):
            cur &= fac[d][1][:, j]
        h[:, r] = cur
    return h


def between_the_zeros(cfg, x):
    """Is some half factor of some query 0 for the kernels and not yet 0 in float64 (tanh(z) + 1 == 0 from z = -19.06 down)?"""
    x64, x32, f32 = np.asarray(x, np.float64), np.asarray(x, np.float32), np.float32
    for d in range(len(cfg["activation_idx"])):
        lo, hi, dl = np.asarray(cfg["lower_bounds"][d]), np.asarray(cfg["upper_bounds"][d]), cfg["delta"][d]
        for z32, z64 in ((f32(dl) * (x32[:, d, None] - lo.astype(f32)[None]), dl * (x64[:, d, None] - lo[None])),
                         (f32(dl) * (hi.astype(f32)[None] - x32[:, d, None]), dl * (hi[None] - x64[:, d, None]))):
            if ((z32 < -Z32) & (np.tanh(z64) + 1 != 0)).any():
                return True
    return False


def forward_reference(cfg, params, x, gam=None):
    """(ref, scale) in float64: orc.wcrbfnet_apply's terms with gamma(), scale = sum |gamma phi W| + |bias|."""
    p = orc.cast_params(params, np.float64)["params"]
    x64 = np.asarray(x, np.float64)
    gam = gamma(cfg, x) if gam is None else gam
    with np.errstate(invalid="ignore", over="ignore"):
        phi = orc.rbf_layer(x64, p["rbf_list"]["centers"], p["rbf_list"]["log_sigs"], cfg["basis_func"])
        W, b = p["linear"]["kernel"], p["linear"]["bias"]
        return (gam[:, :, None] * phi).sum(1) @ W + b, np.abs(gam[:, :, None] * phi).sum(1) @ np.abs(W) + np.abs(b)


def ratios(got, ref, S):
    """(worst |err| / S over the finite elements of ref, max|err| / (5e-5 max|ref| + 1e-7)); ATOL_S / C_S is added to S."""
    fin = np.isfinite(ref)
    if not fin.any():
        return 0.0, 0.0
    err = np.abs(np.asarray(got, np.float64)[fin] - ref[fin])
    if not np.isfinite(err).all():
        return float("inf"), float("inf")
    return float((err / (S[fin] + ATOL_S / C_S)).max()), float(err.max() / (MAXNORM_REL * np.abs(ref[fin]).max() + MAXNORM_ABS))


# ------------------------------------------------------------------------------------------------ cards
def unit_ranges(n):
    """n ranges [i, i + 1]: with delta = 20 (margin 0.45) never more than two of them are non-zero together."""
    return [float(i) for i in range(n)], [float(i + 1) for i in range(n)]


def grid_rows(dims, nrows=None):
    rows = [[]]
    for n in dims:
        rows = [r + [j] for r in rows for j in range(n)]
    return rows[:nrows]


def cfg_only(spec):
    """The card of a spec without drawing anything."""
    lows, highs = spec["lows"], spec["highs"]
    return {"in_features": spec["D"], "out_features": spec["O"], "num_kernels": spec["K"], "basis_func": spec["basis"],
            "num_regions": spec.get("R", len(spec["rows"])), "lower_bounds": [list(map(float, v)) for v in lows],
            "upper_bounds": [list(map(float, v)) for v in highs], "dimension_ranges": [list(r) for r in spec["rows"]],
            "activation_idx": list(range(len(lows))), "delta": [float(v) for v in spec["delta"]]}


class Card:
    """One row of TABLE with its inputs: cfg, params, x[B, D], g[B, O] in float32.  spec: tag, D, O, K, basis, B and
    lows / highs / delta per gated coordinate, rows; R (num_regions, default the number of rows); net (the seed's name, default
    the tag) and draw (rows drawn for the net: cases on one net share one batch, the first B rows of it); queries: how the gated
    coordinates of the batch are chosen (QUERIES)."""

    def __init__(self, spec):
        self.spec, self.tag = spec, spec["tag"]
        self.D, self.O, self.K, self.basis, self.B = spec["D"], spec["O"], spec["K"], spec["basis"], spec["B"]
        D, O, K = self.D, self.O, self.K
        lows, highs, rows = spec["lows"], spec["highs"], [list(r) for r in spec["rows"]]
        ns = len(lows)
        R = spec.get("R", len(rows))
        self.R, self.N, self.ns = R, R * K, ns
        self.cfg = cfg_only(spec)
        rng = np.random.default_rng(zlib.crc32(spec.get("net", self.tag).encode()))
        span = [(min(lows[d]), max(highs[d])) for d in range(ns)]
        ls_lo = 0.2 if self.basis == "gaussian" else -0.5
        c = rng.uniform(-1.0, 1.6, size=(R, K, D))
        for r in range(R):
            for d in range(ns):
                a, b = (lows[d][rows[r][d]] - 0.1, highs[d][rows[r][d]] + 0.1) if r < len(rows) else span[d]
                c[r, :, d] = rng.uniform(a, b, size=K)
        self.params = {"params": {"rbf_list": {"centers": c.astype(np.float32),
                                               "log_sigs": rng.uniform(ls_lo, 1.0, size=(R, K)).astype(np.float32)},
                                  "linear": {"kernel": (rng.normal(size=(K, O)) * 0.5).astype(np.float32),
                                             "bias": rng.normal(size=(O,)).astype(np.float32)}}}
        nb = max(self.B, spec.get("draw", self.B))
        x = rng.uniform(-0.9, 1.5, size=(nb, D))
        x[:, :ns] = QUERIES[spec.get("queries", "boxes")](self, rng, nb)
        self.x = np.ascontiguousarray(x[:self.B].astype(np.float32))
        self.g = np.ascontiguousarray(rng.normal(size=(nb, O))[:self.B].astype(np.float32))

    def gamma(self):
        return gamma(self.cfg, self.x)

    def live(self):
        return live(self.cfg, self.x)

    def forward_reference(self):
        return forward_reference(self.cfg, self.params, self.x)

    def reference(self):
        return k2.vjp_reference(self.basis, self.params, self.x, self.g, self.gamma())

    def yardstick(self):
        return k2.vjp_float32(self.basis, self.params, self.x, self.g, self.gamma())


def _q_boxes(card, rng, nb):
    """Row b lies in the box of row b % nr of dimension_ranges; two rows of three are then moved to a border of that box in one
    gated coordinate: onto it (b % 3 == 1) or within 0.3 / delta of it (b % 3 == 2)."""
    cfg, rows = card.cfg, card.cfg["dimension_ranges"]
    q = np.zeros((nb, card.ns))
    for b in range(nb):
        row = rows[b % len(rows)]
        for d in range(card.ns):
            q[b, d] = rng.uniform(cfg["lower_bounds"][d][row[d]], cfg["upper_bounds"][d][row[d]])
        if b % 3:
            d = int(rng.integers(card.ns))
            edge = (cfg["lower_bounds"], cfg["upper_bounds"])[int(rng.integers(2))][d][row[d]]
            q[b, d] = edge + (0.0 if b % 3 == 1 else rng.uniform(-0.3, 0.3) / cfg["delta"][d])
    return q


def _q_span(card, rng, nb):
    """Uniform over the card's span."""
    cfg = card.cfg
    return np.stack([rng.uniform(min(cfg["lower_bounds"][d]), max(cfg["upper_bounds"][d]), nb) for d in range(card.ns)], axis=1)


def _q_unit(card, rng, nb):
    """Uniform over [0, 1] in every gated coordinate."""
    return rng.uniform(0.0, 1.0, size=(nb, card.ns))


def _q_one_box(card, rng, nb):
    """Every query inside the box of the row spec['box']."""
    cfg, row = card.cfg, card.cfg["dimension_ranges"][card.spec["box"]]
    return np.stack([rng.uniform(cfg["lower_bounds"][d][row[d]], cfg["upper_bounds"][d][row[d]], nb) for d in range(card.ns)], axis=1)


def _q_around(card, rng, nb):
    """Within spec['radius'] of the point spec['at'], the first query on it."""
    at, rad = np.asarray(card.spec["at"], np.float64), card.spec["radius"]
    q = at[None] + rng.uniform(-rad, rad, size=(nb, card.ns))
    q[0] = at
    return q


def _q_empty_middle(card, rng, nb):
    """Blocks of 256 queries: block 1 stays at least two boxes away from the box of row 0, the others are drawn over the span
    with every fourth query inside that box -> row 0 has pairs in blocks 0 and 2 and none in block 1."""
    cfg = card.cfg
    q = _q_span(card, rng, nb)
    row = cfg["dimension_ranges"][0]
    for d in range(card.ns):
        q[::4, d] = rng.uniform(cfg["lower_bounds"][d][row[d]], cfg["upper_bounds"][d][row[d]], len(q[::4]))
    hi0 = cfg["upper_bounds"][0][row[0]]
    q[NT:2 * NT, 0] = rng.uniform(hi0 + 1.0, max(cfg["upper_bounds"][0]), NT)
    return q


def margin_neighbours(cfg):
    """For every half factor of every range: the two neighbouring float32 x on either side of the point where the kernels'
    delta * (x - lo) (delta * (hi - x)) crosses -9.0109133f -> list of (coordinate, x with the factor 0, x with it alive)."""
    f32, out = np.float32, []
    for d in range(len(cfg["activation_idx"])):
        dl = f32(cfg["delta"][d])
        for tab, side in ((cfg["lower_bounds"], -1), (cfg["upper_bounds"], +1)):
            for e in tab[d]:
                e = f32(e)
                dead = (lambda v: dl * (v - e) < -Z32) if side < 0 else (lambda v: dl * (e - v) < -Z32)
                v = f32(float(e) + side * float(Z32) / float(dl))
                out_dir, in_dir = f32(side * np.inf), f32(-side * np.inf)
                while not dead(v):
                    v = np.nextafter(v, out_dir)
                while dead(np.nextafter(v, in_dir)):
                    v = np.nextafter(v, in_dir)
                out.append((d, float(v), float(np.nextafter(v, in_dir))))
    return out


def _q_margin(card, rng, nb):
    """The float32 neighbours of every threshold lo - Z / delta and hi + Z / delta in one gated coordinate, the other coordinates
    in the middle of a box; the rest of the batch as _q_boxes."""
    q, cfg = _q_boxes(card, rng, nb), card.cfg
    b = 0
    for d, dead, alive in margin_neighbours(cfg):
        mid = [int(rng.integers(len(cfg["lower_bounds"][d2]))) for d2 in range(card.ns)]
        for v in (dead, alive):
            for d2, j in enumerate(mid):
                q[b, d2] = 0.5 * (cfg["lower_bounds"][d2][j] + cfg["upper_bounds"][d2][j])
            q[b, d] = v
            b += 1
    card.n_margin = b
    return q


QUERIES = {"boxes": _q_boxes, "span": _q_span, "unit": _q_unit, "one_box": _q_one_box, "around": _q_around, "empty_middle": _q_empty_middle,
           "margin": _q_margin}


# ------------------------------------------------------------------------------------------------ the cases
def _grid(tag, dims, D, O, K, basis, B, nrows=None, delta=20.0, **kw):
    lows, highs = zip(*(unit_ranges(n) for n in dims))
    return dict(tag=tag, lows=list(lows), highs=list(highs), delta=[delta] * len(dims), rows=grid_rows(dims, nrows), D=D, O=O, K=K,
                basis=basis, B=B, **kw)


def _overlap(tag, counts, D, O, K, basis, B, **kw):
    """counts[d] ranges per gated coordinate that all span [0, 1] (range j: [-0.05 j, 1 + 0.05 j]): every combination is live for
    every query inside [0, 1]."""
    lows = [[-0.05 * j for j in range(n)] for n in counts]
    highs = [[1.0 + 0.05 * j for j in range(n)] for n in counts]
    return dict(tag=tag, lows=lows, highs=highs, delta=[20.0] * len(counts), rows=grid_rows(counts), D=D, O=O, K=K, basis=basis, B=B,
                queries="unit", **kw)


# Every D from 1 to 8 (DC = 3, 3, 3, 4, 7, 7, 7, 8; Dreal != DC at 1, 2, 5, 6) with 1 to 8 gated coordinates (fewer than D, D,
# more than 4: the second index word), both pad edges of the forward's OPS list {2, 5, 10, 16} and of K2r's OP list
# {2, 4, 5, 8, 10, 16}, the five fast bases, K = 1, 2, 3, 4, 5, 9 (the two-centre step's tails)
INSTANCES = [
    _grid("i_d1_o1_k1", (4,), 1, 1, 1, "gaussian", 300),
    _grid("i_d2_o2_k2", (3, 3), 2, 2, 2, "inverse_quadratic", 300),
    _grid("i_d3_o3_k3", (4,), 3, 3, 3, "inverse_multiquadric", 300),
    _grid("i_d4_o4_k4", (2, 2, 2, 2), 4, 4, 4, "gaussian_wide", 300),
    _grid("i_d5_o5_k5", (2, 2, 2, 2, 2), 5, 5, 5, "gaussian_wider", 300),
    _grid("i_d6_o6_k9", (2, 2, 2, 2, 2, 2), 6, 6, 9, "gaussian", 300),
    _grid("i_d7_o8_k3", (2, 2, 2, 2, 2, 1, 1), 7, 8, 3, "inverse_quadratic", 300),
    _grid("i_d8_o9_k2", (2, 2, 2, 2, 1, 1, 2, 1), 8, 9, 2, "inverse_multiquadric", 300),
    _grid("i_d8_o10_k5", (3, 3), 8, 10, 5, "gaussian_wide", 300),
    _grid("i_d7_o11_k4", (4, 2), 7, 11, 4, "gaussian", 300),
    _grid("i_d3_o16_k9", (2, 2, 2), 3, 16, 9, "inverse_quadratic", 300),
    _grid("i_d4_o10_k1", (3, 2), 4, 10, 1, "gaussian_wider", 300),
]
GENERIC = [
    _grid("g_d3_o5_multiquadric", (3, 3), 3, 5, 4, "multiquadric", 300),
    _grid("g_d7_o10_matern52", (4,), 7, 10, 3, "matern52", 300),
]
# rows sliced from the combinations of an 8 x 8 x 8 grid (E <= 24): around the 32 regions of a hit word, the 64 of a transposed
# mask, and 256 -> 257: the switch to 16-bit region lists
REGION_COUNTS = [_grid(f"nr{n}", (8, 8, 8), 3, 5, 2, "gaussian_wide", 300, nrows=n) for n in (2, 31, 32, 33, 63, 64, 65, 255, 256, 257)] + [
    _grid("nr1024_e32", (16, 8, 8), 3, 2, 1, "inverse_quadratic", 300),
    _grid("nr12_of_16", (4, 4), 3, 5, 3, "gaussian", 300, nrows=12, R=16),          # fewer rows than num_regions
]
CAPACITY = [
    _overlap("cap96", (12, 8), 3, 2, 2, "gaussian_wide", 300),                         # cap = nr = 96: 96 rounds per block
    _overlap("e32_nr87", (29, 3), 3, 5, 2, "inverse_quadratic", 300),                  # E = 32, every factor live, nr % 32 = 23
    dict(tag="margin", lows=[[0.1, 1.1, 2.3]] * 2, highs=[[1.1, 2.3, 3.0]] * 2, delta=[7.3, 20.0], rows=grid_rows((3, 3)), D=3, O=5,
         K=3, basis="gaussian", B=300, queries="margin"),
    # the card of _k2_util's r6_tiny: rows 2 and 4, 1 and 5 are the same combination
    dict(tag="repeated_rows", lows=[[-1.0, 0.85]] * 2, highs=[[0.5, 2.0]] * 2, delta=[10.0, 10.0],
         rows=[[0, 0], [0, 1], [1, 0], [1, 1], [1, 0], [0, 1]], D=3, O=5, K=5, basis="gaussian", B=300, queries="around",
         at=(0.7, 0.7), radius=0.1),
]
# K2r's lists.  long: 8 x 16 boxes, every query in box (3, 5): its region has B pairs, 8 slices of 1250 -- three trips of the
# chunk loop, the last with 226 pairs (register sets 0..3 full or partly, 4..7 empty); the neighbours have shorter lists, the
# other regions none.  b*: one net, nblk = 1 (no search step), 2, 3, 5.
LISTS = [_grid("long_b10000", (8, 16), 2, 3, 2, "gaussian_wide", 10000, queries="one_box", box=3 * 16 + 5),
         # the planner's instance (whole-row loads of x and the cotangent): 8 slices of 625 pairs, two trips, all eight register sets
         _grid("long_d7_o10_b5000", (8, 16), 7, 10, 2, "inverse_quadratic", 5000, queries="one_box", box=4 * 16 + 9)] + \
        [_grid(f"b{B}", (4, 4), 3, 5, 3, "inverse_quadratic", B, net="batch", draw=1025) for B in (1, 255, 256, 257, 513, 1025)] + \
        [_grid("empty_middle", (6, 2), 3, 5, 3, "gaussian", 768, queries="empty_middle")]
REUSE = [_grid(f"reuse_b{B}", (4, 4), 7, 10, 4, "gaussian", B, net="reuse", draw=3000, queries="span") for B in (3000, 70)]
OVERLAP_SMALL = [_overlap("perm", (3, 3), 3, 5, 3, "gaussian", 600)]
NONFINITE = [_grid("nonfinite", (4, 4), 4, 3, 3, "gaussian_wide", 300)]
TABLE = INSTANCES + GENERIC + REGION_COUNTS + CAPACITY + LISTS + REUSE + OVERLAP_SMALL + NONFINITE
VJP_CASES = [s for s in TABLE if s["basis"] in k2.FAST]
BY_TAG = {s["tag"]: s for s in TABLE}

# refusals: (tag that fits, tag that does not, which limit)
LIMITS = [
    _overlap("lim_e32", (29, 3), 3, 2, 1, "gaussian", 100), _grid("lim_e33", (17, 16), 3, 2, 1, "gaussian", 100),
    _overlap("lim_cap96", (12, 8), 3, 2, 1, "gaussian", 100), _overlap("lim_cap100", (10, 10), 3, 2, 1, "gaussian", 100),
    _grid("lim_nr1024", (11, 10, 10), 3, 2, 1, "gaussian", 100, nrows=1024), _grid("lim_nr1025", (11, 10, 10), 3, 2, 1, "gaussian", 100, nrows=1025),
    _grid("lim_o16", (3, 3), 3, 16, 2, "gaussian", 100), _grid("lim_o17", (3, 3), 3, 17, 2, "gaussian", 100),
]
LIMIT_BY_TAG = {s["tag"]: s for s in LIMITS}
LIMIT_PAIRS = [("lim_e32", "lim_e33"), ("lim_cap96", "lim_cap100"), ("lim_nr1024", "lim_nr1025"), ("lim_o16", "lim_o17")]


def lds_limit_specs():
    """(fits, does not) for K1r's 150 KiB (16 regions, the centre table grows with K) and for K2r's 60 KiB of accumulators
    (2 regions, K (DC + 1 + OP) floats at D = 8, O = 16; the forward's image holds 16 floats of weights per centre, so a narrow
    net passes 150 KiB first): the largest K that fits and the next."""
    def k_spec(tag, dims, K, D=3, O=2):
        return _grid(tag, dims, D, O, K, "gaussian", 100)
    K = 1
    while setup(cfg_only(k_spec("x", (4, 4), K + 1)))["ok"]:
        K += 1
    K2 = 60 * 1024 // ((8 + 1 + 16) * 4)
    return (k_spec("lds150_fits", (4, 4), K), k_spec("lds150_over", (4, 4), K + 1)), \
           (k_spec("lds60_fits", (2,), K2, 8, 16), k_spec("lds60_over", (2,), K2 + 1, 8, 16))


def dense_sample(cfg, n=20000, seed=0):
    """Queries for the brute-force maximum of len(live): uniform over the span widened by the margins, and combinations of the
    critical points of every coordinate (edges, edges -+ the margin, box centres)."""
    rng = np.random.default_rng(seed)
    cols, crit = [], []
    for d in range(len(cfg["activation_idx"])):
        lo, hi, m = np.asarray(cfg["lower_bounds"][d]), np.asarray(cfg["upper_bounds"][d]), float(Z32) / cfg["delta"][d]
        cols.append(rng.uniform(lo.min() - 1.2 * m, hi.max() + 1.2 * m, n))
        pts = np.concatenate([lo, hi, lo - 0.999 * m, hi + 0.999 * m, lo - 0.5 * m, hi + 0.5 * m, (lo + hi) / 2])
        crit.append(pts[rng.integers(len(pts), size=n)])
    return np.vstack([np.stack(cols, axis=1), np.stack(crit, axis=1)]).astype(np.float32)
