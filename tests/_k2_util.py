"""Helpers of tests/test_k2_reference_cpu.py and tests/test_gpu_k2.py: the float32 parameter VJP K2 (`rbf_vjp_kernel`,
irbfn_amd/csrc/rbf_vjp.hip) on its own.  NumPy only: nothing here needs a GPU.

reference(case)   the four gradient formulas at the head of rbf_vjp.hip in float64, every basis, the tanh gate
                  (regions without a range stay 0) or a caller-given gamma[B, R] (cluster nets).  Per leaf -> (grad, S): S has the
                  leaf's shape and is the sum over the queries (d kernel: and regions) of the ABSOLUTE per-query terms, i.e. the
                  scale against which a rounding error of that element is to be read.
yardstick(case)   the same restatement in float32, the queries added one after the other (np.cumsum): what a plain float32
                  evaluation of the formulas loses.  Its worst |err| / S over TABLE is R32.
k2_plan(...)      vjp_layout's K2 rules restated, so that a test states the launch it expects instead of reading it back.

Bounds of tests/test_gpu_k2.py, both on every leaf of every case:
  max|got - ref| <= 5e-5 max|ref| + 1e-7     the project's own (tests/test_gpu_parity.py::test_net_vjp_*), unchanged;
  |got - ref|    <= C_S * S + 1e-30          element-wise, C_S = 4 * R32: the factor 4 covers the kernel's other summation order
                                             (four waves, slabs, a tree) and its v_exp_f32; C_S may not exceed 5e-5, the
                                             coefficient the first bound grants relative to the largest element."""
import zlib

import numpy as np

LEAVES = ("centers", "log_sigs", "kernel", "bias")
LEAF_PATH = {"centers": ("rbf_list", "centers"), "log_sigs": ("rbf_list", "log_sigs"), "kernel": ("linear", "kernel"),
             "bias": ("linear", "bias")}
FAST = {"gaussian": 0, "gaussian_wide": 0, "gaussian_wider": 0, "inverse_quadratic": 1, "inverse_multiquadric": 2}
COMPILED_OP = (2, 4, 5, 8, 10, 16, 32, 64, 100, 128)
GAUSS_A = {"gaussian": 1.0, "gaussian_wide": 0.1, "gaussian_wider": 0.01}

# worst |err| / S of yardstick() over TABLE: 1.62e-6 (r130, centers), rounded up to two digits; np.exp in float32 may differ in the
# last bit between CPUs.  tests/test_k2_reference_cpu.py::test_yardstick_and_the_coefficient recomputes it.
R32 = 1.7e-6
C_S = 4 * R32
MAXNORM_REL, MAXNORM_ABS, ATOL_S = 5e-5, 1e-7, 1e-30


def _cdiv(a, b):
    return -(-a // b)


def bclass(basis):
    return FAST.get(basis, 3)


def padded_D(D):
    return 3 if D <= 3 else 4 if D == 4 else 7 if D <= 7 else 8


def padded_O(O):
    return next(op for op in COMPILED_OP if O <= op)


def k2_plan(N, B, D, O, basis, gated):
    """vjp_layout / plan_vjp / launch_vjp_k2 for K2: 64 centres per group, enough slabs of four waves for 8192 waves in the launch
    but at least 64 queries per wave; the waves share the batch evenly."""
    groups = _cdiv(N, 64)
    QSB = min(_cdiv(8192, 4 * groups), _cdiv(B, 256))
    DC, OP = padded_D(D), padded_O(O)
    return {"groups": groups, "QSB": QSB, "grid": groups * QSB, "per_wave": _cdiv(B, 4 * QSB),
            "bias_blocks": _cdiv(B, 64) if B < 16384 else 256, "lds": 4 * (DC + 1 + OP) * 65 * 4,
            "name": f"rbf_vjp_kernel<D={DC},OP={OP},BC={bclass(basis)},GATED={int(gated)}>"}


# ------------------------------------------------------------------------------------------------ the formulas
def basis_terms(name, d2):
    """(phi, d phi / d(d2), None) at d2 = |x - c|^2 / sigma^2, in d2's dtype, for the bases in d2 alone.  The bases that depend on d = sqrt(d2) itself go through
    phi'(d) * (0.5 / d), as the kernel's generic class does, and return phi'(d) * d as the third value: the width reaches d without
    the sqrt (d = sqrt(sum sq) / exp(log_sig), flax_rbf.py:280), so d phi / d log_sig = -phi'(d) d is finite for a query ON a centre,
    where the slope in d2 is not."""
    if name in GAUSS_A:
        phi = np.exp(-GAUSS_A[name] * d2)
        return phi, -GAUSS_A[name] * phi, None
    if name == "inverse_quadratic":
        phi = 1 / (1 + d2)
        return phi, -phi * phi, None
    if name == "inverse_multiquadric":
        phi = (1 + d2) ** -0.5
        return phi, -0.5 * phi ** 3, None
    if name == "multiquadric":
        phi = (1 + d2) ** 0.5
        return phi, 0.5 / phi, None
    if name == "quadratic":
        return d2, np.ones_like(d2), None
    d = np.sqrt(d2)
    if name == "linear":
        phi, dp = d, np.ones_like(d)
    elif name == "spline":
        phi, dp = d2 * np.log(d + 1), 2 * d * np.log(d + 1) + d2 / (d + 1)
    elif name == "poisson_one":
        phi, dp = (d - 1) * np.exp(-d), (2 - d) * np.exp(-d)
    elif name == "poisson_two":
        phi, dp = ((d - 2) / 2) * d * np.exp(-d), (2 * d - 1 - 0.5 * d2) * np.exp(-d)
    elif name == "matern32":
        s3 = 3 ** 0.5
        phi, dp = (1 + s3 * d) * np.exp(-s3 * d), -3 * d * np.exp(-s3 * d)
    elif name == "matern52":
        s5 = 5 ** 0.5
        phi, dp = (1 + s5 * d + (5 / 3) * d2) * np.exp(-s5 * d), -(5 / 3) * d * (1 + s5 * d) * np.exp(-s5 * d)
    else:
        raise ValueError(name)
    return phi, dp * (0.5 / d), dp * d


def basis_and_slope(name, d2):
    return basis_terms(name, d2)[:2]


def tanh_gate(cfg, x, dtype=np.float64):
    """gamma[B, R] of the smooth indicator (model.py:42-95): the product over the gated coordinates of
    (tanh(delta (x - lo)) + 1) / 2 * (tanh(delta (hi - x)) + 1) / 2; regions past the rows of dimension_ranges stay 0; a card
    without gated coordinates gives 1 to every region with a row.  float64: the expression as written.  float32: 1 / (1 + exp(-2z)),
    which is the same number without the cancellation of tanh(z) + 1, and 0 below z = -13 ln 2, where a float32 tanh IS -1."""
    x = np.asarray(x, dtype)
    B, R, ns = x.shape[0], cfg["num_regions"], len(cfg["activation_idx"])

    def half(z):
        if dtype == np.float64:
            return (np.tanh(z) + 1) / 2
        with np.errstate(over="ignore"):
            return np.where(z < dtype(-13 * np.log(2)), dtype(0), 1 / (1 + np.exp(-2 * z)))

    fac = []
    for d in range(ns):
        lo, hi, dl = np.asarray(cfg["lower_bounds"][d], dtype), np.asarray(cfg["upper_bounds"][d], dtype), dtype(cfg["delta"][d])
        fac.append(half(dl * (x[:, d, None] - lo[None])) * half(dl * (hi[None] - x[:, d, None])))
    gamma = np.zeros((B, R), dtype)
    for r in range(min(len(cfg["dimension_ranges"]), R)):
        cur = np.ones(B, dtype)
        for d in range(ns):
            cur = cur * fac[d][:, cfg["dimension_ranges"][r][d]]
        gamma[:, r] = cur
    return gamma


def softmax_gate(params, x, dtype=np.float64):
    """gamma[B, R] of a cluster net: softmax(x Wc + bc) (model.py:402-404)."""
    p = params["params"]["cluster"]
    z = np.asarray(x, dtype) @ np.asarray(p["kernel"], dtype) + np.asarray(p["bias"], dtype)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def _terms(basis, params, x, g, gamma, dtype):
    """The per-query terms of the four sums: tc[B,R,K,D], tl[B,R,K], h[B,R,K] (d kernel[k,o] = sum_b sum_r h[b,r,k] g[b,o]), g."""
    p = params["params"]
    c, ls, W = (np.asarray(p[a][b], dtype) for a, b in (LEAF_PATH["centers"], LEAF_PATH["log_sigs"], LEAF_PATH["kernel"]))
    x, g, gamma = np.asarray(x, dtype), np.asarray(g, dtype), np.asarray(gamma, dtype)
    diff = x[:, None, None, :] - c[None]
    r2 = (diff * diff).sum(-1)
    s2 = np.exp(-2 * ls)[None]
    d2 = r2 * s2
    phi, dphi, dpd = basis_terms(basis, d2)
    hbar = g @ W.T
    G = hbar[:, None, :] * gamma[:, :, None]
    t = G * dphi
    return (t * s2)[..., None] * -2 * diff, t * (-2 * d2) if dpd is None else -(G * dpd), gamma[:, :, None] * phi, g


def vjp_reference(basis, params, x, g, gamma):
    """float64 -> {leaf: (grad, S)}."""
    with np.errstate(all="ignore"):
        tc, tl, h, g = _terms(basis, params, x, g, gamma, np.float64)
        return {"centers": (tc.sum(0), np.abs(tc).sum(0)), "log_sigs": (tl.sum(0), np.abs(tl).sum(0)),
                "kernel": (h.sum(1).T @ g, np.abs(h).sum(1).T @ np.abs(g)), "bias": (g.sum(0), np.abs(g).sum(0))}


def vjp_float32(basis, params, x, g, gamma):
    """The same in float32, every sum over the queries sequential -> {leaf: grad}."""
    f = np.float32
    seq = lambda a: np.cumsum(a, axis=0, dtype=f)[-1]
    with np.errstate(all="ignore"):
        tc, tl, h, g = _terms(basis, params, x, g, gamma, f)
        kern = seq(seq(h[:, :, :, None] * g[:, None, None, :]))      # [B,R,K,O]: the queries, then the regions
        out = {"centers": seq(tc), "log_sigs": seq(tl), "kernel": kern, "bias": seq(g)}
    assert all(v.dtype == f for v in out.values())
    return out


# ------------------------------------------------------------------------------------------------ the cases
class Case:
    """One row of TABLE with its inputs: cfg (None for a cluster net), params, x[B, D], g[B, O] in float32."""

    def __init__(self, spec):
        self.spec, self.tag, self.kind = spec, spec["tag"], spec["kind"]
        self.D, self.O, self.K, self.basis, self.B = spec["D"], spec["O"], spec["K"], spec["basis"], spec["B"]
        self.cluster = self.kind == "cluster"
        rng = np.random.default_rng(zlib.crc32(spec.get("net", self.tag).encode()))
        D, O, K = self.D, self.O, self.K
        cfg = {"in_features": D, "out_features": O, "num_kernels": K, "basis_func": self.basis}
        ns = 0
        gate_lo = gate_hi = None             # where the queries' gated coordinates are drawn
        if self.kind == "one":
            ns, R = spec.get("ns", 0), 1
            cfg.update(lower_bounds=[[-1.5]] * ns, upper_bounds=[[2.1]] * ns, dimension_ranges=[[0] * ns], delta=[8.0] * ns)
        elif self.kind == "regions":         # a x b boxes over the first two coordinates, region (i, j) = ranges i and j
            (a, b), ns = spec["grid"], 2
            R = a * b
            ea, eb = np.linspace(-1.0, 2.0, a + 1), np.linspace(-1.0, 2.0, b + 1)
            cfg.update(lower_bounds=[ea[:-1].tolist(), eb[:-1].tolist()], upper_bounds=[ea[1:].tolist(), eb[1:].tolist()],
                       dimension_ranges=[[i, j] for i in range(a) for j in range(b)][:spec.get("rows", R)],
                       delta=[spec.get("delta", 20.0)] * 2)
        elif self.kind == "tiny":            # every query in the first box: the other five regions weigh 4e-8 .. 3e-7 and less
            ns, R = 2, 6
            cfg.update(lower_bounds=[[-1.0, 0.85]] * 2, upper_bounds=[[0.5, 2.0]] * 2,
                       dimension_ranges=[[0, 0], [0, 1], [1, 0], [1, 1], [1, 0], [0, 1]], delta=[10.0, 10.0])
            gate_lo, gate_hi = 0.0, 0.1
        else:
            R = spec["R"]
        self.R, self.N, self.ns = R, R * K, ns
        self.gated = R > 1 or self.cluster
        cfg.update(num_regions=R, activation_idx=list(range(ns)))
        self.cfg = None if self.cluster else cfg
        # widths in [-0.5, 1]; the plain Gaussian keeps d2 small enough for a float32 exponent to mean something
        ls_lo = 0.2 if self.basis == "gaussian" else -0.5
        c = rng.uniform(-1.0, 1.6, size=(R, K, D))
        if self.kind == "regions":
            for r in range(R):
                i, j = divmod(r, spec["grid"][1])
                c[r, :, 0] = rng.uniform(ea[i] - 0.1, ea[i + 1] + 0.1, size=K)
                c[r, :, 1] = rng.uniform(eb[j] - 0.1, eb[j + 1] + 0.1, size=K)
        if self.kind == "tiny":
            c = rng.uniform(-0.5, 0.6, size=(R, K, D))
        self.params = {"params": {"rbf_list": {"centers": c.astype(np.float32),
                                               "log_sigs": rng.uniform(ls_lo, 1.0, size=(R, K)).astype(np.float32)},
                                  "linear": {"kernel": (rng.normal(size=(K, O)) * 0.5).astype(np.float32),
                                             "bias": rng.normal(size=(O,)).astype(np.float32)}}}
        if self.cluster:
            self.params["params"]["cluster"] = {"kernel": (rng.normal(size=(D, R)) * 0.7).astype(np.float32),
                                                "bias": rng.normal(size=(R,)).astype(np.float32)}
        nb = max(self.B, spec.get("draw", self.B))        # cases on one net share one batch: the first B rows of it
        x = rng.uniform(-0.9, 1.5, size=(nb, D))
        if self.kind == "regions":
            x[:, :2] = rng.uniform(-1.0, 2.0, size=(nb, 2))
        if gate_lo is not None:
            x[:, :ns] = rng.uniform(gate_lo, gate_hi, size=(nb, ns))
        self.x = np.ascontiguousarray(x[:self.B].astype(np.float32))
        self.g = np.ascontiguousarray(rng.normal(size=(nb, O))[:self.B].astype(np.float32))
        if spec.get("on_centres"):           # three queries that ARE centres
            cc = self.params["params"]["rbf_list"]["centers"]
            k0, k1 = (0, 1) if K == 3 else (3, 17)
            self.x[5], self.x[20], self.x[self.B - 1] = cc[0, k0], cc[0, k1], cc[0, K - 1]
        poison = spec.get("poison")
        if poison == "nan_g":
            self.g[17, 1] = np.nan
        elif poison == "nan_x":
            self.x[23, 3] = np.nan           # an ungated coordinate
        elif poison == "inf_g":
            self.g[40, 2] = np.inf

    def gamma(self, dtype=np.float64):
        return softmax_gate(self.params, self.x, dtype) if self.cluster else tanh_gate(self.cfg, self.x, dtype)

    def plan(self):
        return k2_plan(self.N, self.B, self.D, self.O, self.basis, self.gated)

    def reference(self):
        return vjp_reference(self.basis, self.params, self.x, self.g, self.gamma())

    def yardstick(self):
        return vjp_float32(self.basis, self.params, self.x, self.g, self.gamma(np.float32))


def _one(tag, D, O, K, basis, B, ns=0, **kw):
    return dict(tag=tag, kind="one", D=D, O=O, K=K, basis=basis, B=B, ns=ns, **kw)


def _reg(tag, grid, D, O, K, basis, B, **kw):
    return dict(tag=tag, kind="regions", grid=grid, D=D, O=O, K=K, basis=basis, B=B, **kw)


def _clu(tag, D, O, R, K, basis, B):
    return dict(tag=tag, kind="cluster", D=D, O=O, R=R, K=K, basis=basis, B=B)


BATCH_EDGES = (1, 2, 5, 63, 64, 65, 255, 256, 257, 513, 1021)
BIAS_EDGES = (16383, 16384, 16385)

# Every D from 1 to 8 (DC = 3, 3, 3, 4, 7, 7, 7, 8), every compiled OP at both pad edges (O = OP and O = previous OP + 1), the four
# basis classes without and with per-lane region weights, N = 1, 33, 63, 64, 65, 130 centres.
SHAPES = [
    _one("d1_o1_n1", 1, 1, 1, "gaussian", 70, ns=1),
    _one("d2_o2_n33", 2, 2, 33, "inverse_quadratic", 200, ns=1),                 # nsplit < D
    _one("d3_o3_n63", 3, 3, 63, "inverse_multiquadric", 300),
    _one("d4_o4_n64", 4, 4, 64, "multiquadric", 257),
    _one("d5_o5_n65", 5, 5, 65, "gaussian_wide", 600, ns=2),                     # nsplit < D; odd OP: the h-bar loop's tail
    _one("d6_o6_n130", 6, 6, 130, "matern52", 130),
    _one("d7_o8", 7, 8, 100, "gaussian", 513, ns=7),
    _one("d8_o9", 8, 9, 40, "inverse_quadratic", 100),
    _one("d3_o10", 3, 10, 200, "inverse_multiquadric", 400, ns=3),
    _one("d4_o11", 4, 11, 70, "gaussian_wide", 90),
    _one("d7_o16", 7, 16, 90, "inverse_quadratic", 320),
    _one("d8_o17", 8, 17, 50, "gaussian", 150),
    _one("d5_o32", 5, 32, 66, "inverse_multiquadric", 260),
    _one("d2_o33", 2, 33, 40, "gaussian", 64),
    _one("d6_o65", 6, 65, 20, "inverse_quadratic", 120),
    _one("d1_o101", 1, 101, 30, "gaussian_wide", 77),
]
# the launches above 64 KiB of LDS; O = 100 against one centre group: the reduce grid is O blocks wide; B = 300: two rows per
# sweep of the bias partials, threads idle at O = 100
WIDE = [
    _one("wide_d8_o64", 8, 64, 130, "gaussian", 300),
    _one("wide_d7_o100", 7, 100, 50, "gaussian", 300, ns=2),
    _one("wide_d8_o128", 8, 128, 130, "gaussian", 300),
]
REGIONS = [
    _reg("r2", (2, 1), 3, 5, 5, "gaussian_wide", 200),
    _reg("r63", (9, 7), 4, 2, 3, "inverse_quadratic", 500),
    _reg("r64", (8, 8), 5, 3, 4, "inverse_multiquadric", 500),
    _reg("r65", (13, 5), 7, 10, 3, "multiquadric", 500),
    _reg("r130", (13, 10), 8, 4, 5, "matern52", 600),
    _reg("r6_rows4", (3, 2), 2, 8, 4, "gaussian", 300, rows=4),                  # n_ranges < R
    dict(tag="r6_tiny", kind="tiny", D=3, O=5, K=5, basis="gaussian", B=400),
]
CLUSTER = [
    _clu("clu_d5_o3_r7", 5, 3, 7, 4, "gaussian", 300),
    _clu("clu_d8_o10_r65", 8, 10, 65, 3, "inverse_quadratic", 300),
    _clu("clu_d3_o5_r1", 3, 5, 1, 33, "gaussian", 300),
]
# delta = 2.5 on the 4-region net: no factor of the gate below float32's exact zero, however few the queries
BATCH = [_one(f"b{B}_r1", 3, 5, 100, "gaussian", B, net="batch_r1", draw=1021) for B in BATCH_EDGES] + \
        [_reg(f"b{B}_r4", (2, 2), 4, 4, 20, "inverse_quadratic", B, net="batch_r4", draw=1021, delta=2.5) for B in BATCH_EDGES]
BIAS = [_one(f"bias_b{B}", 3, 5, 10, "gaussian_wide", B, net="bias", draw=16385) for B in BIAS_EDGES]
REUSE = [_one("reuse_b65", 4, 10, 150, "gaussian", 65, net="reuse", draw=4096)]
NONFINITE = [_one(f"nonfinite_{p}", 5, 3, 70, "gaussian_wide", 130, ns=2, net="nonfinite", poison=p) for p in ("nan_g", "nan_x", "inf_g")]
ON_CENTRES = [_one(f"on_centres_{b}", 3, 5, 40, b, 64, ns=1, on_centres=True) for b in ("gaussian", "inverse_quadratic", "inverse_multiquadric")]
# the bases in d itself, every centre under a query: d centers is NaN (sqrt has no derivative at 0), d log_sigs finite
D_BASES = ("linear", "spline", "poisson_one", "poisson_two", "matern32", "matern52")
ON_CENTRES_D = [_one(f"on_centres_{b}", 3, 2, 3, b, 65, ns=1, on_centres=True) for b in D_BASES]
TABLE = SHAPES + WIDE + REGIONS + CLUSTER + BATCH + BIAS + REUSE + NONFINITE + ON_CENTRES + ON_CENTRES_D


# ------------------------------------------------------------------------------------------------ the bounds
def ratios(got, ref, S):
    """(worst |err| / S over the finite elements of ref, max|err| / (5e-5 max|ref| + 1e-7)); elements with S = 0 count through
    the absolute term of the bound: ATOL_S / C_S is added to S."""
    fin = np.isfinite(ref)
    if not fin.any():
        return 0.0, 0.0
    err = np.abs(np.asarray(got, np.float64)[fin] - ref[fin])
    if not np.isfinite(err).all():
        return float("inf"), float("inf")
    return float((err / (S[fin] + ATOL_S / C_S)).max()), float(err.max() / (MAXNORM_REL * np.abs(ref[fin]).max() + MAXNORM_ABS))


def same_nonfinite(got, ref):
    """NaN where the reference has NaN, +-Inf where it has +-Inf, finite elsewhere."""
    got = np.asarray(got, np.float64)
    inf = np.isinf(ref)
    return bool(np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), inf) and
                np.array_equal(np.sign(got[inf]), np.sign(ref[inf])))
