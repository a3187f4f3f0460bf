"""Helpers of tests/test_f64_reference_cpu.py and tests/test_gpu_f64_kernels.py: the float64 kernels (irbfn_amd/csrc/rbf_f64.hip:
gate, forward, parameter VJP with its slab reduce and bias column sums, x-VJP) on their own.  NumPy only: nothing here needs a GPU.

The statement is in np.longdouble (64-bit mantissa), so that it is more precise than what it judges:
  forward_ref(case)  out[b,o] = sum_r gamma[b,r] sum_k phi[b,r,k] W[k,o] + bias[o]
  vjp_ref(case)      the four gradient formulas at the head of rbf_vjp.hip (tests/_k2_util.py::_terms, which is dtype-generic)
  vjpx_ref(case)     the formula of rbf_vjpx.h, with the slopes of rbf_basis.h's basis_value_slope_finite (restated here and not
                     taken from tests/_vjpx_util.py::hand_gx, which has no S_gamma and no error term of its gate)
each -> {name: (value, S, S_gamma)}.  The gate is 1 / (1 + exp(-2 z)) per half-factor: the same number as (tanh z + 1) / 2 without
the cancellation of tanh(z) + 1.  Regions without a row of dimension_ranges get gamma = 0; with nsplit = 0 every region with a row
gets gamma = 1.

S        the sum of the absolute values of the terms the element is made of (the forward adds |bias|): what a rounding error of
         that element is to be read against.
S_gamma  the same sum with |delta gamma| in place of gamma.  The kernels evaluate a half-factor as (tanh(z) + 1) / 2 in float64: a
         tanh within one ulp of a value in (-1, 1) is off by at most 2^-53, the add rounds at 2^-54 or less, the halving is exact,
         so a half-factor carries an ABSOLUTE error eps_gate = 2^-53 however small it is, and the product of the 2 nsplit
         half-factors of a region is off by at most  prod(h_i + eps_gate) - prod(h_i) = delta gamma.
         The x-VJP also uses d log gamma_r / d x_d = delta_d (tanh z2 - tanh z1) from the same two tanh: its absolute error is at
         most 2 delta_d eps_gate, and the term (gamma + delta gamma) |q| 2 delta_d eps_gate is part of the x-VJP's S_gamma.

The bound, on every finite element of the statement:
    |got - ref| <= C64 * 2^-53 * S + S_gamma + 1e-300,      C64 = 4 * R64
R64 is the worst max(|y - ref| - S_gamma, 0) / (2^-53 S) over TABLE of y = the same formulas in plain float64 NumPy in the kernels'
tanh form of the gate, the sums over the queries sequential (np.cumsum).  The factor 4 is K2's (tests/_k2_util.py), for the same
reasons: another summation order (slices, a fixed-order reduce, a 256-tree for the bias), the device library's exp / tanh / log
instead of libm's, and d2 taken as (sqrt(r2) / sigma)^2."""
import zlib

import numpy as np

from _k2_util import D_BASES, LEAF_PATH, LEAVES, _terms, basis_terms, same_nonfinite  # noqa: F401  (same_nonfinite: re-exported)

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "np.longdouble has no 64-bit mantissa here: the statement would be no more precise than the kernels"

U53 = 2.0 ** -53
EPS_GATE = 2.0 ** -53
ATOL = 1e-300
# worst max(|y - ref| - S_gamma, 0) / (2^-53 S) of yardstick() over TABLE, rounded up to two digits; np.exp / np.tanh may differ in the
# last bit between CPUs.  tests/test_f64_reference_cpu.py::test_yardstick_and_the_coefficient recomputes it and prints the case.
R64 = 5.6      # 5.54, set by b_poisson_two, x-VJP (gx)
C64 = 4 * R64
OPS = ("fwd", "vjp", "vjpx")
BASES = ("gaussian", "gaussian_wide", "gaussian_wider", "inverse_quadratic", "linear", "quadratic", "multiquadric",
         "inverse_multiquadric", "spline", "poisson_one", "poisson_two", "matern32", "matern52")
F64_OT, F64_LDS_LIMIT = 16, 64 * 1024            # kF64OT; the gate table's LDS limit in bytes


def _cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ the launch
def f64_plan(N, B, D, R, O):
    """f64_slices, per_slice, Npad and irbfn_f64_workspace_bytes restated; `empty`: the slices that own no query (b0 >= B) and
    still have to write zero slabs."""
    groups = _cdiv(N, 64)
    slices = max(1, min(_cdiv(4096, groups), _cdiv(B, 64), 1024))
    per_slice, Npad = _cdiv(B, slices), groups * 64
    gamma_bytes = _cdiv(8 * B * R, 256) * 256
    return {"groups": groups, "slices": slices, "per_slice": per_slice, "Npad": Npad,
            "empty": sum(1 for q in range(slices) if q * per_slice >= B),
            "bytes_fwd": gamma_bytes, "bytes_vjp": gamma_bytes + slices * (D + 1 + O) * Npad * 8}


def gate_lds_bytes(nsplit, max_ranges):
    return max(nsplit, 1) * max(max_ranges, 1) * 64 * 8


# ------------------------------------------------------------------------------------------------ the cases
class Case:
    """One row of TABLE with its inputs in float64, not rounded to float32: cfg (a WCRBFNet card), params, x[B, D], g[B, O]."""

    def __init__(self, spec):
        self.spec, self.tag, self.kind, self.ops = spec, spec["tag"], spec["kind"], spec["ops"]
        self.D, self.O, self.K, self.basis, self.B = spec["D"], spec["O"], spec["K"], spec["basis"], spec["B"]
        rng = np.random.default_rng(zlib.crc32(("f64:" + spec.get("net", self.tag)).encode()))
        D, O, K = self.D, self.O, self.K
        cfg = {"in_features": D, "out_features": O, "num_kernels": K, "basis_func": self.basis}
        gate_lo = gate_hi = None                  # where the queries' gated coordinates are drawn
        ea = eb = None
        if self.kind == "one":                    # R regions (1 unless said) with the same wide box on the first ns coordinates
            ns, R = spec.get("ns", 0), spec.get("R", 1)
            cfg.update(lower_bounds=[[-1.5]] * ns, upper_bounds=[[2.1]] * ns, dimension_ranges=[[0] * ns] * R, delta=[8.0] * ns)
        elif self.kind == "regions":              # a x b boxes over the first two coordinates, region (i, j) = ranges i and j
            (a, b), ns = spec["grid"], 2
            R = a * b
            ea, eb = np.linspace(-1.0, 2.0, a + 1), np.linspace(-1.0, 2.0, b + 1)
            cfg.update(lower_bounds=[ea[:-1].tolist(), eb[:-1].tolist()], upper_bounds=[ea[1:].tolist(), eb[1:].tolist()],
                       dimension_ranges=[[i, j] for i in range(a) for j in range(b)], delta=[spec.get("delta", 20.0)] * 2)
            R = spec.get("R", R)                  # fewer regions than rows: n_ranges > R; `rows`: fewer rows than regions
            cfg["dimension_ranges"] = cfg["dimension_ranges"][:spec.get("rows", len(cfg["dimension_ranges"]))]
        elif self.kind == "tiny":                 # _k2_util's r6_tiny: every query in the first box, the others weigh 1e-7 .. 1e-14
            ns, R = 2, 6
            cfg.update(lower_bounds=[[-1.0, 0.85]] * 2, upper_bounds=[[0.5, 2.0]] * 2,
                       dimension_ranges=[[0, 0], [0, 1], [1, 0], [1, 1], [1, 0], [0, 1]], delta=[10.0, 10.0])
            gate_lo, gate_hi = 0.0, 0.1
        elif self.kind == "steep":                # delta = 15 on coordinate 0: [-1, 0], [0, 1], [1, 2] and a range no query reaches
            ns, R = 1, 4
            cfg.update(lower_bounds=[[-1.0, 0.0, 1.0, 5.0]], upper_bounds=[[0.0, 1.0, 2.0, 6.0]],
                       dimension_ranges=[[0], [1], [2], [3]], delta=[15.0])
        elif self.kind == "lds":                  # ns split coordinates with mr nested ranges each: ns * mr entries of the gate table
            ns, mr, R = spec["ns"], spec["mr"], 3
            lo = [[-1.5 - 0.05 * i for i in range(mr)]] * ns
            hi = [[2.1 + 0.05 * i for i in range(mr)]] * ns
            cfg.update(lower_bounds=lo, upper_bounds=hi, delta=[4.0] * ns,
                       dimension_ranges=[[(5 * r + 3 * d) % mr for d in range(ns)] for r in range(R)])
        else:
            raise ValueError(self.kind)
        self.R, self.N, self.ns = R, R * K, ns
        cfg.update(num_regions=R, activation_idx=list(range(ns)))
        self.cfg = cfg
        ls_lo = 0.2 if self.basis == "gaussian" else -0.5          # the widths of _k2_util's table
        c = rng.uniform(-1.0, 1.6, size=(R, K, D))
        if self.kind == "regions":
            for r in range(R):
                i, j = divmod(r, spec["grid"][1])
                c[r, :, 0] = rng.uniform(ea[i] - 0.1, ea[i + 1] + 0.1, size=K)
                c[r, :, 1] = rng.uniform(eb[j] - 0.1, eb[j + 1] + 0.1, size=K)
        if self.kind == "tiny":
            c = rng.uniform(-0.5, 0.6, size=(R, K, D))
        self.params = {"params": {"rbf_list": {"centers": c, "log_sigs": rng.uniform(ls_lo, 1.0, size=(R, K))},
                                  "linear": {"kernel": rng.normal(size=(K, O)) * 0.5, "bias": rng.normal(size=(O,))}}}
        if spec.get("small_column") is not None:  # an output column with small weights
            self.params["params"]["linear"]["kernel"][:, spec["small_column"]] *= 1e-9
        nb = max(self.B, spec.get("draw", self.B))                 # cases on one net share one batch: the first B rows of it
        x = rng.uniform(-0.9, 1.5, size=(nb, D))
        if self.kind == "regions":
            x[:, :2] = rng.uniform(-1.0, 2.0, size=(nb, 2))
        if self.kind == "steep":
            x[:, 0] = rng.uniform(-1.0, 2.0, size=nb)
            x[7, 0], x[11, 0] = -3.0, 3.5         # every half-product of these two is exactly 0 in float64
            x[13, 0], x[17, 0] = 1e-3, 0.999      # and these sit on a bound
        if gate_lo is not None:
            x[:, :ns] = rng.uniform(gate_lo, gate_hi, size=(nb, ns))
        self.x = np.ascontiguousarray(x[:self.B])
        self.g = np.ascontiguousarray(rng.normal(size=(nb, O))[:self.B])
        assert self.x.dtype == np.float64 and self.g.dtype == np.float64
        self.on = ()
        if spec.get("on_centres"):                # three queries that ARE centres
            k0, k1 = (0, 1) if K == 3 else (3, 17)
            self.on = ((5, k0), (20, k1), (self.B - 1, K - 1))
            for b, k in self.on:
                self.x[b] = c[0, k]
        poison = spec.get("poison")
        if poison == "nan_g":
            self.g[17, 1] = np.nan
        elif poison == "nan_x":
            self.x[23, 3] = np.nan                # an ungated coordinate
        elif poison == "inf_g":
            self.g[40, 2] = np.inf

    def plan(self):
        return f64_plan(self.N, self.B, self.D, self.R, self.O)

    def tables(self, pad=0.0, n_ranges=None):
        """The gate tables of irbfn_f64_card -> (nsplit, max_ranges, lo[ns, mr], hi[ns, mr], delta[ns], dim_ranges[rows, ns],
        n_ranges).  The entries of lo / hi past a coordinate's own ranges are `pad`; n_ranges: None clamps the rows of
        dimension_ranges to R as WCRBFNet does, a number is passed on as it is (with every row of dimension_ranges in the table)."""
        cfg, ns = self.cfg, self.ns
        mr = max([1] + [len(cfg["lower_bounds"][d]) for d in range(ns)])
        lo, hi = np.full((max(ns, 1), mr), pad, np.float64), np.full((max(ns, 1), mr), pad, np.float64)
        for d in range(ns):
            lo[d, :len(cfg["lower_bounds"][d])] = cfg["lower_bounds"][d]
            hi[d, :len(cfg["upper_bounds"][d])] = cfg["upper_bounds"][d]
        delta = np.asarray(cfg["delta"][:ns] if ns else [0.0], np.float64)
        rows = cfg["dimension_ranges"] if n_ranges is not None else cfg["dimension_ranges"][:self.R]
        dr = np.asarray([r[:ns] for r in rows], np.int32).reshape(len(rows), ns)
        return ns, mr, lo, hi, delta, np.ascontiguousarray(dr), len(rows) if n_ranges is None else n_ranges

    def half_z(self):
        """Every z = delta (x - lo), delta (hi - x) of the half-factors the regions use, float64 [B, rows, 2 ns]."""
        cfg = self.cfg
        out = []
        for row in cfg["dimension_ranges"][:self.R]:
            for d in range(self.ns):
                lo, hi, dl = cfg["lower_bounds"][d][row[d]], cfg["upper_bounds"][d][row[d]], cfg["delta"][d]
                out += [dl * (self.x[:, d] - lo), dl * (hi - self.x[:, d])]
        return np.stack(out, 1) if out else np.zeros((self.B, 0))


# ------------------------------------------------------------------------------------------------ the formulas
def gate(case, dtype=LD, tanh_form=False):
    """-> gamma[B,R], dgam[B,R] = prod(h + eps_gate) - prod(h), dlog[B,R,D] = d log gamma_r / d x_d, ddlog[B,R,D] = 2 delta_d
    eps_gate on the gated coordinates of a region with a row.  tanh_form: the kernels' expressions, (tanh(z) + 1) / 2 and
    delta (tanh z2 - tanh z1); otherwise 1 / (1 + exp(-2 z)) and 2 delta (1 / (1 + exp(2 z1)) - 1 / (1 + exp(2 z2)))."""
    dt = np.dtype(dtype).type
    cfg, x = case.cfg, np.asarray(case.x).astype(dt)
    B, D = x.shape
    R, ns = case.R, case.ns
    one, two, eps = dt(1), dt(2), dt(EPS_GATE)
    fac, fac_e, dlg = [], [], []
    with np.errstate(all="ignore"):
        for d in range(ns):
            lo, hi = np.asarray(cfg["lower_bounds"][d]).astype(dt), np.asarray(cfg["upper_bounds"][d]).astype(dt)
            dl = dt(cfg["delta"][d])
            z1, z2 = dl * (x[:, d, None] - lo[None]), dl * (hi[None] - x[:, d, None])
            if tanh_form:
                t1, t2 = np.tanh(z1), np.tanh(z2)
                a, b, dd = (t1 + one) / two, (t2 + one) / two, dl * (t2 - t1)
            else:
                a, b = one / (one + np.exp(-two * z1)), one / (one + np.exp(-two * z2))
                dd = two * dl * (one / (one + np.exp(two * z1)) - one / (one + np.exp(two * z2)))
            fac.append(a * b)
            fac_e.append((a + eps) * (b + eps))
            dlg.append(dd)
        gamma, gam_e = np.zeros((B, R), dt), np.zeros((B, R), dt)
        dlog, ddlog = np.zeros((B, R, D), dt), np.zeros((B, R, D), dt)
        for r, row in enumerate(cfg["dimension_ranges"][:R]):
            cur, cur_e = np.ones(B, dt), np.ones(B, dt)
            for d in range(ns):
                cur, cur_e = cur * fac[d][:, row[d]], cur_e * fac_e[d][:, row[d]]
                dlog[:, r, d] = dlg[d][:, row[d]]
                ddlog[:, r, d] = two * dt(cfg["delta"][d]) * eps
            gamma[:, r], gam_e[:, r] = cur, cur_e
    return gamma, gam_e - gamma, dlog, ddlog


def basis_finite(name, u):
    """(phi, d phi / d(d2)) in the x-VJP's convention (rbf_basis.h, basis_value_slope_finite): for a query ON a centre spline, matern32
    and matern52 take their finite limit and linear, poisson_one and poisson_two give 0."""
    phi, dphi, _ = basis_terms(name, u)
    limit = {"linear": 0.0, "poisson_one": 0.0, "poisson_two": 0.0, "spline": 0.0, "matern32": -1.5, "matern52": -5.0 / 6.0}
    if name in limit:
        dphi = np.where(u == 0, u.dtype.type(limit[name]), dphi)
    return phi, dphi


def _leaves(case, dt):
    p = case.params["params"]
    return tuple(np.asarray(p[a][b]).astype(dt) for a, b in (LEAF_PATH[n] for n in LEAVES))


def _pairs(case, dt):
    """diff[B,R,K,D], s2[1,R,K], d2[B,R,K] at dt."""
    c, ls, _, _ = _leaves(case, dt)
    diff = np.asarray(case.x).astype(dt)[:, None, None, :] - c[None]
    s2 = np.exp(dt(-2) * ls)[None]
    return diff, s2, (diff * diff).sum(-1) * s2


def forward_terms(case, dtype=LD, tanh_form=False):
    """-> (out, S, S_gamma), each [B, O]."""
    dt = np.dtype(dtype).type
    with np.errstate(all="ignore"):
        _, _, W, bias = _leaves(case, dt)
        gam, dgam, _, _ = gate(case, dt, tanh_form)
        phi = basis_terms(case.basis, _pairs(case, dt)[2])[0]
        out = (gam[:, :, None] * phi).sum(1) @ W + bias
        S = (gam[:, :, None] * np.abs(phi)).sum(1) @ np.abs(W) + np.abs(bias)
        Sg = (dgam[:, :, None] * np.abs(phi)).sum(1) @ np.abs(W)
    return out, S, Sg


def vjp_terms(case, dtype=LD, tanh_form=False, sequential=False):
    """-> {leaf: (grad, S, S_gamma)}.  sequential: every sum over the queries one after the other (np.cumsum), then the regions."""
    dt = np.dtype(dtype).type
    seq = (lambda a: np.cumsum(a, axis=0, dtype=dt)[-1]) if sequential else (lambda a: a.sum(0))
    with np.errstate(all="ignore"):
        gam, dgam, _, _ = gate(case, dt, tanh_form)
        tc, tl, h, g = _terms(case.basis, case.params, case.x, case.g, gam, dt)
        if sequential:
            kern = seq(seq(h[:, :, :, None] * g[:, None, None, :]))          # [B,R,K,O]: the queries, then the regions
        else:
            kern = h.sum(1).T @ g
        ec, el, eh, _ = _terms(case.basis, case.params, case.x, case.g, dgam, dt)
        ag = np.abs(g)
        return {"centers": (seq(tc), np.abs(tc).sum(0), np.abs(ec).sum(0)),
                "log_sigs": (seq(tl), np.abs(tl).sum(0), np.abs(el).sum(0)),
                "kernel": (kern, np.abs(h).sum(1).T @ ag, np.abs(eh).sum(1).T @ ag),
                "bias": (seq(g), ag.sum(0), np.zeros(g.shape[1], dt))}


def vjpx_terms(case, dtype=LD, tanh_form=False):
    """-> (gx, S, S_gamma), each [B, D]: gx[b,d] = sum_r gamma (sum_k 2 hbar f'(u) sigma^-2 (x_d - c_d) + q dlog_rd), hbar = g W^T,
    q[b,r] = sum_k hbar phi."""
    dt = np.dtype(dtype).type
    with np.errstate(all="ignore"):
        _, _, W, _ = _leaves(case, dt)
        gam, dgam, dlog, ddlog = gate(case, dt, tanh_form)
        diff, s2, u = _pairs(case, dt)
        phi, fp = basis_finite(case.basis, u)
        hb = np.asarray(case.g).astype(dt) @ W.T                         # [B,K]
        core = dt(2) * hb[:, None, :] * fp * s2                           # [B,R,K]
        rb, rba = (core[..., None] * diff).sum(2), (np.abs(core)[..., None] * np.abs(diff)).sum(2)     # [B,R,D]
        q, qa = (hb[:, None, :] * phi).sum(-1), (np.abs(hb)[:, None, :] * np.abs(phi)).sum(-1)          # [B,R]
        gx = (gam[:, :, None] * rb).sum(1) + ((gam * q)[:, :, None] * dlog).sum(1)
        S = (gam[:, :, None] * rba).sum(1) + ((gam * qa)[:, :, None] * np.abs(dlog)).sum(1)
        Sg = (dgam[:, :, None] * rba).sum(1) + ((dgam * qa)[:, :, None] * np.abs(dlog)).sum(1) + \
             (((gam + dgam) * qa)[:, :, None] * ddlog).sum(1)
    return gx, S, Sg


def reference(case, op):
    """The statement -> {name: (value, S, S_gamma)} in np.longdouble; name is "out", "gx" or a gradient leaf."""
    if op == "fwd":
        return {"out": forward_terms(case)}
    if op == "vjpx":
        return {"gx": vjpx_terms(case)}
    return vjp_terms(case)


def yardstick(case, op):
    """The same formulas in plain float64, the gate in the kernels' tanh form, the sums over the queries sequential -> {name: value}."""
    f = np.float64
    if op == "fwd":
        out = {"out": forward_terms(case, f, True)[0]}
    elif op == "vjpx":
        out = {"gx": vjpx_terms(case, f, True)[0]}
    else:
        out = {n: v[0] for n, v in vjp_terms(case, f, True, sequential=True).items()}
    assert all(v.dtype == f for v in out.values())
    return out


# ------------------------------------------------------------------------------------------------ the bound
def bound(S, Sg, coef=None):
    return (C64 if coef is None else coef) * LD(U53) * S + Sg + LD(ATOL)


def ratio(got, ref, S, Sg):
    """worst |got - ref| / (C64 2^-53 S + S_gamma + 1e-300) over the finite elements of the statement."""
    fin = np.isfinite(ref)
    if not fin.any():
        return 0.0
    err = np.abs(np.asarray(got).astype(LD)[fin] - ref[fin])
    if not np.isfinite(err).all():
        return float("inf")
    return float((err / bound(S[fin], Sg[fin])).max())


def needed(got, ref, S, Sg):
    """worst max(|got - ref| - S_gamma, 0) / (2^-53 S) over the finite elements of the statement: what R64 is the largest of."""
    fin = np.isfinite(ref) & (S > 0)
    if not fin.any():
        return 0.0
    err = np.abs(np.asarray(got).astype(LD)[fin] - ref[fin])
    return float((np.maximum(err - Sg[fin], 0) / (LD(U53) * S[fin])).max())


# ------------------------------------------------------------------------------------------------ the table
ALL, NO_VJP = OPS, ("fwd", "vjpx")


def _one(tag, D, O, K, basis, B, ns=0, ops=ALL, **kw):
    return dict(tag=tag, kind="one", D=D, O=O, K=K, basis=basis, B=B, ns=ns, ops=ops if O <= F64_OT else NO_VJP, **kw)


def _reg(tag, grid, D, O, K, basis, B, ops=ALL, **kw):
    return dict(tag=tag, kind="regions", grid=grid, D=D, O=O, K=K, basis=basis, B=B, ops=ops, **kw)


# Every D from 1 to 8; forward O in {1, 2, 15, 16, 17, 32, 33} (the output tile loop, kF64OT = 16), VJP O in {1, 2, 5, 15, 16},
# x-VJP O in {1, 16, 17, 33} (the cotangent row in registers or not); N = 1, 33, 63, 64, 65, 130 centres (the VJP's lane-per-centre
# padding); nsplit = 0, nsplit < D, nsplit = D; the four basis classes spread over these edges.
SHAPES = [
    _one("d1_o1_n1", 1, 1, 1, "gaussian", 70, ns=1),
    _one("d2_o2_n33", 2, 2, 33, "inverse_quadratic", 200, ns=1),                  # nsplit < D
    _one("d3_o5_n63", 3, 5, 63, "inverse_multiquadric", 130),                     # nsplit = 0, R = 1
    _one("d4_o15_n64", 4, 15, 64, "multiquadric", 257, ns=4),                     # nsplit = D
    _one("d5_o16_n65", 5, 16, 65, "gaussian_wide", 300, ns=2),
    _one("d6_o17_n130", 6, 17, 130, "matern52", 130),
    _one("d7_o32", 7, 32, 40, "gaussian_wider", 100, ns=7),
    _one("d8_o33", 8, 33, 50, "spline", 150, ns=3),
    _one("d6_o16_n130", 6, 16, 130, "inverse_quadratic", 129, ns=1),
    _one("d7_o2_n65", 7, 2, 65, "inverse_multiquadric", 64),
    _one("d8_o1_n63", 8, 1, 63, "gaussian", 65, ns=8),
    _one("d3_o17_small_column", 3, 17, 20, "gaussian", 90, ns=1, small_column=16),   # an output column with weights of 1e-9
    _one("r2_nsplit0", 4, 5, 17, "inverse_quadratic", 100, R=2),                  # nsplit = 0, R = 2: both regions weigh 1
]
# the bases the shapes above leave out, each at all three operations
BASIS_CASES = [
    _one("b_linear", 8, 16, 20, "linear", 90, ns=1),
    _one("b_quadratic", 7, 1, 30, "quadratic", 65),
    _one("b_poisson_one", 6, 2, 10, "poisson_one", 64, ns=2),
    _one("b_poisson_two", 4, 15, 12, "poisson_two", 63),
    _one("b_matern32", 1, 5, 7, "matern32", 129, ns=1),
    _one("b_matern52", 2, 16, 9, "matern52", 66, ns=2),
    _one("b_gaussian_wider", 5, 1, 33, "gaussian_wider", 70),
    _one("b_spline", 3, 2, 11, "spline", 131, ns=1),
]
REGIONS = [
    _reg("r2", (2, 1), 3, 5, 5, "gaussian_wide", 200),
    _reg("r63", (9, 7), 4, 2, 2, "inverse_quadratic", 300),
    _reg("r64", (8, 8), 5, 3, 2, "inverse_multiquadric", 300),
    _reg("r65", (13, 5), 7, 10, 2, "multiquadric", 300),                          # N = 130
    _reg("r6_rows4", (3, 2), 2, 8, 4, "gaussian", 300, rows=4),                   # n_ranges < R; 3 and 2 ranges: a ragged table
    _reg("r4_rows6", (3, 2), 2, 8, 4, "gaussian", 300, R=4),                      # n_ranges > R once every row is handed over
    dict(tag="r6_tiny", kind="tiny", D=3, O=5, K=5, basis="gaussian", B=400, ops=ALL),
    dict(tag="steep", kind="steep", D=3, O=2, K=5, basis="gaussian", B=200, ops=ALL),
]
LDS = [
    dict(tag="lds_128", kind="lds", ns=8, mr=16, D=8, O=2, K=4, basis="gaussian_wide", B=70, ops=ALL),       # exactly 64 KiB
    dict(tag="lds_129", kind="lds", ns=3, mr=43, D=4, O=2, K=4, basis="gaussian_wide", B=70, ops=("vjpx",)),  # 129 entries: refused
]
BATCH_EDGES = (1, 2, 63, 64, 65, 129, 255, 256, 257, 600)
BATCH = [_reg(f"b{B}", (2, 2), 4, 5, 10, "inverse_quadratic", B, net="batch", draw=600, delta=6.0) for B in BATCH_EDGES]
# f64_slices at its caps, N = 3: 1024 slices of 64; the cap 1024 binds with 15 and with 8 slices behind the batch; N = 449:
# ceil(B / 64) = 10 binds below 4096 / 8 groups = 512
SLICES = [_one(f"slices_b{B}", 3, 2, 3, "inverse_quadratic", B, ops=("vjp",), net="slices", draw=66000) for B in (65536, 65537, 66000)] + \
         [_one("slices_n449", 3, 2, 449, "gaussian_wide", 600, ops=("vjp",))]
NONFINITE = [_one("nonfinite_nan_x", 5, 3, 70, "gaussian_wide", 130, ns=2, net="nonfinite", poison="nan_x")] + \
            [_one(f"nonfinite_{p}", 5, 3, 70, "gaussian_wide", 130, ns=2, ops=("vjp", "vjpx"), net="nonfinite", poison=p)
             for p in ("nan_g", "inf_g")]
ON_CENTRES = [_one(f"on_centres_{b}", 3, 5, 40, b, 64, ns=1, on_centres=True) for b in ("gaussian", "inverse_quadratic", "inverse_multiquadric")]
# the bases in d itself, every centre under a query: d centers is NaN (sqrt has no derivative at 0), d log_sigs finite, gx finite
ON_CENTRES_D = [_one(f"on_centres_{b}", 3, 2, 3, b, 65, ns=1, on_centres=True) for b in D_BASES]
TABLE = SHAPES + BASIS_CASES + REGIONS + LDS + BATCH + SLICES + NONFINITE + ON_CENTRES + ON_CENTRES_D
BY_TAG = {s["tag"]: s for s in TABLE}
assert len(BY_TAG) == len(TABLE)


def tags(op, rows=TABLE):
    return [s["tag"] for s in rows if op in s["ops"]]
