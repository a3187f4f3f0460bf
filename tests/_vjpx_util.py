"""Helpers of the query-VJP tests (test_vjpx_cpu.py, test_gpu_vjpx.py).  A plain module: no fixtures, no hooks.

``ref_gx``   the reference: torch.autograd of the float64 restatement (oracle/irbfn_oracle.py), in row chunks.  It goes through
             ``(sum sq) ** 0.5`` and is NaN for a query exactly on a centre.
``hand_gx``  the formula of irbfn_amd/csrc/rbf_vjpx.h in NumPy at a chosen dtype -- float64 for queries on a centre, float32 as
             "the reference arithmetic at the kernel's precision" -- and S[b,d], the sum of the absolute values of the terms the
             gradient is made of (the counterpart of the forward tests' sum |h_k W_ko|):

    S[b,d] = 2 sum_{r,k} |s[b,r,k]| |x_d - c_d|  +  sum_r gamma[b,r] |dlog_rd| sum_k |hbar[b,k] phi[b,r,k]|,
    s = hbar gamma f'(u) sigma^-2,  hbar = gout W^T.

The rounding errors of a float32 evaluation are relative to those terms, so |gx - ref| <= c S with c a small multiple of 2^-24
that grows slowly with the length of the sums; profiles/vjp_x_parity.txt has the measured c.
"""
import itertools

import numpy as np
import torch

from oracle import irbfn_oracle as orc

BASES = ("gaussian", "gaussian_wide", "gaussian_wider", "inverse_quadratic", "linear", "quadratic", "multiquadric",
         "inverse_multiquadric", "spline", "poisson_one", "poisson_two", "matern32", "matern52")
SINGULAR_AT_CENTRE = ("linear", "poisson_one", "poisson_two")     # f'(u) = phi'(d) / (2 d) diverges at d = 0
CHUNK_ELEMS = 1 << 23          # elements of one chunk's [rows, R, K, D] difference tensor

# |gx - ref| <= RTOL |ref| + C_S * S.  C_S = 4 x the largest max |hand_gx(float32) - ref| / S over the cases of
# tests/test_gpu_vjpx.py (NumPy float32, not the kernel): profiles/vjp_x_parity.txt
RTOL = 1e-5
C_S = 4 * 7.1e-7


def inner(params):
    return params["params"] if "params" in params else params


def synth_net(seed, D=7, O=10, K=50, grid=(2, 2), basis="gaussian", extra_regions=0, delta=8.0, box=2.0, w_scale=0.3):
    """(cfg, params): a WCRBFNet card whose regions are the cells of a grid over the first len(grid) coordinates of
    [-box, box]^D (grid = () or all ones: one region; () has no split dimension at all), plus ``extra_regions`` regions beyond
    len(dimension_ranges) (gamma = 0, model.py:70).  float32 parameters, centres in the box, widths e^0.5 .. e^1.5."""
    rng = np.random.default_rng(seed)
    ns = len(grid)
    lower, upper = [], []
    for n in grid:
        edges = np.linspace(-box, box, n + 1)
        lower.append([float(v) for v in edges[:-1]])
        upper.append([float(v) for v in edges[1:]])
    dr = [list(t) for t in itertools.product(*[range(n) for n in grid])] if ns else [[]]
    R = len(dr) + extra_regions
    cfg = {"in_features": D, "out_features": O, "num_kernels": K, "basis_func": basis, "num_regions": R,
           "lower_bounds": lower, "upper_bounds": upper, "dimension_ranges": dr, "activation_idx": list(range(ns)),
           "delta": [float(delta)] * ns}
    params = {"params": {
        "rbf_list": {"centers": rng.uniform(-box, box, size=(R, K, D)).astype(np.float32),
                     "log_sigs": rng.uniform(0.5, 1.5, size=(R, K)).astype(np.float32)},
        "linear": {"kernel": (rng.normal(size=(K, O)) * w_scale).astype(np.float32),
                   "bias": (rng.normal(size=(O,)) * 0.1).astype(np.float32)}}}
    return cfg, params


def queries(seed, cfg, B, box=2.0, lo=None, hi=None):
    rng = np.random.default_rng(seed + 7919)
    D = cfg["in_features"]
    lo = -box if lo is None else lo
    hi = box if hi is None else hi
    return rng.uniform(lo, hi, size=(B, D)).astype(np.float32)


def cotangent(seed, B, O):
    return np.random.default_rng(seed + 104729).normal(size=(B, O)).astype(np.float32)


def min_scaled_distance(params, x):
    """min over (query, centre) of d = |x - c| / sigma, float64."""
    p = inner(params)
    c = np.asarray(p["rbf_list"]["centers"], np.float64).reshape(-1, x.shape[1])
    sg = np.exp(np.asarray(p["rbf_list"]["log_sigs"], np.float64)).reshape(-1)
    best = np.inf
    for i in range(0, x.shape[0], 256):
        d = np.sqrt(((np.asarray(x[i:i + 256], np.float64)[:, None, :] - c[None]) ** 2).sum(-1)) / sg[None]
        best = min(best, float(d.min()))
    return best


def _rows(cfg):
    return max(1, CHUNK_ELEMS // (cfg["num_regions"] * cfg["num_kernels"] * cfg["in_features"]))


def ref_gx(cfg, params, x, g, apply=None):
    """d sum(apply(x) * g) / d x by torch.autograd of the float64 restatement -> float64 [B,D].  apply: the oracle function
    (default ``orc.wcrbfnet_apply``; ``orc.deeper_wcrbfnet_apply`` for the deeper net), called as apply(cfg, tp, xt)."""
    apply = apply or orc.wcrbfnet_apply
    p = inner(params)
    tp = {"params": {k: {n: torch.tensor(np.asarray(v, np.float64)) for n, v in d.items()} for k, d in p.items()}}
    out = np.empty(x.shape, np.float64)
    c = _rows(cfg)
    for i in range(0, x.shape[0], c):
        xt = torch.tensor(np.asarray(x[i:i + c], np.float64), requires_grad=True)
        gt = torch.tensor(np.asarray(g[i:i + c], np.float64))
        (gx,) = torch.autograd.grad((apply(cfg, tp, xt) * gt).sum(), xt)
        out[i:i + c] = gx.numpy()
    return out


def _basis(u, name, dt):
    """(phi, f'(u)) at dtype dt; the singular bases return f' = 0 at u = 0 (the kernels' convention)."""
    d = np.sqrt(u)
    one, half = dt(1), dt(0.5)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv2d = np.where(d > 0, half / np.where(d > 0, d, one), dt(0))
    if name in ("gaussian", "gaussian_wide", "gaussian_wider"):
        a = dt({"gaussian": 1.0, "gaussian_wide": 0.1, "gaussian_wider": 0.01}[name])
        phi = np.exp(-a * u)
        return phi, -a * phi
    if name == "inverse_quadratic":
        phi = one / (one + u)
        return phi, -(phi * phi)
    if name == "inverse_multiquadric":
        phi = one / np.sqrt(one + u)
        return phi, -half * phi * phi * phi
    if name == "linear":
        return d, inv2d
    if name == "quadratic":
        return u, np.ones_like(u)
    if name == "multiquadric":
        phi = np.sqrt(one + u)
        return phi, half / phi
    if name == "spline":
        l = np.log(d + one)
        return u * l, l + half * d / (d + one)
    if name == "poisson_one":
        e = np.exp(-d)
        return (d - one) * e, (dt(2) - d) * e * inv2d
    if name == "poisson_two":
        e = np.exp(-d)
        return ((d - dt(2)) / dt(2)) * d * e, (dt(2) * d - one - half * u) * e * inv2d
    if name == "matern32":
        s3 = dt(np.sqrt(3.0))
        e = np.exp(-s3 * d)
        return (one + s3 * d) * e, dt(-1.5) * e
    if name == "matern52":
        s5 = dt(np.sqrt(5.0))
        e = np.exp(-s5 * d)
        return (one + s5 * d + dt(5.0 / 3.0) * u) * e, dt(-5.0 / 6.0) * (one + s5 * d) * e
    raise ValueError(name)


def _gate(cfg, x, dt):
    """gamma[B,R] (model.py:74-93) and dlog[B,R,D] = d log gamma_r / d x_d =
    delta_d [tanh(delta_d (hi - x_d)) - tanh(delta_d (x_d - lo))]."""
    B, D = x.shape
    R, ns = cfg["num_regions"], len(cfg["activation_idx"])
    fac, dlg = [], []
    for d in range(ns):
        lo, hi = np.asarray(cfg["lower_bounds"][d], dt), np.asarray(cfg["upper_bounds"][d], dt)
        dl = dt(cfg["delta"][d])
        z1, z2 = dl * (x[:, d, None] - lo[None]), dl * (hi[None] - x[:, d, None])
        # a = (tanh(z1) + 1) / 2 = 1 / (1 + exp(-2 z1)) and 1 - a = 1 / (1 + exp(2 z1)): the same numbers as the tanh form, without
        # its cancellations (tanh(z) + 1 for z << 0 and tanh(z2) - tanh(z1) deep inside a region lose every digit in float32;
        # the kernels evaluate the gate in this form too, rbf_forward.h) -- so that the float32 run of this formula measures
        # rounding in the sums, which is what the tests' constant stands for
        with np.errstate(over="ignore"):
            a, b = dt(1) / (dt(1) + np.exp(dt(-2) * z1)), dt(1) / (dt(1) + np.exp(dt(-2) * z2))
            na, nb = dt(1) / (dt(1) + np.exp(dt(2) * z1)), dt(1) / (dt(1) + np.exp(dt(2) * z2))
        fac.append(a * b)
        dlg.append(dt(2) * dl * (na - nb))
    gamma = np.zeros((B, R), dt)
    dlog = np.zeros((B, R, D), dt)
    for r, rng_ in enumerate(cfg["dimension_ranges"][:R]):
        gm = np.ones((B,), dt)
        for d in range(ns):
            gm = gm * fac[d][:, rng_[d]]
            dlog[:, r, d] = dlg[d][:, rng_[d]]
        gamma[:, r] = gm
    return gamma, dlog


def hand_gx(cfg, params, x, g, dtype=np.float64, gamma=None):
    """(gx, S) of the formula in NumPy at ``dtype``.  gamma: caller-provided region weights [B,R] (the cluster nets): the RBF
    term only, and the third return value q[B,R] = sum_k hbar phi."""
    dt = np.dtype(dtype).type
    p = inner(params)
    c = np.asarray(p["rbf_list"]["centers"]).astype(dt)
    s2 = np.exp(dt(-2) * np.asarray(p["rbf_list"]["log_sigs"]).astype(dt))
    W = np.asarray(p["linear"]["kernel"]).astype(dt)
    x, g = np.asarray(x).astype(dt), np.asarray(g).astype(dt)
    B, D = x.shape
    R = c.shape[0]
    hb = g @ W.T                                                   # [B,K]
    habs = np.abs(hb)
    ext = gamma is not None
    if ext:
        gam, dlog = np.asarray(gamma).astype(dt), np.zeros((B, R, D), dt)
    else:
        gam, dlog = _gate(cfg, x, dt)
    gx, S, q = np.zeros((B, D), dt), np.zeros((B, D), dt), np.zeros((B, R), dt)
    rows = _rows(cfg)
    for i in range(0, B, rows):
        sl = slice(i, i + rows)
        diff = x[sl, None, None, :] - c[None]                     # [b,R,K,D]
        u = (diff * diff).sum(-1) * s2[None]
        phi, fp = _basis(u, cfg["basis_func"], dt)
        s = dt(2) * hb[sl, None, :] * gam[sl, :, None] * fp * s2[None]
        sa = dt(2) * habs[sl, None, :] * gam[sl, :, None] * np.abs(fp) * s2[None]
        gx[sl] = np.einsum("brk,brkd->bd", s, diff)
        S[sl] = np.einsum("brk,brkd->bd", sa, np.abs(diff))
        q[sl] = (hb[sl, None, :] * phi).sum(-1)
        qa = (habs[sl, None, :] * np.abs(phi)).sum(-1)
        if not ext:
            gx[sl] += np.einsum("br,brd->bd", q[sl] * gam[sl], dlog[sl])
            S[sl] += np.einsum("br,brd->bd", qa * gam[sl], np.abs(dlog[sl]))
    return (gx, S, q) if ext else (gx, S)


def within(gx, ref, S):
    """(ok, worst): |gx - ref| <= RTOL |ref| + C_S S per entry; worst = max |gx - ref| / S (what c would have to be)."""
    err = np.abs(np.asarray(gx, np.float64) - ref)
    S = np.asarray(S, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(S > 0, err / np.where(S > 0, S, 1.0), np.where(err > 0, np.inf, 0.0))
    ok = bool(np.all(err <= RTOL * np.abs(ref) + C_S * S))
    return ok, float(np.nanmax(ratio)) if ratio.size else 0.0


# ---- the shape grid of the float32 kernels (test_gpu_vjpx.py; tools/vjpx_parity_constant.py measures C_S on the same inputs) ----
def _case(seed, B, qlo=None, qhi=None, **net):
    cfg, params = synth_net(seed, **net)
    x = queries(seed, cfg, B, lo=qlo, hi=qhi)
    return cfg, params, x, cotangent(seed, B, cfg["out_features"])


def _near_bound(seed):
    """One region split on coordinate 0, every query within 2 / delta of its upper bound: the gate term dominates."""
    cfg, params, x, g = _case(seed, 130, D=7, O=10, K=64, grid=(1,), delta=8.0)
    x[:, 0] = np.random.default_rng(seed).uniform(2.0 - 0.25, 2.0 + 0.25, size=x.shape[0]).astype(np.float32)
    return cfg, params, x, g


def _fixture(run):
    from conftest import load_ckpt_fixture
    cfg, params, x, *_ = load_ckpt_fixture(run)
    params = {"params": {k: {n: np.asarray(v, np.float32) for n, v in d.items()} for k, d in params["params"].items()}}
    x = np.asarray(x, np.float32)
    return cfg, params, x, cotangent(len(run), x.shape[0], cfg["out_features"])


def k5_cases():
    """{name: builder -> (cfg, params, x, g)}: every basis; D in {1,3,5,7,8}; O in {1,2,5,10,16,100}; one region far inside its
    box, one with the queries on a bound, a 300-region grid, regions beyond len(dimension_ranges); 4096 centres; B = 4097 (the
    batches 1, 63, 64, 65 are its prefixes); the four trained fixtures' stored queries."""
    from conftest import CKPT_RUNS
    cases = {}
    for i, b in enumerate(BASES):
        cases[f"basis_{b}"] = lambda i=i, b=b: _case(100 + i, 200, D=7, O=10, K=40, grid=(2, 2), basis=b)
    for D in (1, 3, 5, 7, 8):
        for b in ("gaussian", "spline"):
            cases[f"D{D}_{b}"] = lambda D=D, b=b: _case(200 + D, 130, D=D, O=10, K=64, grid=(2,), basis=b)
    for O in (1, 2, 5, 10, 16, 100):
        for b in ("gaussian", "inverse_multiquadric"):
            cases[f"O{O}_{b}"] = lambda O=O, b=b: _case(300 + O, 130, D=7, O=O, K=64, grid=(2,), basis=b)
    cases["one_region_far_inside"] = lambda: _case(401, 65, qlo=-0.5, qhi=0.5, D=7, O=10, K=4096, grid=(1, 1, 1))
    cases["one_region_on_a_bound"] = lambda: _near_bound(402)
    cases["grid_300_regions"] = lambda: _case(403, 300, D=7, O=10, K=4, grid=(10, 6, 5), basis="inverse_quadratic")
    cases["regions_beyond_ranges"] = lambda: _case(404, 130, D=7, O=10, K=32, grid=(2, 2), extra_regions=3)
    cases["B4097"] = lambda: _case(405, 4097, D=7, O=10, K=128, grid=(2,))
    for run in CKPT_RUNS:
        cases[f"ckpt_{run}"] = lambda run=run: _fixture(run)
    return cases


def _cfg_case(idx, B, K=None, O=None):
    """BASELINE config idx (irbfn_amd/configs.py), optionally with fewer centres / another output width."""
    from irbfn_amd import configs
    cfg, p = configs.model_card(idx), inner(configs.synth_params(idx))
    K = K or cfg["num_kernels"]
    O = O or cfg["out_features"]
    cfg = dict(cfg, num_kernels=K, out_features=O)
    params = {"params": {"rbf_list": {"centers": p["rbf_list"]["centers"][:, :K], "log_sigs": p["rbf_list"]["log_sigs"][:, :K]},
                         "linear": {"kernel": p["linear"]["kernel"][:K, :O], "bias": p["linear"]["bias"][:O]}}}
    return cfg, params, configs.synth_queries(idx, B), cotangent(idx, B, O)


def k5m_cases():
    """{name: builder}: the shapes K5m accepts -- BASELINE config 2 (4096 centres, O = 10) and config 4 (O = 100), d = 8, output
    widths that are no multiple of 4, a net of one 16-centre chunk, the other two fast basis classes."""
    return {
        "cfg2": lambda: _cfg_case(2, 130),
        "cfg4_O100": lambda: _cfg_case(4, 70),
        "d8_O16": lambda: _case(501, 130, D=8, O=16, K=200, grid=(1, 1), basis="inverse_quadratic"),
        "O7": lambda: _case(502, 130, D=7, O=7, K=100, grid=(1,), basis="inverse_multiquadric"),
        "O33_d3": lambda: _case(503, 65, D=3, O=33, K=77, grid=(1, 1, 1), basis="gaussian_wide"),
        "one_chunk": lambda: _case(504, 17, D=7, O=10, K=10, grid=(1,)),
        "on_a_bound": lambda: _near_bound(505),
    }
