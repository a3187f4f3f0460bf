"""Times the query VJP (K5 / K5m, forced and auto) next to two yardsticks taken in the same process: the forward forced to K1 on
the same net, and what a user could do without it -- torch.autograd of a chunked float32 torch restatement on the GPU.

Shapes: BASELINE config 2 (4096 centres, d = 7, O = 10, B = 65 536), the config-4 net (O = 100, B = 32 768) and its first 32 and 16
outputs (where does K5m overtake K5?), the four trained fixture nets and the 64-wide RBF stage of the DeeperWCRBFNet fixture at
B = 65 536, the R = 500 cluster case of tests/_cluster_util.py.  One warm-up pass over every variant (code
objects, clocks), then ROUNDS interleaved rounds (every variant once per round, INNER calls between two device events); the
median over the rounds is reported with the min / max.  GPU box; output kept as profiles/vjp_x.txt."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _cluster_util import cluster_case  # noqa: E402
from conftest import CKPT_RUNS, load_ckpt_fixture, load_deeper_fixture  # noqa: E402
from irbfn_amd import _lib, configs  # noqa: E402
from irbfn_amd.model import ClusterWCRBFNet, WCRBFNet  # noqa: E402

ROUNDS, INNER = 7, 5


def span(fn, n):
    fn()                                         # untimed: whatever ran before this variant (caches, clocks) stays out of its time
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def measure(variants):
    """variants: [(label, fn, inner)] -> {label: (median, min, max)} in us."""
    for _, fn, _ in variants:
        fn()
    torch.cuda.synchronize()
    t = {label: [] for label, _, _ in variants}
    for _ in range(ROUNDS):
        for label, fn, inner in variants:
            t[label].append(span(fn, inner))
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in t.items()}


def dev(params):
    return {"params": {k: {n: torch.from_numpy(np.asarray(v, np.float32)).cuda() for n, v in d.items()} for k, d in params["params"].items()}}


_BASIS = {"gaussian": lambda d: torch.exp(-d * d), "gaussian_wide": lambda d: torch.exp(-0.1 * d * d),
          "inverse_quadratic": lambda d: 1.0 / (1.0 + d * d), "inverse_multiquadric": lambda d: 1.0 / torch.sqrt(1.0 + d * d)}


def torch_phi(cfg, p, x):
    """flax_rbf.py:275-283 as the reference writes it: d = sqrt(sum (x - c)^2) / exp(log_sig), phi = basis(d) -> [b,R,K]."""
    diff = x[:, None, None, :] - p["rbf_list"]["centers"][None]
    return _BASIS[cfg["basis_func"]]((diff ** 2).sum(-1) ** 0.5 / torch.exp(p["rbf_list"]["log_sigs"])[None])


def torch_wcrbf(cfg, P, x):
    """WCRBFNet.__call__ (model.py:169-198) on device tensors: the tanh gate, the RBF layers, the Dense layer."""
    p, ns = P["params"], len(cfg["activation_idx"])
    fac = []
    for d in range(ns):
        lo = torch.tensor(cfg["lower_bounds"][d], dtype=x.dtype, device=x.device)
        hi = torch.tensor(cfg["upper_bounds"][d], dtype=x.dtype, device=x.device)
        dl = cfg["delta"][d]
        fac.append(((torch.tanh(dl * (x[:, d, None] - lo[None])) + 1) / 2) * ((torch.tanh(dl * (hi[None] - x[:, d, None])) + 1) / 2))
    cols = []
    for r in range(cfg["num_regions"]):
        if r < len(cfg["dimension_ranges"]):
            cur = torch.ones_like(x[:, 0])
            for d in range(ns):
                cur = cur * fac[d][:, cfg["dimension_ranges"][r][d]]
        else:
            cur = torch.zeros_like(x[:, 0])
        cols.append(cur)
    gamma = torch.stack(cols, 1)
    return (gamma[:, :, None] * torch_phi(cfg, p, x)).sum(1) @ p["linear"]["kernel"] + p["linear"]["bias"]


def torch_cluster(cfg, P, x):
    """ClusterWCRBFNet.__call__ (model.py:393-414) -> (out, logits)."""
    p = P["params"]
    logits = x @ p["cluster"]["kernel"] + p["cluster"]["bias"]
    out = (torch.softmax(logits, 1)[:, :, None] * torch_phi(cfg, p, x)).sum(1) @ p["linear"]["kernel"] + p["linear"]["bias"]
    return out, logits


def torch_autograd(apply, cfg, P, x, g, chunk):
    """d sum(apply(x) g) / d x of the float32 torch restatement, in row chunks (its [rows, R, K, D] intermediate)."""
    out = torch.empty_like(x)
    for i in range(0, x.shape[0], chunk):
        xt = x[i:i + chunk].detach().requires_grad_()
        y = apply(cfg, P, xt)
        y = y[0] if isinstance(y, tuple) else y
        (out[i:i + chunk],) = torch.autograd.grad((y * g[i:i + chunk]).sum(), xt)
    return out


def in_box(cfg, B, seed=0):
    rng = np.random.default_rng(seed)
    ns, D = len(cfg["activation_idx"]), cfg["in_features"]
    lo = np.array([min(cfg["lower_bounds"][d]) for d in range(ns)])
    hi = np.array([max(cfg["upper_bounds"][d]) for d in range(ns)])
    return np.hstack([rng.uniform(lo, hi, size=(B, ns)), rng.normal(size=(B, D - ns)) * 0.1]).astype(np.float32)


def wcrbf_shape(name, cfg, params, x):
    net, P = WCRBFNet.from_config(cfg), dev(params)
    B, O = x.shape[0], cfg["out_features"]
    N, D = cfg["num_regions"] * cfg["num_kernels"], cfg["in_features"]
    xt = torch.from_numpy(x).cuda()
    g = torch.randn(B, O, device="cuda")
    names = {}

    def vjpx(kernel, label):
        def fn():
            net.set_options(vjpx_kernel=kernel)
            net.vjp_x(P, xt, g)
            names[label] = net.last_launch()["kernel"]
        return fn

    def fwd():
        net.set_options(fwd_kernel=_lib.FWD_K1)
        net.apply(P, xt)
        names["K1 forward"] = net.last_launch()["kernel"]

    variants = [("K5", vjpx(_lib.VJPX_K5, "K5"), INNER)]
    try:
        vjpx(_lib.VJPX_K5M, "K5m")()
        variants.append(("K5m", vjpx(_lib.VJPX_K5M, "K5m"), INNER))
    except ValueError:
        pass                                     # not eligible for this net
    variants += [("auto", vjpx(_lib.VJPX_AUTO, "auto"), INNER), ("K1 forward", fwd, INNER)]
    chunk = max(64, min(B, (1 << 26) // (N * D)))
    variants.append(("torch autograd", lambda: torch_autograd(torch_wcrbf, cfg, P, xt, g, chunk), 1))
    res = measure(variants)
    report(name, B, N, D, O, res, names)


def cluster_shape(B=16384):
    _, cfg, params, x = cluster_case(500, R=500, K=10, O=10, B=B, D=8)
    net, P = ClusterWCRBFNet(**cfg), dev(params)
    xt = torch.from_numpy(x).cuda()
    g = torch.randn(B, 10, device="cuda")
    gl = torch.randn(B, 500, device="cuda")
    names = {}

    def vx():
        net.vjp_x(P, xt, g, glogits=gl)
        names["K5"] = net.stage.last_launch()["kernel"]

    def fwd():
        net.apply(P, xt)
        names["K1 forward"] = net.stage.last_launch()["kernel"]

    def ta():
        out = torch.empty_like(xt)
        for i in range(0, B, 1024):
            x_ = xt[i:i + 1024].detach().requires_grad_()
            o, lg = torch_cluster(cfg, P, x_)
            (out[i:i + 1024],) = torch.autograd.grad((o * g[i:i + 1024]).sum() + (lg * gl[i:i + 1024]).sum(), x_)
        return out
    res = measure([("K5", vx, INNER), ("K1 forward", fwd, INNER), ("torch autograd", ta, 1)])
    report("cluster R=500 K=10 (gate + kernel + softmax chain)", B, 5000, 8, 10, res, names)


def report(name, B, N, D, O, res, names):
    print(f"== {name}: B = {B}, {N} centres, d = {D}, O = {O}")
    k1 = res["K1 forward"][0]
    for label, (med, lo, hi) in res.items():
        extra = f"  = {med / k1:.2f} x K1 forward" if label != "K1 forward" else f"  (cost model: x-VJP = {(5 * D + 3 + 2 * O) / (3 * D + 2 + 2 * O):.2f} x)"
        print(f"   {label:15s} {med:10.1f} us  [{lo:.1f} .. {hi:.1f}]{extra}   {names.get(label, '')}")
    sys.stdout.flush()


def main():
    torch.manual_seed(0)
    wcrbf_shape("config 2", configs.model_card(2), configs.synth_params(2), configs.synth_queries(2, 65536))
    wcrbf_shape("config 4 net", configs.model_card(4), configs.synth_params(4), configs.synth_queries(4, 32768))
    c4, p4 = configs.model_card(4), configs.synth_params(4)["params"]
    for O in (32, 16):
        cut = {"params": {"rbf_list": p4["rbf_list"], "linear": {"kernel": p4["linear"]["kernel"][:, :O].copy(), "bias": p4["linear"]["bias"][:O].copy()}}}
        wcrbf_shape(f"config 4 net, first {O} outputs", dict(c4, out_features=O), cut, configs.synth_queries(4, 32768))
    for run in CKPT_RUNS:
        cfg, params, *_ = load_ckpt_fixture(run)
        wcrbf_shape(f"fixture {run}", cfg, params, in_box(cfg, 65536))
    cfg, params, *_ = load_deeper_fixture()
    stage = {"params": {"rbf_list": params["params"]["rbf_list"], "linear": params["params"]["linear_pre1"]}}
    wcrbf_shape("DeeperWCRBFNet fixture, RBF stage (linear_pre1, 64 wide)", dict(cfg, out_features=64), stage, in_box(cfg, 65536))
    cluster_shape()


if __name__ == "__main__":
    main()
