"""Times the region-weighted parameter VJP (irbfn_net_vjp_gamma) on the gated K2 (rbf_vjp_kernel, GATED = 1: the default) and on
K2g over padded regions (rbf_vjp_f16gram_gamma, vjp_kernel = VJP_K2G_GAMMA), alternated in one process on two descriptors bound
to the same parameters: synthetic nets of tests/_cluster_util.py at the reference's shape (R = 500, D = 8, O = 10) with K = 50
and K = 10, B = 80 000 and 65 536.

  vjp     irbfn_net_vjp_gamma alone (d gamma included), region weights from irbfn_cluster_gate computed once (not timed)
  model   ClusterWCRBFNet.vjp with a cotangent of the logits (gate, VJP, softmax + Dense backward)
  step    train_step_fullint_withcluster on a ClusterTrainState; fwd_gamma_kernel = FWDG_K1G in both legs
  error   per leaf max |err| / max |leaf| and d gamma's max err / (1e-5 |ref| + 3e-6 sum |hbar phi|) against the float64 statement
          of tests/_cluster_vjp_gram_util.py at B = 512, both kernels

One warm-up pass over every variant of a shape, then ROUNDS interleaved rounds (every variant once per round, INNER calls between
two device events); median over the rounds with min / max (the spread between repeats).  ``--profile`` runs the VJP of one shape
(``--k 50`` / ``--k 10``) on one kernel (``--kernel k2`` / ``--kernel k2g``) a few times only, for a
``rocprofv3 --kernel-trace --stats`` pass in a run of its own.  ``--vjp-only`` stops each shape after the first block (to compare
builds of the library, IRBFN_LIB, process by process), ``--outside`` puts one query outside K1g's box (the hand-over to the gated K2).  GPU box; output kept as profiles/cluster_vjp_gram.txt."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _cluster_util import cluster_case  # noqa: E402
from _cluster_vjp_gram_util import STAGE, gamma_vjp64  # noqa: E402
from irbfn_amd import _lib, configs, train  # noqa: E402
from irbfn_amd.model import ClusterWCRBFNet, _ptr, _stream_ptr  # noqa: E402

PROFILE = "--profile" in sys.argv
VJP_ONLY, OUTSIDE = "--vjp-only" in sys.argv, "--outside" in sys.argv
ROUNDS, INNER = (1, 3) if PROFILE else (10, 5)
R, D, O, T = 500, 8, 10, 5
KERNELS = (("K2", _lib.VJP_K2), ("K2g", _lib.VJP_K2G_GAMMA))
DP = np.array(configs.DYN_PARAMS)


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def span(fn, n):
    fn()                                         # untimed: whatever ran before this variant stays out of its time
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def measure(title, variants):
    """variants: [(label, fn)]; prints median [min .. max] in us per call."""
    for _, fn in variants:
        fn()
    torch.cuda.synchronize()
    t = {label: [] for label, _ in variants}
    for _ in range(ROUNDS):
        for label, fn in variants:
            t[label].append(span(fn, INNER))
    print(f"== {title}")
    res = {}
    for label, v in t.items():
        med = float(np.median(v))
        res[label] = (med, min(v), max(v))
        print(f"   {label:24s} {med:9.1f} us  [{min(v):.1f} .. {max(v):.1f}]  spread {100 * (max(v) - min(v)) / med:4.1f} %")
    sys.stdout.flush()
    return res


def verdict(res, what):
    (k2, k2lo, _), (kg, _, kghi) = res[f"{what} K2"], res[f"{what} K2g"]
    clear = "beyond both spreads" if kghi < k2lo else ("NOT beyond both spreads" if kg < k2 else "K2g LOSES")
    print(f"   {what}: K2 / K2g = {k2 / kg:.2f} ({clear})")


def cluster_net(K, B, kernels=KERNELS):
    """One descriptor per kernel of one synthetic net (parameter scales of tests/test_gpu_cluster_gram.py::_case)."""
    rng, cfg, params, x = cluster_case(K, R=R, K=K, O=O, B=B, D=D)
    p = params["params"]
    p["rbf_list"]["log_sigs"] = rng.uniform(0.0, 1.0, size=(R, K)).astype(np.float32)
    p["linear"]["kernel"] = rng.normal(size=(K, O)).astype(np.float32)
    p["cluster"]["kernel"] = rng.normal(size=(D, R)).astype(np.float32) * 2.0
    nets = {n: ClusterWCRBFNet(**cfg).set_options(vjp_kernel=opt, fwd_gamma_kernel=_lib.FWDG_K1G) for n, opt in kernels}
    return rng, cfg, params, x, nets


def vjp_gamma(stage, xt, gt, gd, out):
    lib = _lib.load()
    h = stage._handle(torch)
    B = xt.shape[0]
    nbytes = int(lib.irbfn_net_vjp_workspace_bytes(h, B))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

    def fn():
        _lib.check(lib.irbfn_net_vjp_gamma(h, _ptr(xt), _ptr(gt), _ptr(gd), _ptr(out["centers"]), _ptr(out["log_sigs"]), _ptr(out["kernel"]),
                                           _ptr(out["bias"]), _ptr(out["dgamma"]), B, _ptr(ws), nbytes, _stream_ptr(torch)),
                   "irbfn_net_vjp_gamma")
    return fn


def leaves(K, B):
    return {"centers": torch.empty((R, K, D), device="cuda"), "log_sigs": torch.empty((R, K), device="cuda"),
            "kernel": torch.empty((K, O), device="cuda"), "bias": torch.empty((O,), device="cuda"), "dgamma": torch.empty((B, R), device="cuda")}


def shape(K, B, kernels=KERNELS):
    rng, cfg, params, x, nets = cluster_net(K, B, kernels)
    if OUTSIDE:
        x[123, 4] = 50.0                         # outside K1g's box: the matrix-core kernel hands the call to the gated K2 behind it
    xt = torch.from_numpy(x).cuda()
    gd = torch.from_numpy(rng.normal(size=(B, O)).astype(np.float32)).cuda()
    gld = torch.from_numpy(rng.normal(size=(B, R)).astype(np.float32)).cuda()
    for n in nets:
        _, gt = nets[n]._bind_and_gate(params, xt, torch, _lib.load())
    outs = {n: leaves(K, B) for n in nets}
    title = f"R = {R}, K = {K} (cpr = {(K + 31) // 32}, {32 * ((K + 31) // 32) / K:.2f} x padding), B = {B}"
    res = measure("irbfn_net_vjp_gamma, " + title, [(f"vjp {n}", vjp_gamma(nets[n].stage, xt, gt, gd, outs[n])) for n in nets])
    for n in nets:
        print(f"   {n}: {nets[n].stage.last_launch()}")
    if PROFILE:
        return
    verdict(res, "vjp")
    for k in outs["K2"]:
        a, b = outs["K2g"][k], outs["K2"][k]
        print(f"   max |K2g - K2| / max |K2| {k:9s} {float((a - b).abs().max() / b.abs().max()):.2e}")
    if VJP_ONLY:
        return
    res = measure("ClusterWCRBFNet.vjp, " + title,
                  [(f"model {n}", (lambda net: lambda: net.vjp(params, xt, gd, glogits=gld))(nets[n])) for n in nets])
    verdict(res, "model")
    # Frenet queries (speed in [1, 6]); the centres' third coordinate is moved there so that they stay inside the expansion's box
    params["params"]["rbf_list"]["centers"][:, :, 2] = rng.uniform(1.0, 6.0, size=(R, K)).astype(np.float32)
    x2 = x.copy()
    x2[:, 7] = rng.normal(size=B).astype(np.float32) * 0.05
    x2[:, 0] = rng.normal(size=B).astype(np.float32) * 0.2
    x2[:, 2] = rng.uniform(1.0, 6.0, size=B).astype(np.float32)
    yt = torch.from_numpy(np.hstack([rng.normal(size=(B, T)) * 2, rng.normal(size=(B, T)) * 0.5]).astype(np.float32)).cuda()
    it = torch.from_numpy(np.eye(R, dtype=np.float32)[rng.integers(0, R, size=B)]).cuda()
    x2t = torch.from_numpy(x2).cuda()
    states = {n: train.ClusterTrainState.create(nets[n], params, lr=1e-3, max_grad_norm=1.0) for n in nets}

    def step(n):
        def fn():
            states[n], _ = train.train_step_fullint_withcluster(states[n], x2t, yt, it, DP)
        return fn

    res = measure("train_step_fullint_withcluster (fwd_gamma_kernel = K1G), " + title, [(f"step {n}", step(n)) for n in nets])
    verdict(res, "step")


def errors(K, B=512):
    rng, cfg, params, x, nets = cluster_net(K, B)
    xt = torch.from_numpy(x).cuda()
    g = rng.normal(size=(B, O)).astype(np.float32)
    gd = torch.from_numpy(g).cuda()
    print(f"== error against float64, R = {R}, K = {K}, B = {B}")
    ref = None
    for n in nets:
        _, gt = nets[n]._bind_and_gate(params, xt, torch, _lib.load())
        if ref is None:
            ref = gamma_vjp64(cfg, params, x, gt.cpu().numpy(), g)
        out = leaves(K, B)
        vjp_gamma(nets[n].stage, xt, gt, gd, out)()
        torch.cuda.synchronize()
        line = [f"{k} {np.abs(out[k].cpu().numpy() - ref[0][k]).max() / np.abs(ref[0][k]).max():.2e}" for k in STAGE]
        bound = 1e-5 * np.abs(ref[1]) + 3e-6 * ref[2]
        line.append(f"dgamma err / bound {float((np.abs(out['dgamma'].cpu().numpy() - ref[1]) / bound).max()):.3f}")
        print(f"   {n:4s} max |err| / max |leaf|: " + ", ".join(line))
    sys.stdout.flush()


def main():
    torch.manual_seed(0)
    if PROFILE:
        which = arg("--kernel", "k2g")
        shape(int(arg("--k", "50")), int(arg("--b", "80000")), [k for k in KERNELS if k[0].lower() == which])
        return
    for K in (50, 10):
        for B in (80000, 65536):
            shape(K, B)
    for K in () if VJP_ONLY else (50, 10):
        errors(K)


if __name__ == "__main__":
    main()
