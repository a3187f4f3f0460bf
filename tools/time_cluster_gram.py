"""Times the region-weighted forward (irbfn_net_forward_gamma) and its planning tick (irbfn_plan_tick_gamma) on the gated K1
(rbf_fwd_qlane, GATED = 1: the default) and on K1g over padded regions (rbf_fwd_f16gram_gamma, fwd_gamma_kernel = FWDG_K1G),
alternated in one process on two descriptors bound to the same parameters.

  forward   synthetic nets of tests/_cluster_util.py at the reference's shape (R = 500, D = 8, O = 10) with K = 50 and K = 10,
            B = 65 536 and 80 000; region weights from irbfn_cluster_gate, computed once (not timed)
  tick      the same two nets through the one-launch Frenet tick (T = 5) at B = 65 536, next to the K1g forward followed by the
            stand-alone roll-out (torch.cat + irbfn_rollout_forward)
  planner   the golden 12-region Frenet net (tests/golden, K = 100 -> 128 padded) at B = 65 536: irbfn_net_gate (timed on its own)
            -> irbfn_net_forward_gamma on both kernels, next to its fused forwards (irbfn_net_forward: the gated K1 and K1r)

One warm-up pass over every variant of a shape, then ROUNDS interleaved rounds (every variant once per round, INNER launches
between two device events, 200 launches per variant); median over the rounds with min / max (the spread between repeats).
``--profile`` runs every variant a few times only, for a ``rocprofv3 --kernel-trace --stats`` pass in a run of its own.
GPU box; output kept as profiles/cluster_gram.txt."""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _cluster_util import cluster_case  # noqa: E402
from conftest import load_ckpt_fixture  # noqa: E402
from irbfn_amd import _lib, configs  # noqa: E402
from irbfn_amd.dynamics import _dyn  # noqa: E402
from irbfn_amd.model import ClusterWCRBFNet, WCRBFNet, _ptr, _stream_ptr  # noqa: E402

PROFILE = "--profile" in sys.argv
ROUNDS, INNER = (1, 3) if PROFILE else (10, 20)
MODE, T = _lib.ROLLOUT_FRENET_LS, 5


def span(fn, n):
    fn()                                         # untimed: whatever ran before this variant stays out of its time
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def measure(title, variants, pairs=None):
    """variants: [(label, fn)]; prints median [min .. max] in us per launch (pairs: (query, centre) pairs for a rate)."""
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
        res[label] = med
        rate = f"  {pairs / med * 1e-6:6.2f} Tpairs/s" if pairs and ("forward" in label or "tick" in label) else ""
        print(f"   {label:44s} {med:9.1f} us  [{min(v):.1f} .. {max(v):.1f}]  spread {100 * (max(v) - min(v)) / med:4.1f} %{rate}")
    sys.stdout.flush()
    return res


def frenet_state0(rng, B):
    return np.hstack([rng.normal(size=(B, 1)) * 0.2, rng.normal(size=(B, 1)) * 0.2, rng.normal(size=(B, 1)) * 0.1,
                      rng.uniform(1, 6, size=(B, 1)), rng.normal(size=(B, 3)) * 0.1, rng.normal(size=(B, 1)) * 0.05]).astype(np.float32)


def fwd_gamma(stage, xt, gt, out):
    lib = _lib.load()
    h = stage._handle(torch)

    def fn():
        _lib.check(lib.irbfn_net_forward_gamma(h, _ptr(xt), _ptr(gt), _ptr(out), xt.shape[0], _stream_ptr(torch)), "irbfn_net_forward_gamma")
    return fn


def cluster_net(K, B):
    """Two descriptors of one synthetic net (parameter scales of tests/test_gpu_cluster_scale.py::_forward_case), region weights."""
    rng, cfg, params, x = cluster_case(K, R=500, K=K, O=10, B=B, D=8)
    p = params["params"]
    p["rbf_list"]["log_sigs"] = rng.uniform(0.0, 1.0, size=(500, K)).astype(np.float32)
    p["linear"]["kernel"] = rng.normal(size=(K, 10)).astype(np.float32)
    p["cluster"]["kernel"] = rng.normal(size=(8, 500)).astype(np.float32) * 2.0
    xt = torch.from_numpy(x).cuda()
    nets = {}
    for name, opt in (("K1", _lib.FWDG_AUTO), ("K1g", _lib.FWDG_K1G)):
        nets[name] = ClusterWCRBFNet(**cfg).set_options(fwd_gamma_kernel=opt)
        _, gt = nets[name]._bind_and_gate(params, xt, torch, _lib.load())
    return rng, nets, xt, gt


def forward_shape(K, B):
    _, nets, xt, gt = cluster_net(K, B)
    out = {n: torch.empty((B, 10), dtype=torch.float32, device="cuda") for n in nets}
    variants = [(f"forward {n}", fwd_gamma(nets[n].stage, xt, gt, out[n])) for n in nets]
    res = measure(f"forward, R = 500, K = {K} (cpr = {(K + 31) // 32}, {32 * ((K + 31) // 32) / K:.2f} x padding), B = {B}", variants,
                  pairs=B * 500 * K)
    for n in nets:
        print(f"   {n}: {nets[n].stage.last_launch()}")
    print(f"   K1 / K1g = {res['forward K1'] / res['forward K1g']:.2f};  max |K1g - K1| = {float((out['K1g'] - out['K1']).abs().max()):.2e}"
          f" at max |out| = {float(out['K1'].abs().max()):.2e}")


def tick_shape(K, B):
    lib = _lib.load()
    rng, nets, xt, gt = cluster_net(K, B)
    st = torch.from_numpy(frenet_state0(rng, B)).cuda()
    mt = torch.from_numpy((rng.random(B) < 0.5).astype(np.int32)).cuda()
    keep, pp = _dyn(configs.DYN_PARAMS)
    ctrl = torch.empty((B, 10), dtype=torch.float32, device="cuda")
    states = torch.empty((B, T, 8), dtype=torch.float32, device="cuda")

    def tick(n):
        h = nets[n].stage._handle(torch)

        def fn():
            _lib.check(lib.irbfn_plan_tick_gamma(h, MODE, _ptr(xt), _ptr(gt), _ptr(mt), _ptr(st), pp, _ptr(ctrl), _ptr(states), B, T,
                                                 _stream_ptr(torch)), "irbfn_plan_tick_gamma")
        return fn

    fwd = fwd_gamma(nets["K1g"].stage, xt, gt, ctrl)

    def chain():
        fwd()
        ctrl[:, T:] = torch.where(mt[:, None] != 0, -ctrl[:, T:], ctrl[:, T:])
        x0u = torch.cat([st, ctrl], dim=1)
        _lib.check(lib.irbfn_rollout_forward(MODE, _ptr(x0u), pp, _ptr(states), B, T, _stream_ptr(torch)), "irbfn_rollout_forward")

    res = measure(f"Frenet tick T = {T}, R = 500, K = {K}, B = {B}",
                  [("tick K1 (roll-out in its epilogue)", tick("K1")), ("tick K1g (one launch)", tick("K1g")),
                   ("forward K1g alone", fwd), ("K1g forward -> flip -> cat -> roll-out", chain)], pairs=B * 500 * K)
    tick("K1g")()
    print(f"   K1g tick: {nets['K1g'].stage.last_launch()}")
    print(f"   tick K1 / tick K1g = {res['tick K1 (roll-out in its epilogue)'] / res['tick K1g (one launch)']:.2f};  "
          f"K1g tick / (K1g forward + roll-out) = {res['tick K1g (one launch)'] / res['K1g forward -> flip -> cat -> roll-out']:.2f}")


def planner_shape(B):
    lib = _lib.load()
    cfg, params, *_ = load_ckpt_fixture("dnmpc_12regions_frenet_l1_bigdata")
    rng = np.random.default_rng(12)
    ns = len(cfg["activation_idx"])
    lo = np.array([min(cfg["lower_bounds"][d]) for d in range(ns)])
    hi = np.array([max(cfg["upper_bounds"][d]) for d in range(ns)])
    x = np.hstack([rng.uniform(lo, hi, size=(B, ns)), rng.normal(size=(B, cfg["in_features"] - ns)) * 0.1]).astype(np.float32)
    xt = torch.from_numpy(x).cuda()
    nets = {}
    for name, opts in (("gamma K1", {}), ("gamma K1g", {"fwd_gamma_kernel": _lib.FWDG_K1G}), ("fused K1", {"fwd_kernel": _lib.FWD_K1}),
                       ("fused auto", {})):
        nets[name] = WCRBFNet.from_config(cfg).set_options(**opts).bind(params)
    gt = torch.empty((B, cfg["num_regions"]), dtype=torch.float32, device="cuda")
    out = {n: torch.empty((B, cfg["out_features"]), dtype=torch.float32, device="cuda") for n in nets}

    def gate():
        _lib.check(lib.irbfn_net_gate(nets["gamma K1"]._handle(torch), _ptr(xt), _ptr(gt), B, _stream_ptr(torch)), "irbfn_net_gate")

    def fused(n):
        h = nets[n]._handle(torch)

        def fn():
            _lib.check(lib.irbfn_net_forward(h, _ptr(xt), _ptr(out[n]), B, _stream_ptr(torch)), "irbfn_net_forward")
        return fn

    gate()
    K, R = cfg["num_kernels"], cfg["num_regions"]
    res = measure(f"golden 12-region Frenet planner (K = {K}, cpr = {(K + 31) // 32}), B = {B}",
                  [("irbfn_net_gate", gate), ("forward gamma K1", fwd_gamma(nets["gamma K1"], xt, gt, out["gamma K1"])),
                   ("forward gamma K1g", fwd_gamma(nets["gamma K1g"], xt, gt, out["gamma K1g"])),
                   ("forward fused K1 (fwd_kernel = K1)", fused("fused K1")), ("forward fused automatic", fused("fused auto"))],
                  pairs=B * R * K)
    for n in nets:
        print(f"   {n}: {nets[n].last_launch()}")
    print(f"   gamma K1 / gamma K1g = {res['forward gamma K1'] / res['forward gamma K1g']:.2f};  max |K1g - K1| = "
          f"{float((out['gamma K1g'] - out['gamma K1']).abs().max()):.2e}")


def main():
    torch.manual_seed(0)
    for K in (50, 10):
        for B in (65536, 80000):
            forward_shape(K, B)
    for K in (50, 10):
        tick_shape(K, 65536)
    planner_shape(65536)


if __name__ == "__main__":
    main()
