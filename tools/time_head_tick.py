"""Times the planning tick of DeeperWCRBFNet and ClusterWCRBFNet next to the chain of separate launches it replaces, taken in the
same process.

Golden Deeper net (tests/golden, D = 8, O = 10: FRENET_LS, T = 5) at B in {1, 8192, 65 536, 80 000}:
  head alone   `irbfn_mlp_head_tick` on a fixed stage output h1 against `irbfn_mlp_head_forward` -> torch.where flip ->
               torch.cat([state0, controls]) -> `irbfn_rollout_forward` (what a caller had to compose before the tick existed),
               both as direct library calls on preallocated outputs;
  whole tick   `planner.plan_tick(DeeperWCRBFNet)` against `net.apply` -> flip -> cat -> `dynamics.rollout_forward`.
Cluster net of tests/_cluster_util.py (R = 500, K = 10, D = 8, O = 10) at B in {5000, 65 536}: `planner.plan_tick` against
`net.apply` -> flip -> cat -> roll-out.

One warm-up pass over every variant (code objects, clocks), then ROUNDS interleaved rounds (every variant once per round, INNER
calls between two device events); the median over the rounds is reported with the min / max.  GPU box; output kept as
profiles/head_tick.txt."""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _cluster_util import cluster_case  # noqa: E402
from conftest import load_deeper_fixture  # noqa: E402
from irbfn_amd import _lib, configs, dynamics, planner  # noqa: E402
from irbfn_amd.dynamics import _dyn  # noqa: E402
from irbfn_amd.model import ClusterWCRBFNet, DeeperWCRBFNet, _ptr, _stream_ptr  # noqa: E402

ROUNDS, INNER = 7, 20
MODE, T = _lib.ROLLOUT_FRENET_LS, 5


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
    """variants: [(label, fn)] -> {label: (median, min, max)} in us."""
    for _, fn in variants:
        fn()
    torch.cuda.synchronize()
    t = {label: [] for label, _ in variants}
    for _ in range(ROUNDS):
        for label, fn in variants:
            t[label].append(span(fn, INNER))
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in t.items()}


def dev(params):
    return {"params": {k: {n: torch.from_numpy(np.asarray(v, np.float32)).cuda() for n, v in d.items()} for k, d in params["params"].items()}}


def frenet_state0(rng, B):
    return np.hstack([rng.normal(size=(B, 1)) * 0.2, rng.normal(size=(B, 1)) * 0.2, rng.normal(size=(B, 1)) * 0.1,
                      rng.uniform(1, 6, size=(B, 1)), rng.normal(size=(B, 3)) * 0.1, rng.normal(size=(B, 1)) * 0.05]).astype(np.float32)


def flip(u, mt):
    u[:, T:] = torch.where(mt[:, None] != 0, -u[:, T:], u[:, T:])
    return u


def report(title, res, fused, chain):
    print(f"== {title}")
    for label, (med, lo, hi) in res.items():
        print(f"   {label:34s} {med:9.1f} us  [{lo:.1f} .. {hi:.1f}]")
    print(f"   fused / chain = {res[fused][0] / res[chain][0]:.2f}")
    sys.stdout.flush()


def deeper_shape(B):
    lib = _lib.load()
    cfg, params, *_ = load_deeper_fixture()
    net, P = DeeperWCRBFNet.from_config(cfg), dev(params)
    rng = np.random.default_rng(B)
    ns = len(cfg["activation_idx"])
    lo = np.array([min(cfg["lower_bounds"][d]) for d in range(ns)])
    hi = np.array([max(cfg["upper_bounds"][d]) for d in range(ns)])
    xt = torch.from_numpy(rng.uniform(lo, hi, size=(B, 8)).astype(np.float32)).cuda()
    st = torch.from_numpy(frenet_state0(rng, B)).cuda()
    mt = torch.from_numpy((rng.random(B) < 0.5).astype(np.int32)).cuda()
    h1, head = net._stage_and_head(P, xt, torch)
    keep, pp = _dyn(configs.DYN_PARAMS)
    ctrl = torch.empty((B, 10), dtype=torch.float32, device="cuda")
    states = torch.empty((B, T, 8), dtype=torch.float32, device="cuda")
    null = C.c_void_p(None)

    def head_fused(c):
        def fn():
            _lib.check(lib.irbfn_mlp_head_tick(_ptr(h1), _ptr(head[0]), _ptr(head[1]), _ptr(head[2]), _ptr(head[3]), MODE, _ptr(mt),
                                               _ptr(st), pp, c, _ptr(states), B, 64, 64, 10, T, _stream_ptr(torch)), "irbfn_mlp_head_tick")
        return fn

    def head_chain():
        _lib.check(lib.irbfn_mlp_head_forward(_ptr(h1), _ptr(head[0]), _ptr(head[1]), _ptr(head[2]), _ptr(head[3]), _ptr(ctrl), B, 64, 64,
                                              10, _stream_ptr(torch)), "irbfn_mlp_head_forward")
        x0u = torch.cat([st, flip(ctrl, mt)], dim=1)
        _lib.check(lib.irbfn_rollout_forward(MODE, _ptr(x0u), pp, _ptr(states), B, T, _stream_ptr(torch)), "irbfn_rollout_forward")

    def tick():
        planner.plan_tick(net, P, xt, mt, st, configs.DYN_PARAMS, mode=MODE)

    def tick_chain():
        u = flip(net.apply(P, xt), mt)
        dynamics.rollout_forward(MODE, torch.cat([st, u], dim=1), configs.DYN_PARAMS, T)

    res = measure([("head: irbfn_mlp_head_tick", head_fused(_ptr(ctrl))), ("head: tick, no controls buffer", head_fused(null)),
                   ("head: forward -> flip -> roll-out", head_chain), ("whole: plan_tick", tick),
                   ("whole: apply -> flip -> roll-out", tick_chain)])
    print(f"-- DeeperWCRBFNet fixture, B = {B} (stage: {net.stage.last_launch()['kernel']})")
    report("head alone", {k: v for k, v in res.items() if k.startswith("head")}, "head: irbfn_mlp_head_tick", "head: forward -> flip -> roll-out")
    report("whole tick, stage included", {k: v for k, v in res.items() if k.startswith("whole")}, "whole: plan_tick",
           "whole: apply -> flip -> roll-out")


def cluster_shape(B):
    rng, cfg, params, x = cluster_case(500, R=500, K=10, O=10, B=B, D=8)
    net, P = ClusterWCRBFNet(**cfg), dev(params)
    xt = torch.from_numpy(x).cuda()
    st = torch.from_numpy(frenet_state0(rng, B)).cuda()
    mt = torch.from_numpy((rng.random(B) < 0.5).astype(np.int32)).cuda()

    def tick():
        planner.plan_tick(net, P, xt, mt, st, configs.DYN_PARAMS, mode=MODE)

    def chain():
        u = flip(net.apply(P, xt)[0], mt)
        dynamics.rollout_forward(MODE, torch.cat([st, u], dim=1), configs.DYN_PARAMS, T)

    res = measure([("cluster: plan_tick", tick), ("cluster: apply -> flip -> roll-out", chain)])
    tick()
    print(f"-- ClusterWCRBFNet R = 500, K = 10, B = {B} (tick: {net.stage.last_launch()['kernel']})")
    report("gate + tick", res, "cluster: plan_tick", "cluster: apply -> flip -> roll-out")


def main():
    torch.manual_seed(0)
    for B in (1, 8192, 65536, 80000):
        deeper_shape(B)
    for B in (5000, 65536):
        cluster_shape(B)


if __name__ == "__main__":
    main()
