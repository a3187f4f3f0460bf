"""One float64 train_step_fullint (a use_float64 net: float64 forward, seeds through the 5-step bicycle, parameter VJP,
clip + Adam) on dnmpc_128regions -- the reference trained it under --use_float64 -- at the reference's batch of 80000
(scripts/configs/*.yaml), and the float32 step on the same net for comparison.  Needs a GPU."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_ckpt_fixture  # noqa: E402
from irbfn_amd import train  # noqa: E402
from irbfn_amd.model import WCRBFNet  # noqa: E402


def timed(fn, n):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3          # us per step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=80000)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    cfg, P, _, *_ = load_ckpt_fixture("dnmpc_128regions")
    ns = len(cfg["activation_idx"])
    lo = np.array([min(cfg["lower_bounds"][d]) for d in range(ns)])
    hi = np.array([max(cfg["upper_bounds"][d]) for d in range(ns)])
    rng = np.random.default_rng(1)
    B = args.batch
    x = rng.uniform(lo, hi, size=(B, cfg["in_features"]))
    y = np.hstack([rng.normal(size=(B, 5)) * 2, rng.normal(size=(B, 5)) * 0.5])
    for f64 in (True, False):
        dt = torch.float64 if f64 else torch.float32
        net = WCRBFNet.from_config(cfg, use_float64=f64)
        state = train.TrainState.create(net, P, lr=1e-3, max_grad_norm=1.0)
        xd, yd = torch.tensor(x, dtype=dt).cuda(), torch.tensor(y, dtype=dt).cuda()

        def step():
            nonlocal state
            state, _ = train.train_step_fullint(state, xd, yd)
        us = timed(step, args.iters)
        fw = timed(lambda: net.apply(state.params, xd), args.iters)
        g = torch.randn(B, cfg["out_features"], dtype=dt, device="cuda")
        vj = timed(lambda: net.vjp(state.params, xd, g, out=state.grads), args.iters)
        print(f"dnmpc_128regions {'float64' if f64 else 'float32'} train_step_fullint, B={B}: {us:.1f} us/step "
              f"(forward {fw:.1f}, parameter VJP {vj:.1f})", flush=True)


if __name__ == "__main__":
    main()
