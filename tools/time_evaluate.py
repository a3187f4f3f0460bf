"""Times the table evaluation (irbfn_amd/evaluate.py) at the reference's batch: B = 80 000 rows, T = 5.

Per kind (cartesian: inline bicycle, cartesian_st: single-track select model, frenet: Frenet model), a one-region gaussian
WCRBFNet with 4096 centres (BASELINE config 2's card; the Frenet one with D = 8):
  net.apply alone                 the forward of one batch;
  irbfn_eval_rollout_errors alone the evaluation kernel (two roll-outs, metrics, statistics, final merge) on a fixed prediction,
                                  accumulating, without and with the per-row output;
  evaluate_table over 8 batches   640 000 rows resident on the device: apply + kernel per batch, no host synchronisation inside.
One warm-up round over every variant, then ROUNDS interleaved rounds (every variant once per round, INNER calls between two
device events; evaluate_table: one call per span); the median over the rounds is reported with the min / max.  GPU box; output
kept in profiles/evaluate.txt."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from irbfn_amd import _lib, configs, evaluate  # noqa: E402
from irbfn_amd.dynamics import _dyn  # noqa: E402
from irbfn_amd.model import WCRBFNet  # noqa: E402

ROUNDS, INNER = 10, 20
B, T, NBATCH = 80000, 5, 8


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
    """variants: [(label, fn, calls per span)] -> {label: (median, min, max)} in us."""
    for _, fn, _ in variants:
        fn()
    torch.cuda.synchronize()
    t = {label: [] for label, _, _ in variants}
    for _ in range(ROUNDS):
        for label, fn, n in variants:
            t[label].append(span(fn, n))
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in t.items()}


def case(kind):
    rng = np.random.default_rng(len(kind))
    card = dict(configs.model_card(2))
    lo, hi = np.array([r[0] for r in card["lower_bounds"]]), np.array([r[0] for r in card["upper_bounds"]])
    N = B * NBATCH
    if kind == "frenet":
        x = (rng.normal(size=(N, 8)) * [.2, .2, 1, .1, 1, .1, .15, .08] + [0, 0, 4, 0, 4, 0, 0, 0]).astype(np.float32)
        lo, hi = x.min(0), x.max(0)
        card.update(in_features=8, lower_bounds=[[float(v)] for v in lo], upper_bounds=[[float(v)] for v in hi],
                    dimension_ranges=[[0] * 8], activation_idx=list(range(8)), delta=[100.0] * 8)
    else:
        x = rng.uniform(lo, hi, size=(N, 7)).astype(np.float32)
    D, K, O = card["in_features"], card["num_kernels"], 2 * T
    card["out_features"] = O
    params = {"params": {"rbf_list": {"centers": rng.uniform(lo, hi, size=(1, K, D)).astype(np.float32),
                                      "log_sigs": rng.uniform(0.0, 1.5, size=(1, K)).astype(np.float32)},
                         "linear": {"kernel": (rng.normal(size=(K, O)) * 0.05).astype(np.float32),
                                    "bias": np.zeros(O, np.float32)}}}
    y = np.hstack([rng.normal(size=(N, T)) * 2.0, rng.normal(size=(N, T)) * 0.5]).astype(np.float32)
    return WCRBFNet.from_config(card), params, x, y


def time_kind(kind):
    lib = _lib.load()
    net, params, x, y = case(kind)
    P = evaluate._tree_to_device(params, torch)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    dp = None if kind == "cartesian" else configs.DYN_PARAMS
    mode = evaluate.KINDS[kind][0]
    xb, yb = xd[:B], yd[:B]
    y_pred = net.apply(P, xb)
    s0 = evaluate._initial_state(kind, xb, torch)
    stats = evaluate.ErrorStats(mode)
    err = torch.empty((B, stats.num_metrics), dtype=torch.float32, device="cuda")
    keep, pp = _dyn(dp)
    res = measure([
        ("net.apply", lambda: net.apply(P, xb), INNER),
        ("eval kernel", lambda: evaluate._run(stats, s0, y_pred, yb, pp, 0, 1, None, torch, lib), INNER),
        ("eval kernel + per-row output", lambda: evaluate._run(stats, s0, y_pred, yb, pp, 0, 1, err, torch, lib), INNER),
        ("evaluate_table, 8 batches", lambda: evaluate.evaluate_table(net, P, xd, yd, kind, dp, batch_size=B), 1),
    ])
    print(f"-- {kind}: mode {mode}, M = {stats.num_metrics}, B = {B}, T = {T}, net {net.last_launch()['kernel']}")
    for label, (med, lo, hi) in res.items():
        print(f"   {label:32s} {med:10.1f} us  [{lo:.1f} .. {hi:.1f}]")
    k, a, tab = res["eval kernel"][0], res["net.apply"][0], res["evaluate_table, 8 batches"][0]
    print(f"   kernel share of a batch (kernel / (apply + kernel)) = {k / (a + k):.3f}; evaluate_table per batch = {tab / NBATCH:.1f} us "
          f"= {tab / NBATCH / (a + k):.2f} x (apply + kernel)")
    s = evaluate.evaluate_table(net, P, xd, yd, kind, dp, batch_size=B).summary()
    print("   position: " + ", ".join(f"{k_}={v}" for k_, v in s["position"].items() if k_ != "quantiles"))
    sys.stdout.flush()


def main():
    for kind in ("cartesian", "cartesian_st", "frenet"):
        time_kind(kind)


if __name__ == "__main__":
    main()
