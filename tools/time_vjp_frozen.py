"""Full K2g against K2g's frozen-leaf instances (irbfn_net_vjp_frozen) on the same net and batch: the fixed-centre net
(no_centres) and the fixed-width net (linear), interleaved A/B, median over rounds of the mean of `reps` VJPs each.
    python tools/time_vjp_frozen.py [--rounds 7] [--reps 20]
Sizes: 1 region x 500 centres, d = 8, O = 10, B = 80000 (the reference's fixed-centre checkpoint at its batch size);
1000 centres, same otherwise (its fixed-width checkpoint); config 3 (d = 7, 4096 centres, O = 10, B = 65536)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from irbfn_amd import _lib, configs, distributed  # noqa: E402
from irbfn_amd.model import WCRBFNet  # noqa: E402


def t_us(fn, reps):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def case_ref(K, B, D=8, O=10, seed=0):
    rng = np.random.default_rng(seed)
    card = {"in_features": D, "out_features": O, "num_kernels": K, "basis_func": "gaussian", "num_regions": 1,
            "lower_bounds": [[-1.0]] * D, "upper_bounds": [[2.0]] * D, "dimension_ranges": [[0] * D],
            "activation_idx": list(range(D)), "delta": [20.0] * D}
    P = {"params": {"rbf_list": {"centers": rng.uniform(-1.4, 2.4, size=(1, K, D)).astype(np.float32),
                                 "log_sigs": rng.uniform(-0.2, 0.9, size=(1, K)).astype(np.float32)},
                    "linear": {"kernel": rng.normal(size=(K, O)).astype(np.float32), "bias": rng.normal(size=(O,)).astype(np.float32)}}}
    x = rng.uniform(-1.0, 2.0, size=(B, D)).astype(np.float32)
    g = (rng.normal(size=(B, O)) * 1e-2).astype(np.float32)
    return card, P, x, g


def case_cfg3():
    return configs.model_card(3), configs.synth_params(3), configs.synth_queries(3), configs.synth_cotangent(3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    print(f"# {torch.cuda.get_device_name(0)}; median over {a.rounds} interleaved rounds of the mean of {a.reps} VJPs (us)")
    cases = (("1x500, d=8, O=10, B=80000", lambda: case_ref(500, 80000)),
             ("1x1000, d=8, O=10, B=80000", lambda: case_ref(1000, 80000)),
             ("config 3 (4096, d=7, O=10, B=65536)", case_cfg3))
    for title, mk in cases:
        card, P, x, g = mk()
        xt, gt = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()
        c = P["params"]["rbf_list"]["centers"]
        runs = {}
        plain = WCRBFNet(**card)
        runs["full"] = (plain, distributed.params_to_device(P))
        fc = WCRBFNet(**card, centers=c, fixed_centers=True)
        runs["no_centres"] = (fc, distributed.params_to_device({"params": {"rbf_list": {"log_sigs": P["params"]["rbf_list"]["log_sigs"]},
                                                                           "linear": P["params"]["linear"]}}))
        fw = WCRBFNet(**card, centers=c, fixed_width=True, log_sigs=P["params"]["rbf_list"]["log_sigs"])
        runs["linear"] = (fw, distributed.params_to_device({"params": {"linear": P["params"]["linear"]}}))
        names = {}
        for k, (net, p) in runs.items():
            net.set_options(vjp_kernel=_lib.VJP_K2G, gram_sticky=1)
            net.bind(p)
            net.vjp(p, xt, gt)
            names[k] = net.last_launch()["kernel"]
        t = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, (net, p) in runs.items():
                t[k].append(t_us(lambda: net.vjp(p, xt, gt), a.reps))
        med = {k: float(np.median(v)) for k, v in t.items()}
        print(f"\n## {title}")
        for k in runs:
            spread = f"{min(t[k]):.1f}-{max(t[k]):.1f}"
            ratio = med[k] / med["full"]
            print(f"{k:11s} {med[k]:7.1f} us  (rounds {spread})  ratio to full {ratio:.3f}  [{names[k]}]", flush=True)


if __name__ == "__main__":
    main()
