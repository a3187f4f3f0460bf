"""DeeperWCRBFNet training on one MI355X (output: profiles/train_deeper.txt).

1. The stage VJP (irbfn_net_vjp on the 64-wide stage) on K2 and on K2m, at B = 80000 (the reference's batch) and 4096, on the
   golden net's stage (K = 100, d = 8, gaussian) and on a 4096-centre d = 8 O = 64 stage: the whole call (query pack, kernel,
   bias column sums, slab reduce) by events, and the K2 / K2m kernel alone from rocprofv3 when run under it.
2. The whole Deeper training step (train_step_frenet_fullint, T = 5) at B = 80000, and the forward + VJP it replaces."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
from conftest import load_deeper_fixture  # noqa: E402
from irbfn_amd import _lib, configs, train  # noqa: E402
from irbfn_amd.model import DeeperWCRBFNet, WCRBFNet  # noqa: E402


def timed(fn, n=20):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


cfg, P, _, _ = load_deeper_fixture()
P32 = {"params": {k: {n: torch.from_numpy(np.asarray(v, np.float32)).cuda() for n, v in d.items()} for k, d in P["params"].items()}}
ns = len(cfg["activation_idx"])
lo = np.array([min(cfg["lower_bounds"][d]) for d in range(ns)]); hi = np.array([max(cfg["upper_bounds"][d]) for d in range(ns)])
rng = np.random.default_rng(0)


def queries(B):
    x = rng.uniform(lo, hi, size=(B, 8)).astype(np.float32)
    x[:, 7] = rng.normal(size=B).astype(np.float32) * 0.05
    x[:, 0] = rng.normal(size=B).astype(np.float32) * 0.2
    return torch.from_numpy(x).cuda()


golden_stage = {"rbf_list": P32["params"]["rbf_list"], "linear": P32["params"]["linear_pre1"]}
big_cfg = dict(cfg, out_features=64, num_kernels=4096)
big = {"rbf_list": {"centers": torch.from_numpy(rng.uniform(lo.min(), hi.max(), size=(1, 4096, 8)).astype(np.float32)).cuda(),
                    "log_sigs": torch.zeros((1, 4096), device="cuda")},
       "linear": {"kernel": torch.randn(4096, 64, device="cuda") / 64, "bias": torch.zeros(64, device="cuda")}}
print("# stage VJP (irbfn_net_vjp, whole call) per kernel; max |K2m - K2| / max |K2| over the four leaves")
for label, scfg, sp in (("golden stage K=100 d=8 O=64", dict(cfg, out_features=64), golden_stage),
                        ("stage K=4096 d=8 O=64", big_cfg, big)):
    net = WCRBFNet.from_config(scfg)
    for B in (80000, 4096):
        x = queries(B)
        g = torch.randn(B, 64, device="cuda")
        res = {}
        for name, k in (("K2", _lib.VJP_K2), ("K2m", _lib.VJP_K2M)):
            net.set_options(vjp_kernel=k)
            t = timed(lambda: net.vjp(sp, x, g))
            res[name] = (t, net.vjp(sp, x, g)["params"], net.last_launch()["kernel"])
        err = max(float((res["K2m"][1][gr][n] - res["K2"][1][gr][n]).abs().max() / res["K2"][1][gr][n].abs().max())
                  for gr, n in (("rbf_list", "centers"), ("rbf_list", "log_sigs"), ("linear", "kernel"), ("linear", "bias")))
        print(f"{label} B={B}: K2 {res['K2'][0]:.1f} us [{res['K2'][2]}]  K2m {res['K2m'][0]:.1f} us [{res['K2m'][2]}]  "
              f"ratio {res['K2m'][0] / res['K2'][0]:.2f}  rel diff {err:.1e}", flush=True)
    net.set_options(vjp_kernel=_lib.VJP_AUTO)

print("# Deeper training step (train_step_frenet_fullint, T = 5, golden net) and the forward + VJP of the previous version")
DP = np.array(configs.DYN_PARAMS)
for B in (80000, 4096):
    x = queries(B)
    T = cfg["out_features"] // 2
    y = torch.from_numpy(np.hstack([rng.normal(size=(B, T)) * 2, rng.normal(size=(B, T)) * 0.5]).astype(np.float32)).cuda()
    net = DeeperWCRBFNet.from_config(cfg)
    st = train.DeeperTrainState.create(net, P, lr=1e-4)
    kern = st.stage_vjp_kernel(B)

    def step():
        global st
        st, _ = train.train_step_frenet_fullint(st, x, y, DP)
    t_step = timed(step)
    ref = DeeperWCRBFNet.from_config(cfg)
    gy = torch.randn(B, cfg["out_features"], device="cuda")
    t_fv = timed(lambda: (ref.apply(P32, x), ref.vjp(P32, x, gy)))
    print(f"B={B}: DeeperTrainState step {t_step:.1f} us (stage VJP {'K2m' if kern == _lib.VJP_K2M else 'auto'}, "
          f"[{net.stage.last_launch()['kernel']}]); apply + vjp as before: {t_fv:.1f} us", flush=True)
