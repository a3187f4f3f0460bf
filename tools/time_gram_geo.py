"""K1g launch geometries (timing only): python tools/time_gram_geo.py [--B n] [--trained] [--geo S,QG ...]
Default: config 2 at its own batch over five geometries.  --B: another batch (config-2 queries, tiled).  --trained: the reference's
trained one-region planner (tests/golden, N = 1000) on queries drawn inside its bounds.  --geo 0,0: the planner's own choice."""
import argparse, json, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from irbfn_amd import _lib, configs, distributed  # noqa: E402
from irbfn_amd.model import WCRBFNet  # noqa: E402
from tools.time_gram import t_us  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=0)
ap.add_argument("--trained", action="store_true")
ap.add_argument("--geo", nargs="*", default=["2,4", "1,4", "1,8", "2,2", "4,2"])
a = ap.parse_args()
if a.trained:
    run = "dnmpc_1regions_newdata_oldintloss_nomirror_highk"
    g = os.path.join(ROOT, "tests", "golden")
    z, cfg = np.load(os.path.join(g, f"ckpt_{run}.npz")), json.load(open(os.path.join(g, f"ckpt_{run}.json")))
    P = {"params": {"rbf_list": {"centers": z["centers"].astype(np.float32), "log_sigs": z["log_sigs"].astype(np.float32)},
                    "linear": {"kernel": z["kernel"].astype(np.float32), "bias": z["bias"].astype(np.float32)}}}
    ns = len(cfg["activation_idx"])
    lo, hi = np.array([min(cfg["lower_bounds"][d]) for d in range(ns)]), np.array([max(cfg["upper_bounds"][d]) for d in range(ns)])
    xq = np.random.default_rng(0).uniform(lo, hi, size=(a.B or 80000, cfg["in_features"])).astype(np.float32)
else:
    cfg, P = configs.model_card(2), configs.synth_params(2)
    xq = configs.synth_queries(2)
    if a.B:
        xq = np.tile(xq, ((a.B + len(xq) - 1) // len(xq), 1))[:a.B]
net = WCRBFNet.from_config(cfg); net.bind(distributed.params_to_device(P))
x = torch.from_numpy(np.ascontiguousarray(xq)).cuda()
out = []
for S, QG in (tuple(int(v) for v in s.split(",")) for s in a.geo):
    net.set_options(fwd_kernel=_lib.FWD_K1G, fwd_f16_s=S, fwd_f16_qg=QG)
    try:
        t = sorted(t_us(lambda: net(x)) for _ in range(5))
        out.append(f"{net.last_launch()['kernel']}: min {t[0]:.1f} median {t[2]:.1f} max {t[4]:.1f}")
    except Exception as e:
        out.append(f"S={S} QG={QG}: {str(e)[:60]}")
print(os.environ.get("IRBFN_LIB", "regular"), f"N={cfg['num_kernels']} B={len(xq)}", " | ".join(out), flush=True)
