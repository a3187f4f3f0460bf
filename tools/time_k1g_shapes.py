"""K1g at the shapes of profiles/k1g_loop_addresses.txt section D, one process per call: us per launch as min / median / max of five
timings of 50 launches (the timer of tools/time_gram.py).  ``--root DIR`` times the package of another checkout (an A/B against
the parent: alternate processes of the two trees in one job).

  forward   config 2 (N = 4096) at B = 16 384, 49 152, 65 536; its first 2048 centres at B = 65 536; the trained single-region
            planner of tests/golden (N = 1000) at B = 65 536 and 80 000; config 5; config 4 (O = 100: the wide forward)
  tick      planner.plan_tick on config 2 at B = 65 536, with its host work
  gamma     irbfn_net_forward_gamma on K1g at R = 8, K = 128, D = 8, B = 65 536"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
TAG = sys.argv[sys.argv.index("--tag") + 1] if "--tag" in sys.argv else os.path.basename(ROOT)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from _cluster_util import cluster_case  # noqa: E402
from conftest import load_ckpt_fixture  # noqa: E402
from irbfn_amd import _lib, configs, distributed  # noqa: E402
from irbfn_amd.model import ClusterWCRBFNet, WCRBFNet, _ptr, _stream_ptr  # noqa: E402
from irbfn_amd.planner import plan_tick  # noqa: E402
from oracle import irbfn_oracle as orc  # noqa: E402


def t_us(fn, reps=50):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def report(what, fn, last_launch):
    v = [t_us(fn) for _ in range(5)]
    print(f"{TAG}: {what} {last_launch()['kernel']}: min {min(v):.1f} median {float(np.median(v)):.1f} max {max(v):.1f}", flush=True)


def forward(what, cfg, P, x):
    net = WCRBFNet.from_config(cfg)
    net.bind(distributed.params_to_device(P))
    xt = torch.from_numpy(x).cuda()
    report(f"forward {what} B={x.shape[0]}", lambda: net(xt), net.last_launch)
    return net, xt


def main():
    cfg, P = configs.model_card(2), configs.synth_params(2)
    half = {"params": {"rbf_list": {k: v[:, :2048].copy() for k, v in P["params"]["rbf_list"].items()},
                       "linear": {"kernel": P["params"]["linear"]["kernel"][:2048].copy(), "bias": P["params"]["linear"]["bias"]}}}
    forward("N=2048", dict(cfg, num_kernels=2048), half, configs.synth_queries(2, B=65536))
    for B in (16384, 49152, 65536):
        net, xt = forward("N=4096", cfg, P, configs.synth_queries(2, B=B))
    B = 65536
    rng = np.random.default_rng(0)
    st = torch.from_numpy(np.hstack([rng.normal(size=(B, 3)) * 0.3, rng.uniform(0.5, 7.0, size=(B, 1)), rng.normal(size=(B, 3)) * 0.2]).astype(np.float32)).cuda()
    mt = torch.from_numpy((rng.random(B) < 0.5).astype(np.int32)).cuda()
    report(f"tick N=4096 B={B}", lambda: plan_tick(net, P, xt, mt, st, configs.DYN_PARAMS, mode=_lib.ROLLOUT_ST_KS), net.last_launch)

    tcfg, tP, *_ = load_ckpt_fixture("dnmpc_1regions_newdata_oldintloss_nomirror_highk")
    ns = len(tcfg["activation_idx"])
    lo = np.array([min(tcfg["lower_bounds"][d]) for d in range(ns)]); hi = np.array([max(tcfg["upper_bounds"][d]) for d in range(ns)])
    for B in (65536, 80000):
        x = np.random.default_rng(B).uniform(lo, hi, size=(B, tcfg["in_features"])).astype(np.float32)
        forward("trained N=1000", tcfg, orc.cast_params(tP, np.float32), x)

    R, K, B = 8, 128, 65536
    rng, ccfg, cP, x = cluster_case(7, R=R, K=K, O=10, B=B, D=8)
    cP["params"]["rbf_list"]["log_sigs"] = rng.uniform(0.0, 1.0, size=(R, K)).astype(np.float32)
    cnet = ClusterWCRBFNet(**ccfg).set_options(fwd_gamma_kernel=_lib.FWDG_K1G)
    xt = torch.from_numpy(x).cuda()
    _, gt = cnet._bind_and_gate(cP, xt, torch, _lib.load())
    out = torch.empty((B, 10), dtype=torch.float32, device="cuda")
    lib, h = _lib.load(), cnet.stage._handle(torch)
    report(f"gamma R={R} K={K} B={B}",
           lambda: _lib.check(lib.irbfn_net_forward_gamma(h, _ptr(xt), _ptr(gt), _ptr(out), B, _stream_ptr(torch)), "irbfn_net_forward_gamma"),
           cnet.stage.last_launch)

    for ci in (5, 4):
        B = min(configs.batch_size(ci), 1 << 20)
        forward(f"config {ci}", configs.model_card(ci), configs.synth_params(ci), configs.synth_queries(ci, B=B))


if __name__ == "__main__":
    main()
