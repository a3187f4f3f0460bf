"""What the pack costs: irbfn_net_set_params (through net.bind with two alternating parameter sets) at config 2 and config 4, and
train_step_oneint at config 3, which re-packs every step; us as min / median / max of five timings.  The package of the WORKING
DIRECTORY is timed, so an A/B against another checkout alternates processes:  (cd TREE && python THIS_FILE TAG)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402
from irbfn_amd import configs, distributed, train  # noqa: E402
from irbfn_amd.model import WCRBFNet  # noqa: E402

TAG = sys.argv[1]


def t_us(fn, reps):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


for ci in (2, 4):
    cfg, P = configs.model_card(ci), configs.synth_params(ci)
    P2 = {"params": {"rbf_list": {k: (v + np.float32(1e-3)) for k, v in P["params"]["rbf_list"].items()}, "linear": P["params"]["linear"]}}
    a, b = distributed.params_to_device(P), distributed.params_to_device(P2)
    net = WCRBFNet.from_config(cfg)
    state = {"i": 0}

    def rebind():
        state["i"] ^= 1
        net.bind(b if state["i"] else a)
    v = [t_us(rebind, 40) for _ in range(5)]
    print(f"{TAG}: bind (irbfn_net_set_params) config {ci}: min {min(v):.1f} median {float(np.median(v)):.1f} max {max(v):.1f} us", flush=True)

cfg = configs.model_card(3)
net = WCRBFNet.from_config(cfg)
x = torch.from_numpy(configs.synth_queries(3)).cuda()
yt = torch.from_numpy(configs.synth_cotangent(3)).cuda()
st = train.TrainState.create(net, configs.synth_params(3), lr=1e-3, max_grad_norm=1.0)
v = [t_us(lambda: train.train_step_oneint(st, x, yt, configs.DYN_PARAMS), 20) for _ in range(5)]
print(f"{TAG}: cfg3 train_step_oneint B={x.shape[0]}: min {min(v):.1f} median {float(np.median(v)):.1f} max {max(v):.1f} us", flush=True)
