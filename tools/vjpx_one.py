"""ONE query-VJP (or K1 forward) kernel on ONE BASELINE config, N launches: the unit of a rocprofv3 summary or counter pass
    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python3 tools/vjpx_one.py <config 2|4> <B> <k5|k5m|k1> [launches]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from irbfn_amd import _lib, configs, distributed  # noqa: E402
from irbfn_amd.model import WCRBFNet  # noqa: E402

idx, B, what = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
n = int(sys.argv[4]) if len(sys.argv) > 4 else 20
net = WCRBFNet.from_config(configs.model_card(idx))
P = distributed.params_to_device(configs.synth_params(idx))
x = torch.from_numpy(configs.synth_queries(idx, B=B)).cuda()
g = torch.from_numpy(configs.synth_cotangent(idx, B=B)).cuda()
if what == "k1":
    net.set_options(fwd_kernel=_lib.FWD_K1)
    fn = lambda: net.apply(P, x)
else:
    net.set_options(vjpx_kernel=_lib.VJPX_K5M if what == "k5m" else _lib.VJPX_K5)
    fn = lambda: net.vjp_x(P, x, g)
for _ in range(n):
    fn()
torch.cuda.synchronize()
print(net.last_launch())
