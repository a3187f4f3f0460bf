"""Phase timings inside rbf_fwd_f16gram (diagnosis build):
   python tools/build_variant.py gstamps rbf_forward_gram.hip -DIRBFN_GRAM_STAMPS
   IRBFN_LIB=tools/_bin/libirbfn_gstamps.so python tools/gram_stamps.py [S QG]
Per geometry: the phases of a step (ticks per step) and the phases of the launch -- s_memtime of wave 0 of blocks 0 and 1 at
kernel entry, query operands ready, first barrier passed, loop start, loop end, gate done, last store, as shader cycles since
entry and, scaled by the s_memrealtime (100 MHz) span of the same wave, as microseconds."""
import ctypes as C, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from irbfn_amd import _lib, configs, distributed  # noqa: E402
from irbfn_amd.model import WCRBFNet  # noqa: E402
PHASES = ("entry", "operands ready", "first barrier", "loop start", "loop end", "gate done", "last store")
cfg, P = configs.model_card(2), configs.synth_params(2)
net = WCRBFNet.from_config(cfg); net.bind(distributed.params_to_device(P))
x = torch.from_numpy(configs.synth_queries(2)).cuda()
lib = _lib.load()
geos = ((int(sys.argv[1]), int(sys.argv[2])),) if len(sys.argv) > 2 else ((2, 4), (1, 4), (2, 8), (1, 8))
for S, QG in geos:
    net.set_options(fwd_kernel=_lib.FWD_K1G, fwd_f16_s=S, fwd_f16_qg=QG)
    for _ in range(10):
        net(x)
    torch.cuda.synchronize()
    buf = (C.c_ulonglong * 64)()
    assert lib.irbfn_debug_gram_stamps(buf) == 0
    for b in (0, 1):
        t = np.array(buf[b * 32:b * 32 + 5], dtype=np.float64)
        n = max(t[4], 1)
        print(f"S={S} QG={QG} block {b}: steps {int(t[4])}; ticks per step: A reads + distance MFMAs issued {t[0]/n:.0f} | trans + split + PhiW {t[1]/n:.0f} | "
              f"waitcnt + barrier {t[2]/n:.0f} | DMA issue {t[3]/n:.0f} | total {t[:4].sum()/n:.0f}", flush=True)
        ph = np.array(buf[b * 32 + 8:b * 32 + 15], dtype=np.float64) - float(buf[b * 32 + 8])
        real_us = (float(buf[b * 32 + 17]) - float(buf[b * 32 + 16])) / 100.0
        us = ph * (real_us / ph[-1]) if ph[-1] > 0 else ph * 0
        print(f"S={S} QG={QG} block {b}: launch phases, wave 0 ({real_us:.2f} us entry to last store):")
        for k, name in enumerate(PHASES):
            d = ph[k] - ph[k - 1] if k else 0.0
            print(f"    {name:15s} at {ph[k]:9.0f} cycles ({us[k]:6.2f} us)   +{d:8.0f} cycles (+{d * (real_us / ph[-1]) if ph[-1] > 0 else 0:5.2f} us)", flush=True)
