"""Times the closed-form output-layer fit (irbfn_amd/linear_fit.py): the f64 matrix instruction's rate (tools/ubench_mfma_f64.hip,
if its binary is in tools/_bin), then

* ``irbfn_net_hidden`` at B = 65 536, D = 7, K = 1000 and K = 4096 (BASELINE config 2's card and parameter draws at that K), next
  to the forward of the same net;
* ``irbfn_syrk_f64`` at rows = 65 536, M = 1011 and M = 4107, in TFLOP/s counted as rows M (M + 1) flops (the products of one
  triangle and their additions), next to ``Zd = Z.double(); Zd.T @ Zd`` through torch on the same GPU;
* ``fit_linear`` on 2^20 rows at K = 1000, O = 10, D = 7 and, for context, one ``train_epoch`` over the same rows (batches of
  65 536, ``train_step_fullint``).

One warm-up pass over every variant, then ROUNDS interleaved rounds (every variant once per round, INNER calls between two
device events); medians with min / max.  GPU box; output kept as profiles/linear_fit.txt."""
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from irbfn_amd import _lib, configs, linear_fit, tables, train  # noqa: E402
from irbfn_amd.model import WCRBFNet, _ptr, _stream_ptr  # noqa: E402

ROUNDS, INNER = 7, 3
B = 1 << 16
N_FIT = 1 << 20


def span(fn, n):
    fn()
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


def net_of(K):
    """Config 2's card with K kernels and its parameter draws at that K."""
    card = dict(configs.model_card(2), num_kernels=K)
    rng = np.random.default_rng(123)
    lo, hi = np.asarray(configs._LO7), np.asarray(configs._HI7)
    p = {"params": {"rbf_list": {"centers": rng.uniform(lo - 1.0, hi + 1.0, size=(1, K, 7)).astype(np.float32),
                                 "log_sigs": rng.uniform(0.0, 2.0, size=(1, K)).astype(np.float32)},
                    "linear": {"kernel": rng.normal(size=(K, 10)).astype(np.float32),
                               "bias": rng.normal(0.0, 0.1, size=10).astype(np.float32)}}}
    return WCRBFNet.from_config(card), p


def main():
    assert torch.cuda.is_available(), "time_linear_fit.py measures on the GPU"
    ub = os.path.join(ROOT, "tools", "_bin", "ubench_mfma_f64")
    print("== v_mfma_f64_16x16x4_f64 (tools/ubench_mfma_f64.hip)")
    if os.path.exists(ub):
        print(subprocess.run([ub], capture_output=True, text=True, timeout=300).stdout, end="")
    else:
        print("   not built: hipcc --offload-arch=gfx950 -O3 -o tools/_bin/ubench_mfma_f64 tools/ubench_mfma_f64.hip")
    lib = _lib.load()
    stream = _stream_ptr(torch)
    print(f"== on {torch.cuda.get_device_name(0)}: {ROUNDS} rounds x {INNER} calls, median us [min .. max]")
    x = torch.from_numpy(configs.synth_queries(2, B)).cuda()
    print(f"-- irbfn_net_hidden, B = {B}, D = 7, gaussian, one region")
    for K in (1000, 4096):
        net, p = net_of(K)
        net.bind(p)
        h = torch.empty((B, K), dtype=torch.float32, device="cuda")
        res = measure([("irbfn_net_hidden", lambda: net._hidden_into(x, h, torch)), ("irbfn_net_forward (O = 10)", lambda: net(x))])
        for label, (med, lo, hi) in res.items():
            print(f"   K = {K:5d}  {label:28s} {med:10.1f} us  [{lo:.1f} .. {hi:.1f}]   {B * K / med * 1e-6:6.3f} Tpairs/s")
        print(f"   K = {K:5d}  hidden writes {B * K * 4 / 1e6:.0f} MB: {B * K * 4 / res['irbfn_net_hidden'][0] * 1e-6:.2f} TB/s of stores")
    print(f"-- irbfn_syrk_f64, rows = {B}; flops = rows M (M + 1)")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    for M in (1011, 4107):
        Z = torch.randn((B, M), device="cuda", generator=gen)
        G = torch.empty((M, M), dtype=torch.float64, device="cuda")
        ws = torch.empty(lib.irbfn_syrk_f64_workspace_bytes(B, M), dtype=torch.uint8, device="cuda")

        def syrk():
            st = lib.irbfn_syrk_f64(_ptr(Z), M, B, M, _ptr(G), 0, _ptr(ws), ws.numel(), stream)
            assert st == 0, st

        def torch_gram():
            Zd = Z.double()
            return Zd.T @ Zd
        res = measure([("irbfn_syrk_f64", syrk), ("torch Z.double().T @ Z.double()", torch_gram)])
        flops = B * M * (M + 1)
        for label, (med, lo, hi) in res.items():
            print(f"   M = {M:5d}  {label:34s} {med:10.1f} us  [{lo:.1f} .. {hi:.1f}]   {flops / med * 1e-6:6.2f} TFLOP/s")
        a, b = res["irbfn_syrk_f64"][0], res["torch Z.double().T @ Z.double()"][0]
        syrk()
        ref = torch_gram()
        torch.cuda.synchronize()
        print(f"   M = {M:5d}  torch / syrk = {b / a:.2f}; workspace {ws.numel() / 2 ** 20:.0f} MiB (torch: a float64 copy of Z, "
              f"{B * M * 8 / 2 ** 20:.0f} MiB); largest |G - torch| / |torch| = {((G - ref).abs().max() / ref.abs().max()).item():.2e}")
        del Z, G, ws, ref
    print(f"-- end to end: {N_FIT} rows, K = 1000, O = 10, D = 7")
    net, p = net_of(1000)
    xf = torch.from_numpy(configs.synth_queries(2, N_FIT)).cuda()
    yf = net.apply(p, xf) + 0.05 * torch.randn((N_FIT, 10), device="cuda", generator=gen)
    table = tables.DeviceTable(xf.cpu().numpy(), yf.cpu().numpy())
    state = [train.TrainState.create(net, p, lr=1e-3, max_grad_norm=1.0)]

    def epoch():
        state[0], losses = train.train_epoch(state[0], table, B)
        return losses
    fit = [None]

    def do_fit():
        fit[0] = linear_fit.fit_linear(net, p, xf, yf)[1]
    for label, fn in (("fit_linear (16 chunks of 65 536, solve included)", do_fit), ("train_epoch (16 steps of 65 536, train_step_fullint)", epoch)):
        fn()
        torch.cuda.synchronize()
        walls = []
        for _ in range(3):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
        print(f"   {label:56s} wall {np.median(walls) * 1e3:8.1f} ms  [{min(walls) * 1e3:.1f} .. {max(walls) * 1e3:.1f}]")
    print(f"   fit: n = {fit[0].n}, mse = {fit[0].mse:.6e} (label noise 0.05^2 = 2.5e-3), ridge_abs = {fit[0].ridge_abs:.3e}")


if __name__ == "__main__":
    main()
