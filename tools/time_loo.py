"""Times the leave-one-out pass of the closed-form fit (irbfn_amd/loo.py, kernel K11 ``irbfn_rows_quad_f64``):

* K11 at rows = 65 536, m = 1001 and m = 4097, nd = 10, in TFLOP/s counted as rows m (m + 1 + 2 nd) flops (the products of the
  triangle and of the dense columns, and their additions); interleaved with it in the same process ``irbfn_syrk_f64`` of the same
  rows and M = m + nd (the same number of products: the yardstick) and the torch baseline
  ``U = Z[:, :m].double() @ P; q = (U[:, :m] ** 2).sum(1)``;
* ``loo.loo`` on 2^20 rows at K = 1000, O = 10, D = 7 (factor apart), next to ``fit_linear`` on the same rows;
* ``loo.select_scale`` (all rows, PRESS) next to ``widths.select_scale`` (a fifth held out) on the same inputs.

The timer is ``measure`` of tools/time_linear_fit.py: one warm-up pass over every variant, then ROUNDS interleaved rounds, INNER
calls between two device events; medians with min / max.  GPU box; the output is printed and kept as profiles/loo.txt (or the
file after ``--out``)."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from irbfn_amd import _lib, configs, linear_fit, loo, widths  # noqa: E402
from irbfn_amd.model import WCRBFNet, _ptr, _stream_ptr  # noqa: E402
from time_linear_fit import B, N_FIT, INNER, ROUNDS, measure, net_of  # noqa: E402

ND = 10
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def wall(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), min(t), max(t)


def main():
    assert torch.cuda.is_available(), "time_loo.py measures on the GPU"
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "loo.txt")
    lib = _lib.load()
    stream = _stream_ptr(torch)
    say(f"== tools/time_loo.py on {torch.cuda.get_device_name(0)}: {ROUNDS} rounds x {INNER} calls, median us [min .. max]")
    say(f"-- irbfn_rows_quad_f64 (K11), rows = {B}, nd = {ND}; flops = rows m (m + 1 + 2 nd)")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    for m in (1001, 4097):
        M = m + ND
        Z = torch.randn((B, M), device="cuda", generator=gen)
        P = torch.randn((m, M), dtype=torch.float64, device="cuda", generator=gen) / m ** 0.5
        Pt = torch.cat([torch.triu(P[:, :m]), P[:, m:]], dim=1)             # what the kernel reads of P
        q = torch.empty((B,), dtype=torch.float64, device="cuda")
        v = torch.empty((B, ND), dtype=torch.float64, device="cuda")
        G = torch.empty((M, M), dtype=torch.float64, device="cuda")
        ws = torch.empty(lib.irbfn_syrk_f64_workspace_bytes(B, M), dtype=torch.uint8, device="cuda")

        def k11():
            st = lib.irbfn_rows_quad_f64(_ptr(Z), M, B, m, _ptr(P), M, ND, _ptr(q), _ptr(v), stream)
            assert st == 0, st

        def syrk():
            st = lib.irbfn_syrk_f64(_ptr(Z), M, B, M, _ptr(G), 0, _ptr(ws), ws.numel(), stream)
            assert st == 0, st

        def torch_quad():
            U = Z[:, :m].double() @ Pt
            return (U[:, :m] ** 2).sum(1), U[:, m:]
        res = measure([("irbfn_rows_quad_f64", k11), ("irbfn_syrk_f64 (M = m + nd)", syrk), ("torch Z.double() @ P, squares summed", torch_quad)])
        flops = B * m * (m + 1 + 2 * ND)
        for label, (med, lo, hi) in res.items():
            say(f"   m = {m:5d}  {label:40s} {med:10.1f} us  [{lo:.1f} .. {hi:.1f}]   {flops / med * 1e-6:6.2f} TFLOP/s")
        a, s, t = (res[k][0] for k in ("irbfn_rows_quad_f64", "irbfn_syrk_f64 (M = m + nd)", "torch Z.double() @ P, squares summed"))
        k11()
        qr, vr = torch_quad()
        torch.cuda.synchronize()
        say(f"   m = {m:5d}  K11 / syrk = {a / s:.2f}; torch / K11 = {t / a:.2f} (torch: a float64 copy of Z and U, {2 * B * M * 8 / 2 ** 20:.0f} MiB; "
            f"K11: none); largest |q - torch| / |torch| = {((q - qr).abs().max() / qr.abs().max()).item():.2e}, "
            f"|v - torch| / |torch| = {((v - vr).abs().max() / vr.abs().max()).item():.2e}")
        del Z, P, Pt, q, v, G, ws, qr, vr
    say(f"-- end to end: {N_FIT} rows, K = 1000, O = 10, D = 7, chunks of {B}; wall ms, median of 3 [min .. max]")
    net, p = net_of(1000)
    xf = torch.from_numpy(configs.synth_queries(2, N_FIT)).cuda()
    yf = net.apply(p, xf) + 0.05 * torch.randn((N_FIT, 10), device="cuda", generator=gen)
    ne = linear_fit.NormalEquations(net).add(p, xf, yf)
    keep = {}

    def do_factor():
        keep["fac"] = loo.factor(ne)

    def do_loo():
        keep["res"] = loo.loo(net, p, xf, yf, keep["fac"])

    def do_lev():
        keep["lev"] = loo.leverage(net, p, xf, keep["fac"])

    def do_fit():
        keep["fit"] = linear_fit.fit_linear(net, p, xf, yf)[1]
    for label, fn in (("fit_linear (16 chunks, solve included)", do_fit), ("loo.factor (solve's steps + one triangular solve)", do_factor),
                      ("loo.loo (16 chunks: hidden, K11, residuals)", do_loo), ("loo.leverage (16 chunks: hidden, K11)", do_lev)):
        med, lo, hi = wall(fn)
        say(f"   {label:56s} {med:8.1f} ms  [{lo:.1f} .. {hi:.1f}]")
    r, fit = keep["res"], keep["fit"]
    say(f"   fit mse {fit.mse:.6e}; loo: rss / (n O) {float(r.rss.sum()) / (r.n * 10):.6e}, PRESS / (n O) {r.press_mse:.6e}, trace {float(r.trace):.3f}, "
        f"max leverage {float(r.max_leverage):.4f}, degenerate rows {int(r.n_degenerate)}")
    say("-- the width multiplier: loo.select_scale (all rows, PRESS) next to widths.select_scale (every fifth row held out); same rows, "
        "1000 centres on rows of x, widths from the 2 nearest centres, scales (0.5, 1, 2, 4, 8)")
    rng = np.random.default_rng(5)
    centers = xf[torch.from_numpy(rng.choice(N_FIT, 1000, replace=False)).cuda()].cpu().numpy()
    net0 = WCRBFNet.from_config(dict(net.config(), fixed_centers=True, fixed_width=True), centers=centers)
    w = widths.nearest_neighbour(centers, p=2)

    def by_loo():
        keep["sl"] = loo.select_scale(net0, w, xf, yf)

    def by_holdout():
        keep["sh"] = widths.select_scale(net0, w, xf, yf)
    fmt = lambda v: " ".join(f"{e:.4e}" for e in v)                          # noqa: E731
    for label, fn, key, what in (("loo.select_scale", by_loo, "sl", "leave-one-out MSE per scale"),
                                 ("widths.select_scale", by_holdout, "sh", "held-out MSE per scale     ")):
        try:
            med, lo, hi = wall(fn)
        except ValueError as e:            # every scale refused: said, not hidden
            say(f"   {label:56s} refused: {e}")
            continue
        say(f"   {label:56s} {med:8.1f} ms  [{lo:.1f} .. {hi:.1f}]")
        say(f"   {what} {fmt(keep[key].holdout_mse)} -> scale {keep[key].best_scale:g}")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
