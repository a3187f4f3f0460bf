"""Times the Frenet NMPC solver (irbfn_nmpc_solve_frenet, K15; irbfn_amd/nmpc.py) on one GPU and reports what it does.

  regs  : registers and scratch of every instance of nmpc_solve_kernel, from hipcc's resource remarks with build.py's flags
          (no GPU needed).
  solve : one nmpc.solve_frenet call on the `reg` family (tests/_nmpc_frenet_util.py), T = 5, max_iter = 30, B = 2^16 and 2^20,
          next to one nmpc.solve call with ST_KS on its own `reg` family (tests/_nmpc_util.py) at the same B and T, interleaved.
  table : the label-table chain of tests/test_gpu_nmpc_frenet.py (make_table_frenet -> kmeans -> closed-form output layer).
  loop  : a 1000-tick nmpc.closed_loop_frenet at B = 1024 on the ellipse of tools/closed_loop_frenet_timing.py, next to
          nmpc.closed_loop on the same line, cars and plant.

Without arguments every step runs as a child process under its own time limit, the first failure ends the run, and
profiles/nmpc_frenet.txt (or the file after ``--out``) is written afresh.  ``--step NAME`` runs one step in this process."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

STEPS = (("regs", 300), ("solve", 300), ("table", 120), ("loop", 300))      # (name, seconds)
T = 5
ROUNDS = 7
PREAMBLE = """\
Frenet NMPC solver (irbfn_amd/nmpc.py, irbfn_nmpc_solve_frenet = csrc/nmpc_solve.hip, K15): registers, times on one GPU and what
the controller does, written by tools/nmpc_frenet_timing.py.  Every step is a process of its own under its own time limit.
"solve" = one call (one launch), start u0 = 0, T = 5, max_iter = 30, tol = 1e-6, timed between two device events over several
calls after a warm-up of each; median of 7 rounds, the two solvers alternating within a round [min .. max].
  frenet : nmpc.solve_frenet on the `reg` family of tests/_nmpc_frenet_util.py (seed 123)
  st_ks  : nmpc.solve, ST_KS, on the `reg` family of tests/_nmpc_util.py (seed 123)
The two solve different problems and take different numbers of iterations: no ratio of the times is claimed.  rows x iterations
/ s counts the iterations the rows actually took and is the comparable figure.
"table" = 4096 `reg` queries -> nmpc.make_table_frenet -> kmeans.fit (64 centres, on the first three quarters of the rows) ->
linear_fit.fit_linear; RMS control error on the last quarter.
"loop" = 1000 ticks at B = 1024 on the ellipse of tools/closed_loop_frenet_timing.py (semi-axes 12 m and 8 m, N = 1000, line speed
4 m/s, lookahead 1 m, half width 3 m), the same cars and plant (ST_SELECT) as its golden-net runs; one host clock around the call
and a device synchronise, median of 3 alternating rounds.  The summary lines are SimResult.summary(): a report, no claim.  The
golden Frenet nets' figures on this line are in profiles/closed_loop_frenet.txt.
Not measured: kernel time apart from launch gaps (no profiler run), PMC counters, the clocks under load.

"""


def timed(torch, fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps                            # milliseconds per call


def fmt(v):
    v = sorted(v)
    return f"{v[len(v) // 2]:9.3f} ms [{v[0]:.3f} .. {v[-1]:.3f}]"


def step_regs():
    from irbfn_amd import build
    unit = next(u for u in build.UNITS if u[0] == "nmpc_solve.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = build.compile_cmd(unit[0], unit[2] + ["-Rpass-analysis=kernel-resource-usage"], ["-c"], os.path.join(tmp, "nmpc.o"))
        r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        print(r.stderr[-2000:])
        sys.exit(1)
    names = {"0": "ST_SELECT", "1": "ST_KS", "3": "FRENET_LS"}
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: _ZN5irbfn17nmpc_solve_kernelILi(\d+)ELi(\d+)EEE", line)
        if m:
            cur = dict(mode=names[m.group(1)], T=int(m.group(2)))
            rows.append(cur)
            continue
        for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("agpr", r"AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occ", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = m.group(1)
    print("registers of csrc/nmpc_solve.hip (hipcc -Rpass-analysis=kernel-resource-usage, build.py's flags, gfx950): "
          "VGPRs + AGPRs, scratch bytes / lane, waves / SIMD")
    print("   T   " + "".join(f"{n:>32s}" for n in ("FRENET_LS", "ST_KS", "ST_SELECT")))
    for t in range(1, 9):
        cells = []
        for n in ("FRENET_LS", "ST_KS", "ST_SELECT"):
            c = next(x for x in rows if x["mode"] == n and x["T"] == t)
            cells.append(f"{c['vgpr']:>4s} + {c['agpr']:>3s}, scratch {c['scratch']}, occ {c['occ']}")
        print(f"   {t}   " + "".join(f"{c:>32s}" for c in cells))
    print(flush=True)


def step_solve():
    import torch
    from irbfn_amd import _lib, nmpc
    import _nmpc_frenet_util as fu
    import _nmpc_util as nu
    dp = nu.DP
    up = lambda a: torch.from_numpy(a.astype(np.float32)).cuda()
    for logB in (16, 20):
        B = 1 << logB
        reps = 10 if logB == 16 else 3
        fs0, fgoal, fW = fu.family("reg", B, T, seed=123)
        ks0, kgoal, kW = nu.family("reg", B, T, seed=123, select=False)
        fsd, fgd, ksd, kgd = up(fs0), up(fgoal), up(ks0), up(kgoal)
        runs = {"frenet": lambda: nmpc.solve_frenet(fsd, fgd, dp, T=T, weights=nmpc.FrenetWeights(**fW), **nu.DEFAULTS),
                "st_ks": lambda: nmpc.solve(ksd, kgd, dp, T=T, weights=nmpc.Weights(**kW), mode=_lib.ROLLOUT_ST_KS, **nu.DEFAULTS)}
        res = {n: f() for n, f in runs.items()}                # warm-up of each
        torch.cuda.synchronize()
        ms = {n: [] for n in runs}
        for _ in range(ROUNDS):
            for n, f in runs.items():
                ms[n].append(timed(torch, f, reps))
        print(f"solve    B = 2^{logB}, T = {T}, max_iter = {nu.DEFAULTS['max_iter']}")
        for n in runs:
            it = res[n].iterations.double()
            med = sorted(ms[n])[ROUNDS // 2]
            print(f"  {n:7s} {fmt(ms[n])}   iterations mean {float(it.mean()):.2f} max {int(it.max())}   "
                  f"{float(it.sum()) / (med * 1e-3):.3e} rows x iterations / s   status counts "
                  f"{torch.bincount(res[n].status, minlength=4).tolist()}")
        print(flush=True)


def step_table():
    from irbfn_amd import kmeans, linear_fit, nmpc, tables
    from irbfn_amd.model import WCRBFNet
    import _nmpc_frenet_util as fu
    N, K = 4096, 64
    s0, goal, W = fu.family("reg", N, T, seed=77)
    x = np.zeros((N, 8), np.float32)
    x[:, 0:3], x[:, 4], x[:, 6:8] = s0[:, 1:4], goal[:, 3], s0[:, 6:8]
    inputs, outputs = nmpc.make_table_frenet(x, fu.DP, T=T, weights=nmpc.FrenetWeights(**W))
    xi, yo, valid = tables.remove_infeasible(inputs, outputs)
    y = tables.flatten_outputs(yo)
    n_fit = (3 * len(xi)) // 4
    centers = kmeans.fit(xi[:n_fit], K, max_iter=20, seed=1).centers.cpu().numpy()
    cfg = dict(in_features=8, out_features=2 * T, num_kernels=K, basis_func="gaussian", num_regions=1, lower_bounds=[[-50.0]] * 8,
               upper_bounds=[[50.0]] * 8, dimension_ranges=[[0] * 8], activation_idx=list(range(8)), delta=[100.0] * 8)
    net = WCRBFNet.from_config(cfg)
    p = net.init()
    p["params"]["rbf_list"]["centers"] = centers[None].astype(np.float32)
    p["params"]["rbf_list"]["log_sigs"] = np.zeros((1, K), np.float32)
    new, _ = linear_fit.fit_linear(net, p, xi[:n_fit], y[:n_fit])
    out = np.asarray(net.apply(new, xi[n_fit:]), np.float64)
    rms_net = np.sqrt(((out - y[n_fit:]) ** 2).mean())
    rms_mean = np.sqrt(((y[n_fit:] - y[:n_fit].mean(0)) ** 2).mean())
    print(f"table    {N} `reg` queries (seed 77), T = {T}: {N - len(valid)} rows not converged, {len(valid)} kept")
    print(f"  held-out RMS control error ({len(xi) - n_fit} rows): fitted 8-input net ({K} Gaussian centres) {rms_net:.4f}, "
          f"mean predictor {rms_mean:.4f}")
    print(flush=True)


def step_loop():
    import time

    import torch
    from irbfn_amd import configs, nmpc, simulate
    from closed_loop_frenet_timing import N_WAY, brief, cars, ellipse
    track = simulate.Track(ellipse(N_WAY), wrap=True, lookahead=1.0, max_reacquire=4.0, half_width=3.0)
    p, ticks, B = configs.DYN_PARAMS, 1000, 1024
    st = torch.from_numpy(cars(track, B)).cuda()
    q = (0.0, 0.5, 0.9, 1.0)

    def clock(fn):
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res
    runs = {"nmpc.closed_loop_frenet (Frenet model, FrenetWeights)": lambda: nmpc.closed_loop_frenet(track, st, ticks, p, T=T),
            "nmpc.closed_loop (ST_SELECT model, Weights)": lambda: nmpc.closed_loop(track, st, ticks, p, T=T)}
    ts, res = {n: [] for n in runs}, {}
    for n, f in runs.items():
        clock(f)
    for _ in range(3):
        for n, f in runs.items():
            t, res[n] = clock(f)
            ts[n].append(t)
    print(f"loop     B = {B}, N = {N_WAY}, {ticks} ticks, T = {T}, plant ST_SELECT")
    for n in runs:
        med = sorted(ts[n])[1]
        s = res[n].summary(q)
        print(f"  {n}")
        print(f"    {med * 1e3:9.1f} ms [{min(ts[n]) * 1e3:.1f} .. {max(ts[n]) * 1e3:.1f}]   {med / ticks * 1e6:8.1f} us per tick")
        print(f"    {brief(s)}; rms_dev quantiles (0, 0.5, 0.9, 1) {['%.3f' % v for v in s['rms_dev']]}")
    print(flush=True)


def main():
    args = sys.argv[1:]
    if "--step" in args:
        {"regs": step_regs, "solve": step_solve, "table": step_table, "loop": step_loop}[args[args.index("--step") + 1]]()
        return 0
    out = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "nmpc_frenet.txt")
    text = PREAMBLE
    for name, limit in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name],
                           capture_output=True, text=True)
        text += r.stdout
        if r.returncode != 0:
            text += f"step {name} ended with status {r.returncode}\n{r.stderr[-2000:]}\n"
        open(out, "w").write(text)                             # after every step: a later one that fails loses nothing
        if r.returncode != 0:
            print(text)
            return 1
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
