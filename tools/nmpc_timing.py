"""Times the batched NMPC solver (irbfn_nmpc_solve, irbfn_amd/nmpc.py) on one GPU.

  solve : one nmpc.solve call on the `reg` family (tests/_nmpc_util.py), T = 5, B = 2^16 and 2^20, both models; next to it the
          float32 statement of the same rule in batched torch ops (kinematic model; torch.linalg.cholesky_ex / cholesky_solve,
          masks instead of branches, no host read, so every row runs all max_iter iterations).
  loop  : one nmpc.closed_loop of 1000 ticks at B = 1024 on the line of tools/closed_loop_timing.py.

Without arguments every step runs as a child process under its own time limit, the first failure ends the run, and
profiles/nmpc.txt (or the file after ``--out``) is written afresh.  ``--step NAME`` runs one step in this process."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STEPS = (("solve", 500), ("loop", 300))                        # (name, seconds)
T = 5
PREAMBLE = """\
Batched NMPC solver (irbfn_amd/nmpc.py, irbfn_nmpc_solve = csrc/nmpc_solve.hip, K13): times on one GPU, written by
tools/nmpc_timing.py.  Every step is a process of its own under its own time limit.
"solve" = one nmpc.solve call (one launch) on the `reg` family of tests/_nmpc_util.py: state0 = [0, 0, 0, v, 0, 0, 0], v ~ U(0.5, 6),
goal = the end of a random roll-out, start u0 = 0, T = 5, max_iter = 30, tol = 1e-6; timed between two device events over several
calls after a warm-up, median of 5 rounds [min .. max].  rows x iterations / s counts the iterations the rows actually took.
"torch" = the float32 statement of the same rule in batched torch ops on the same GPU (kinematic model only): roll-out,
sensitivities, H and g by einsum, torch.linalg.cholesky_ex + cholesky_solve, accept / reject by masks, nothing read by the host --
so it runs max_iter = 30 iterations for every row; its final costs are compared with the kernel's.
"loop" = nmpc.closed_loop for 1000 ticks (simulate.advance + nmpc.solve + the warm-start shift per tick), one host clock around
the call and a device synchronise, median of 3.
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


def torch_solve_ks(torch, s0, goal, dp, W, max_iter=30, lambda0=1e-3, lambda_min=1e-9, lambda_max=1e6, tol=1e-6, eps=1e-6):
    """tests/_nmpc_util.py: solve, kinematic model, float32 torch ops, masks for every branch"""
    s0 = s0[:, :5].contiguous()                                # the kinematic model never moves psi_dot and beta
    B, N = s0.shape[0], 2 * T
    f = lambda v: torch.tensor(v, dtype=torch.float32, device=s0.device)
    dt, svm, am, sm, vm, Lw = (float(np.float32(x)) for x in (dp[8], dp[9], dp[10], dp[11], dp[12], np.float32(dp[4]) + np.float32(dp[3])))
    hi = f([am] * T + [svm] * T)
    q, qf = f(np.asarray(W["q"], np.float32)), f(np.asarray(W["qf"], np.float32))
    Hc = np.zeros((N, N), np.float32)
    for o, k in ((0, 0), (T, 1)):
        for t in range(T):
            Hc[o + t, o + t] += np.float32(W["r"][k])
        for t in range(T - 1):
            Hc[o + t, o + t] += np.float32(W["rd"][k])
            Hc[o + t + 1, o + t + 1] += np.float32(W["rd"][k])
            Hc[o + t, o + t + 1] -= np.float32(W["rd"][k])
            Hc[o + t + 1, o + t] -= np.float32(W["rd"][k])
    Hc = f(Hc)
    comp = [0, 1, 4, 3]
    two_pi = 2.0 * np.pi

    def step(s, a, sv):
        D, V, psi = s[:, 2].clamp(-sm, sm), s[:, 3].clamp(-vm, vm), s[:, 4]
        return s + dt * torch.stack([V * torch.cos(psi), V * torch.sin(psi), sv, a, (V / Lw) * torch.tan(D)], dim=1)

    def resid(s):
        e = s[:, comp] - goal
        e[:, 2] = e[:, 2] - two_pi * torch.round(e[:, 2] / two_pi)
        return e

    def cost(u):
        s, c = s0, (0.5 * (u @ Hc) * u).sum(1)
        for t in range(T):
            s = step(s, u[:, t], u[:, T + t])
            e = resid(s)
            c = c + 0.5 * ((qf if t == T - 1 else q) * e * e).sum(1)
        return c

    def linearize(u):
        s = s0
        S = torch.zeros((B, 5, N), dtype=torch.float32, device=s0.device)
        g = u @ Hc
        H = Hc.expand(B, N, N).clone()
        for t in range(T):
            D, V, psi = s[:, 2].clamp(-sm, sm), s[:, 3].clamp(-vm, vm), s[:, 4]
            md = ((s[:, 2] > -sm) & (s[:, 2] < sm)).float()
            mv = ((s[:, 3] > -vm) & (s[:, 3] < vm)).float()
            cp, sp, td = torch.cos(psi), torch.sin(psi), torch.tan(D)
            Fx = torch.eye(5, dtype=torch.float32, device=s0.device).expand(B, 5, 5).clone()
            Fx[:, 0, 3], Fx[:, 0, 4] = mv * dt * cp, -dt * V * sp
            Fx[:, 1, 3], Fx[:, 1, 4] = mv * dt * sp, dt * V * cp
            Fx[:, 4, 2], Fx[:, 4, 3] = md * (V / Lw) * (1.0 + td * td) * dt, mv * dt * (td / Lw)
            S = Fx @ S
            S[:, 3, t] = dt
            S[:, 2, T + t] = dt
            s = step(s, u[:, t], u[:, T + t])
            e = resid(s)
            w = qf if t == T - 1 else q
            rows = S[:, comp, :]
            g = g + torch.einsum("bk,bkn->bn", w * e, rows)
            H = H + torch.einsum("bkn,bkm->bnm", w[None, :, None] * rows, rows)
        return g, H

    u = torch.zeros((B, N), dtype=torch.float32, device=s0.device)
    lam = torch.full((B,), lambda0, dtype=torch.float32, device=s0.device)
    c = cost(u)
    done = c == 0
    iters = torch.zeros((B,), dtype=torch.int32, device=s0.device)
    eye = torch.eye(N, dtype=torch.float32, device=s0.device)
    for _ in range(max_iter):
        g, H = linearize(u)
        fixed = ((u <= -hi) & (g > 0)) | ((u >= hi) & (g < 0))
        diag = torch.diagonal(H, dim1=1, dim2=2)
        damp = diag + (lam[:, None] * diag + eps * diag.max(dim=1).values[:, None])
        free = (~fixed).float()
        A = H * free[:, :, None] * free[:, None, :] * (1.0 - eye) + torch.diag_embed(torch.where(fixed, torch.ones_like(damp), damp))
        L, _ = torch.linalg.cholesky_ex(A)
        d = torch.cholesky_solve((-g * free)[:, :, None], L)[:, :, 0]
        d = torch.where(torch.isfinite(d), d, torch.zeros_like(d))
        up = torch.minimum(torch.maximum(u + d, -hi), hi)
        cp = cost(up)
        act = ~done
        acc = act & (cp < c)
        conv = act & (((c - cp).abs() <= tol * c) | (acc & (cp == 0)))
        rej = act & ~acc & ~conv
        iters = iters + act.int()
        u = torch.where(acc[:, None], up, u)
        c = torch.where(acc, cp, c)
        lam = torch.where(acc, (lam / 10.0).clamp(min=lambda_min), torch.where(rej, (lam * 10.0).clamp(max=lambda_max), lam))
        done = done | conv | (rej & (lam >= lambda_max))
    return u, c, iters


def step_solve():
    import torch
    from irbfn_amd import _lib, nmpc
    import _nmpc_util as nu
    dp = nu.DP
    for logB in (16, 20):
        B = 1 << logB
        reps = 10 if logB == 16 else 3
        for select in (False, True):
            s0, goal, W = nu.family("reg", B, T, seed=123, select=select)
            sd, gd = torch.from_numpy(s0.astype(np.float32)).cuda(), torch.from_numpy(goal.astype(np.float32)).cuda()
            mode = _lib.ROLLOUT_ST_SELECT if select else _lib.ROLLOUT_ST_KS
            run = lambda: nmpc.solve(sd, gd, dp, T=T, weights=nmpc.Weights(**W), mode=mode, **nu.DEFAULTS)
            res = run()
            torch.cuda.synchronize()
            ms = [timed(torch, run, reps) for _ in range(5)]
            it = res.iterations.double()
            total = float(it.sum())
            counts = torch.bincount(res.status, minlength=4).tolist()
            med = sorted(ms)[2]
            print(f"solve    B = 2^{logB}, T = {T}, {'ST_SELECT' if select else 'ST_KS'}")
            print(f"  kernel {fmt(ms)}   iterations mean {float(it.mean()):.2f} max {int(it.max())}   "
                  f"{total / (med * 1e-3):.3e} rows x iterations / s   status counts {counts}")
            if not select:
                trun = lambda: torch_solve_ks(torch, sd, gd, dp, W, **nu.DEFAULTS)
                tu, tc, ti = trun()
                torch.cuda.synchronize()
                tms = [timed(torch, trun, 1) for _ in range(3 if logB == 16 else 1)]
                tmed = sorted(tms)[len(tms) // 2]
                rel = ((res.cost.double() - tc.double()) / tc.double())
                print(f"  torch  {tmed:9.3f} ms [{min(tms):.3f} .. {max(tms):.3f}]   iterations counted mean {float(ti.double().mean()):.2f} "
                      f"(run: {nu.DEFAULTS['max_iter']} for every row)   torch / kernel = {tmed / med:.1f}")
                print(f"  kernel cost against the torch statement's: (kernel - torch) / torch in [{float(rel.min()):.2e}, {float(rel.max()):.2e}]")
            print(flush=True)


def step_loop():
    import time

    import torch
    from irbfn_amd import _lib, configs, nmpc, simulate
    from closed_loop_timing import cars, ellipse
    wp = ellipse(1000)
    track = simulate.Track(wp, wrap=True, lookahead=1.5, max_reacquire=4.0, half_width=3.0)
    B, ticks = 1024, 1000
    st = torch.from_numpy(cars(wp, B)).cuda()
    for mode, name in ((_lib.ROLLOUT_ST_SELECT, "ST_SELECT"), (_lib.ROLLOUT_ST_KS, "ST_KS")):
        def run():
            t0 = time.perf_counter()
            res = nmpc.closed_loop(track, st, ticks, configs.DYN_PARAMS, T=T, mode=mode)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, res
        run()
        ts = []
        for _ in range(3):
            t, res = run()
            ts.append(t)
        med = sorted(ts)[1]
        s = res.summary()
        print(f"loop     B = {B}, N = 1000, {ticks} ticks, {name}, T = {T}")
        print(f"  {med * 1e3:9.1f} ms [{min(ts) * 1e3:.1f} .. {max(ts) * 1e3:.1f}]   {med / ticks * 1e6:8.1f} us per tick")
        print(f"  status {s['status']}; rms_dev quantiles (0, 0.5, 0.9, 1) {['%.3f' % v for v in s['rms_dev']]}; "
              f"laps {['%.2f' % v for v in s['laps']]}")
        print(flush=True)


def main():
    args = sys.argv[1:]
    if "--step" in args:
        {"solve": step_solve, "loop": step_loop}[args[args.index("--step") + 1]]()
        return 0
    out = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "nmpc.txt")
    text = PREAMBLE
    for name, limit in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name],
                           capture_output=True, text=True)
        text += r.stdout
        if r.returncode != 0:
            text += f"step {name} ended with status {r.returncode}\n{r.stderr[-2000:]}\n"
            open(out, "w").write(text)
            return 1
    open(out, "w").write(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
