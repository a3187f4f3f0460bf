"""Times the Frenet closed-loop tick (irbfn_sim_advance_frenet, K14; irbfn_amd/simulate.py) on one GPU against its two
yardsticks: the Cartesian tick it extends (irbfn_sim_advance) and the same Frenet tick composed from three launches
(irbfn_sim_advance -> irbfn_cartesian_to_frenet -> irbfn_plan_queries_frenet).

  advance : one call of each form at B in {1, 1024, 65536} on a line of N = 1000 way-points with the default window (8, 55).
  loop    : a 1000-tick closed_loop_frenet at B = 1024 with each golden Frenet net, fused and composed, and what the nets do
            (SimResult.summary()), next to nmpc.closed_loop on the same line and plant.
  regs    : registers and scratch of every instance of the kernel, from hipcc's resource remarks with build.py's flags
            (no GPU needed).

Without arguments every step runs as a child process under its own time limit, the first failure ends the run, and
profiles/closed_loop_frenet.txt (or the file after ``--out``) is written afresh.  ``--step NAME`` runs one step in this process."""
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS = 7
N_WAY = 1000
STEPS = (("regs", 240), ("advance", 300), ("loop", 420))       # (name, seconds)
GOLDEN = os.path.join(ROOT, "tests", "golden")
PREAMBLE = """\
Frenet closed loop (irbfn_amd/simulate.py, irbfn_sim_advance_frenet = csrc/sim_advance.hip, K14): times on one GPU, written by
tools/closed_loop_frenet_timing.py.  Every step is a process of its own under its own time limit.  The line: N = 1000 way-points
on the ellipse with semi-axes 12 m and 8 m (radius of curvature >= 5.3 m), closed (wrap), line speed 4 m/s; lookahead 1 m.
"advance" = one call with a plant step (ST_SELECT, n_sub = 1), default window (8, 55), timed as 2000 calls (500 at B = 65536)
between two device events (launch gaps included) divided by their number; median of 7 rounds interleaved over the forms after a
warm-up of each [min .. max]; every round starts from the same car states; the plant's dt is 1e-4 s, so that the cars stay where
they are and every car does the whole tick in every call (the count of cars still driving at the end is printed).
  frenet fused    : irbfn_sim_advance_frenet (pose stored too)
  cartesian fused : irbfn_sim_advance, the yardstick for what the frame change adds
  frenet composed : irbfn_sim_advance, irbfn_cartesian_to_frenet (window around the segments the tick started from),
                    irbfn_plan_queries_frenet into preallocated arrays, plus the two device copies the form cannot do without
                    (the segments before the tick, the goal's speed column); frozen cars are not masked (none freezes)
"loop" = simulate.closed_loop_frenet for 1000 ticks at B = 1024 (plan_tick + irbfn_sim_advance_frenet per tick), one host clock
around the call and a device synchronise, against the composed loop with the same plan_tick; median of 5 alternating rounds.
The summary lines are SimResult.summary(): a report of what the nets do on this line, no claim.
Not measured: kernel time apart from launch gaps (no profiler run), PMC counters, the clocks under load.

"""


def ellipse(n, a=12.0, b=8.0, v=4.0):
    th = np.linspace(0, 2 * np.pi, n, endpoint=False)
    xy = np.stack([a * np.cos(th), b * np.sin(th)], axis=1)
    nxt = np.roll(xy, -1, axis=0) - xy
    return np.concatenate([xy, np.arctan2(nxt[:, 1], nxt[:, 0])[:, None], np.full((n, 1), v)], axis=1)


def cars(track, B, seed=0):
    """single-track states on the line: |ey| <= 0.15 m, |epsi| <= 0.1 rad, 3 .. 4.5 m/s"""
    rng = np.random.default_rng(seed + B)
    x, y, psi = track.pose_at(rng.uniform(0.0, track.cum[-1], B), rng.uniform(-0.15, 0.15, B), rng.uniform(-0.1, 0.1, B))
    st = np.zeros((B, 7), np.float32)
    st[:, 0], st[:, 1], st[:, 4], st[:, 3] = x, y, psi, rng.uniform(3.0, 4.5, B)
    return st


class Arrays:
    """the per-car arrays of simulate.closed_loop_frenet"""

    def __init__(self, torch, simulate, track, st, width):
        B = st.shape[0]
        self.state = st.clone()
        self.seg = track.seed(st[:, :2].double()).contiguous()
        self.status = torch.zeros(B, dtype=torch.int32, device="cuda")
        self.rec = simulate.new_record(B, torch)
        self.x = torch.zeros((B, width), dtype=torch.float32, device="cuda")
        self.m = torch.zeros(B, dtype=torch.int32, device="cuda")
        self.goal = torch.zeros((B, 4), dtype=torch.float64, device="cuda")
        self.old = self.seg.clone()
        self.fr = torch.zeros((B, 8), dtype=torch.float64, device="cuda")
        self.vg = torch.zeros(B, dtype=torch.float64, device="cuda")
        self.qx = torch.zeros((B, 8), dtype=torch.float32, device="cuda")
        self.qm = torch.zeros(B, dtype=torch.int32, device="cuda")


def composed_tick(torch, simulate, track, a, **kw):
    """the Frenet tick in three launches and two device copies on the arrays `a` of a Cartesian tick, nothing allocated:
    -> (x8, m8) of this tick, in a's buffers"""
    import ctypes as C

    from irbfn_amd import _lib
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    a.old.copy_(a.seg)
    simulate.advance(track, a.state, a.seg, a.status, a.rec, a.x, a.m, goal_out=a.goal, **kw)
    tr = track.struct(torch)
    _lib.check(lib.irbfn_cartesian_to_frenet(C.byref(tr), track.curvature_device(torch).data_ptr(), a.state.data_ptr(),
                                             a.old.data_ptr(), a.fr.data_ptr(), None, None, None, a.state.shape[0], stream),
               "irbfn_cartesian_to_frenet")
    a.vg.copy_(a.goal[:, 3])
    _lib.check(lib.irbfn_plan_queries_frenet(a.fr.data_ptr(), a.vg.data_ptr(), a.qx.data_ptr(), None, a.qm.data_ptr(),
                                             a.state.shape[0], stream), "irbfn_plan_queries_frenet")
    return a.qx, a.qm


def timed(torch, fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps                      # microseconds per call


def fmt(v):
    v = sorted(v)
    return f"{v[len(v) // 2]:9.1f} us [{v[0]:.1f} .. {v[-1]:.1f}]"


def step_advance():
    import torch
    from irbfn_amd import configs, simulate
    track = simulate.Track(ellipse(N_WAY), wrap=True, lookahead=1.0, max_reacquire=4.0)
    p = list(configs.DYN_PARAMS)
    p[8] = 1e-4                                                # dt: the cars stay where they are through the timed calls
    for B in (1, 1024, 65536):
        reps = 500 if B > 1024 else 2000
        st = torch.from_numpy(cars(track, B)).cuda()
        ctrl = torch.zeros((B, 2), dtype=torch.float32, device="cuda")
        ctrl[:, 0] = 0.2
        fr_out = torch.zeros((B, 8), dtype=torch.float64, device="cuda")

        def run_frenet():
            a = Arrays(torch, simulate, track, st, 8)
            simulate.advance_frenet(track, a.state, a.seg, a.status, a.rec, a.x, a.m, frenet_out=fr_out)
            us = timed(torch, lambda: simulate.advance_frenet(track, a.state, a.seg, a.status, a.rec, a.x, a.m, controls=ctrl,
                                                              plant_params=p, tick=1, frenet_out=fr_out), reps)
            return us, int((a.status == 0).sum())

        def run_cartesian():
            a = Arrays(torch, simulate, track, st, 7)
            simulate.advance(track, a.state, a.seg, a.status, a.rec, a.x, a.m)
            us = timed(torch, lambda: simulate.advance(track, a.state, a.seg, a.status, a.rec, a.x, a.m, controls=ctrl,
                                                       plant_params=p, tick=1), reps)
            return us, int((a.status == 0).sum())

        def run_composed():
            a = Arrays(torch, simulate, track, st, 7)
            composed_tick(torch, simulate, track, a)
            us = timed(torch, lambda: composed_tick(torch, simulate, track, a, controls=ctrl, plant_params=p, tick=1), reps)
            return us, int((a.status == 0).sum())
        variants = {"frenet fused": run_frenet, "cartesian fused": run_cartesian, "frenet composed": run_composed}
        times, alive = {n: [] for n in variants}, {}
        for n, f in variants.items():                          # warm-up
            f()
        for _ in range(ROUNDS):
            for n, f in variants.items():
                us, alive[n] = f()
                times[n].append(us)
        med = {n: sorted(v)[len(v) // 2] for n, v in times.items()}
        print(f"advance  B = {B}, N = {N_WAY}, window (8,55): one tick without the net")
        for n in variants:
            print(f"  {n:18s} {fmt(times[n])}   cars still driving: {alive[n]}")
        print(f"  frenet fused / cartesian fused = {med['frenet fused'] / med['cartesian fused']:.2f}, "
              f"frenet fused / frenet composed = {med['frenet fused'] / med['frenet composed']:.2f}"
              + ("   <-- the fused call is SLOWER than the composed form" if med["frenet fused"] > med["frenet composed"] else ""))
        print(flush=True)


def golden_net(kind):
    from irbfn_amd.model import DeeperWCRBFNet, WCRBFNet
    if kind == "12 regions (T = 1)":
        run = "dnmpc_12regions_frenet_l1_bigdata"
        z = np.load(os.path.join(GOLDEN, f"ckpt_{run}.npz"))
        params = {"params": {"rbf_list": {"centers": z["centers"], "log_sigs": z["log_sigs"]},
                             "linear": {"kernel": z["kernel"], "bias": z["bias"]}}}
        return WCRBFNet.from_config(json.load(open(os.path.join(GOLDEN, f"ckpt_{run}.json")))), params
    run = "dnmpc_1regions_frenet_l1_bigdata_5stepint_deeper"
    z = np.load(os.path.join(GOLDEN, f"ckpt_{run}.npz"))
    params = {"params": {k: {n: z[f"{k}__{n}"] for n in names} for k, names in (
        ("rbf_list", ("centers", "log_sigs")), ("linear_pre1", ("kernel", "bias")), ("linear_pre2", ("kernel", "bias")),
        ("linear", ("kernel", "bias")))}}
    return DeeperWCRBFNet.from_config(json.load(open(os.path.join(GOLDEN, f"ckpt_{run}.json")))), params


def brief(s):
    med = lambda v: f"{v[1]:.4g}" if v else "-"
    return f"status {s['status']}, median rms_dev {med(s['rms_dev'])} m, median laps {med(s['laps'])}"


def step_loop():
    import time

    import torch
    from irbfn_amd import _lib, configs, nmpc, planner, simulate
    track = simulate.Track(ellipse(N_WAY), wrap=True, lookahead=1.0, max_reacquire=4.0, half_width=3.0)
    p, ticks, mode, B = configs.DYN_PARAMS, 1000, _lib.ROLLOUT_ST_SELECT, 1024
    st = torch.from_numpy(cars(track, B)).cuda()
    q = (0.0, 0.5, 0.9, 1.0)
    for kind in ("12 regions (T = 1)", "deeper (T = 5)"):
        net, params = golden_net(kind)

        def fused():
            t0 = time.perf_counter()
            res = simulate.closed_loop_frenet(net, params, track, st, ticks, dyn_params=p)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, res

        def composed():
            t0 = time.perf_counter()
            a = Arrays(torch, simulate, track, st, 7)
            qx, qm = composed_tick(torch, simulate, track, a, mode=mode, tick=0)
            x8, m8 = qx.clone(), qm.clone()
            for k in range(ticks):
                ctrl, _ = planner.plan_tick(net, params, x8, m8, rollout=False, mode=mode)
                qx, qm = composed_tick(torch, simulate, track, a, controls=ctrl, plant_params=p, mode=mode, tick=k + 1)
                live = a.status == 0                           # a stopped car keeps its last query
                x8, m8 = torch.where(live[:, None], qx, x8), torch.where(live, qm, m8)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, a
        fused(), composed()
        tf, tc = [], []
        for _ in range(5):
            f = fused()
            c = composed()
            tf.append(f[0])
            tc.append(c[0])
        same = bool(torch.equal(f[1].state.view(torch.int32), c[1].state.view(torch.int32))) and bool(torch.equal(f[1].status, c[1].status))
        med = lambda v: sorted(v)[len(v) // 2]
        print(f"loop     B = {B}, N = {N_WAY}, {ticks} ticks, golden Frenet net {kind}")
        print(f"  fused    {med(tf) * 1e3:9.1f} ms [{min(tf) * 1e3:.1f} .. {max(tf) * 1e3:.1f}]   {med(tf) / ticks * 1e6:8.1f} us per tick")
        print(f"  composed {med(tc) * 1e3:9.1f} ms [{min(tc) * 1e3:.1f} .. {max(tc) * 1e3:.1f}]   {med(tc) / ticks * 1e6:8.1f} us per tick")
        print(f"  final states and statuses bit-equal: {same}")
        print(f"  what the net does: {brief(f[1].summary(q))}")
        print(flush=True)
    t0 = time.perf_counter()
    res = nmpc.closed_loop(track, st, ticks, dyn_params=p)
    torch.cuda.synchronize()
    print(f"nmpc.closed_loop on the same line, cars and plant (defaults), {ticks} ticks: {(time.perf_counter() - t0) * 1e3:.1f} ms")
    print(f"  what the MPC baseline does: {brief(res.summary(q))}")
    print(flush=True)


def step_regs():
    from irbfn_amd import build
    unit = next(u for u in build.UNITS if u[0] == "sim_advance.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = build.compile_cmd(unit[0], unit[2] + ["-Rpass-analysis=kernel-resource-usage"], ["-c"], os.path.join(tmp, "sim.o"))
        r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        print(r.stderr[-2000:])
        sys.exit(1)
    form = {"0": "cartesian tick (irbfn_sim_advance)", "1": "frenet tick (irbfn_sim_advance_frenet)", "2": "pose only (irbfn_cartesian_to_frenet)"}
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: _ZN5irbfn18sim_advance_kernelILi(\d+)ELb([01])ELi(\d)EEE", line)
        if m:
            cur = dict(name=f"sim_advance_kernel<{m.group(1)}, {'ST_SELECT' if m.group(2) == '1' else 'ST_KS'}, {m.group(3)}>  {form[m.group(3)]}")
            rows.append(cur)
            continue
        for key, pat in (("sgpr", r"TotalSGPRs: (\d+)"), ("vgpr", r" VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = m.group(1)
    print("registers of csrc/sim_advance.hip (hipcc -Rpass-analysis=kernel-resource-usage, build.py's flags, gfx950)")
    for c in rows:
        print(f"  {c['name']:86s} VGPRs {c['vgpr']:>3s}  SGPRs {c['sgpr']:>3s}  scratch {c['scratch']} B/lane  LDS {c.get('lds', '0')} B  "
              f"occupancy {c['occ']} waves/SIMD")
    print(flush=True)


def main():
    args = sys.argv[1:]
    if "--step" in args:
        {"advance": step_advance, "loop": step_loop, "regs": step_regs}[args[args.index("--step") + 1]]()
        return 0
    out = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "closed_loop_frenet.txt")
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
