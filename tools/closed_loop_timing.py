"""Times the closed-loop tick (irbfn_sim_advance, irbfn_amd/simulate.py) on one GPU, next to the same work composed from the
older entry points: nearest_point -> intersect_point -> gather -> build_queries (-> plan_tick -> rollout_forward), with the
status rule in torch ops and nothing read by the host.

  advance : one irbfn_sim_advance call (plant step + search + goal + statistics + query) at B in {1, 1024, 65536} on a line of
            N = 1000 way-points, for the default window (8, 55) and the whole line; next to it the composed tick without the
            net.  (Other lane layouts of the kernel: tools/ab_sim_lanes.hip.)
  loop    : a whole 1000-tick closed_loop on the golden 1000-centre net at B = 1024 and 65536, fused and composed.

Without arguments every step runs as a child process under its own time limit, the first failure ends the run, and
profiles/closed_loop.txt (or the file after ``--out``) is written afresh.  ``--step NAME`` runs one step in this process."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS = 7
N_WAY = 1000
STEPS = (("advance", 300), ("loop", 540))                      # (name, seconds)
GOLDEN = "dnmpc_1regions_newdata_oldintloss_nomirror_highk"
PREAMBLE = """\
Closed-loop simulation (irbfn_amd/simulate.py, irbfn_sim_advance = csrc/sim_advance.hip): times on one GPU, written by
tools/closed_loop_timing.py.  Every step is a process of its own under its own time limit.  The line: N = 1000 way-points on an
ellipse, about 0.5 m apart, closed (wrap); cars within 0.3 m of it at 1 .. 5 m/s; lookahead 1.5 m.
"advance" = one irbfn_sim_advance call with a plant step (ST_SELECT, n_sub = 1), timed as 2000 calls (500 at B = 65536) between two
device events (launch gaps included) divided by their number, median of 7 rounds interleaved over all variants after a warm-up of
each [min .. max]; every round starts from the same car states; the plant's dt is 1e-4 s, so that the cars stay where they are and
every car does the whole tick in every call (the count of cars still driving at the end is printed).
"composed" = the same tick from the older entry points on the same GPU: rollout_forward
(T = 1), nearest_point, intersect_point, gather, build_queries and the status rule in torch ops, nothing read by the host.
"loop" = simulate.closed_loop for 1000 ticks on the golden 1000-centre net (plan_tick + irbfn_sim_advance per tick), one host
clock around the call and a device synchronise, against the composed loop with the same plan_tick; median of 3 alternating rounds.
The states of the fused and of the composed loop are compared bit for bit after the timed runs.
Not measured: kernel time apart from launch gaps (no profiler run), PMC counters, the clocks under load.

"""


def ellipse(n):
    th = np.linspace(0, 2 * np.pi, n, endpoint=False)
    r = 0.08 * n
    xy = np.stack([r * np.cos(th), 0.6 * r * np.sin(th)], axis=1)
    nxt = np.roll(xy, -1, axis=0) - xy
    return np.concatenate([xy, np.arctan2(nxt[:, 1], nxt[:, 0])[:, None], (2.5 + np.cos(2 * th))[:, None]], axis=1)


def cars(wp, B, seed=0):
    rng = np.random.default_rng(seed + B)
    j = rng.integers(0, wp.shape[0] - 1, B)
    st = np.zeros((B, 7), np.float32)
    st[:, :2] = wp[j, :2] + rng.normal(size=(B, 2)) * 0.15
    st[:, 3] = rng.uniform(1, 5, B)
    st[:, 4] = wp[j, 2] + rng.uniform(-0.2, 0.2, B)
    return st


class Composed:
    """the tick from the older entry points; the arrays of simulate.closed_loop, updated by torch ops"""

    def __init__(self, torch, track, state):
        self.torch, self.track = torch, track
        self.wp, self.xy = track.device(torch)[:2]
        B = state.shape[0]
        self.state = state.clone()
        self.status = torch.zeros(B, dtype=torch.int32, device="cuda")
        self.fail = torch.full((B,), -1, dtype=torch.int64, device="cuda")
        self.x = torch.zeros((B, 7), dtype=torch.float32, device="cuda")
        self.mirror = torch.zeros(B, dtype=torch.int32, device="cuda")

    def tick(self, ctrl, p, mode, k):
        from irbfn_amd import dynamics, planner, planner_utils
        torch, tr = self.torch, self.track
        live = self.status == 0
        if ctrl is not None:
            T = ctrl.shape[1] // 2
            new = dynamics.rollout_forward(mode, torch.cat([self.state, ctrl[:, :1], ctrl[:, T:T + 1]], dim=1), p, 1)[:, -1, :]
            self.state = torch.where(live[:, None], new, self.state)
            bad = live & ~torch.isfinite(new).all(dim=1)
            self.status[bad], self.fail[bad] = 1, k
            live = live & ~bad
        pts = self.state[:, :2].double()
        _, d, t, i = planner_utils.nearest_point(pts, self.xy)
        _, fi, _, found = planner_utils.intersect_point(pts, tr.lookahead, self.xy, i.double() + t, tr.wrap)
        off = live & (d > tr.half_width) if tr.half_width > 0 else torch.zeros_like(live)
        near = d < tr.lookahead
        lost = live & ~off & ((near & (found == 0)) | (~near & ~(d < tr.max_reacquire)))
        self.status[off], self.status[lost] = 2, 3
        self.fail[off | lost] = k
        live = live & ~off & ~lost
        gidx = torch.where(near & (found != 0), (fi.long() + tr.N) % tr.N, i.long())
        qx, _, qm = planner.build_queries(self.state.double(), self.wp[gidx])
        self.x = torch.where(live[:, None], qx, self.x)
        self.mirror = torch.where(live, qm, self.mirror)


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
    from irbfn_amd import _lib, configs, simulate
    wp = ellipse(N_WAY)
    p = list(configs.DYN_PARAMS)
    p[8] = 1e-4                                                # dt: the cars stay where they are through the timed calls
    for B in (1, 1024, 65536):
        reps = 500 if B > 1024 else 2000
        st = torch.from_numpy(cars(wp, B)).cuda()
        ctrl = torch.zeros((B, 10), dtype=torch.float32, device="cuda")
        ctrl[:, 0] = 0.2
        variants = {}
        for wname, window in (("window (8,55)", (8, 55)), ("whole line", None)):
            track = simulate.Track(wp, wrap=True, lookahead=1.5, max_reacquire=4.0, window=window)
            seg0 = track.seed(st[:, :2].double()).contiguous()

            def run(track=track, seg0=seg0):
                state, seg = st.clone(), seg0.clone()
                status = torch.zeros(B, dtype=torch.int32, device="cuda")
                rec = simulate.new_record(B, torch)
                x = torch.zeros((B, 7), dtype=torch.float32, device="cuda")
                m = torch.zeros(B, dtype=torch.int32, device="cuda")
                simulate.advance(track, state, seg, status, rec, x, m)
                us = timed(torch, lambda: simulate.advance(track, state, seg, status, rec, x, m, controls=ctrl, plant_params=p,
                                                           tick=1), reps)
                return us, int((status == 0).sum())
            variants[f"fused, {wname}"] = run
        track = simulate.Track(wp, wrap=True, lookahead=1.5, max_reacquire=4.0)

        def run_composed():
            c = Composed(torch, track, st)
            c.tick(None, p, _lib.ROLLOUT_ST_SELECT, 0)
            return timed(torch, lambda: c.tick(ctrl, p, _lib.ROLLOUT_ST_SELECT, 1), reps), int((c.status == 0).sum())
        variants["composed (whole line)"] = run_composed
        times, alive = {n: [] for n in variants}, {}
        for n, f in variants.items():                          # warm-up
            f()
        for _ in range(ROUNDS):
            for n, f in variants.items():
                us, alive[n] = f()
                times[n].append(us)
        print(f"advance  B = {B}, N = {N_WAY}: one tick without the net")
        for n in variants:
            print(f"  {n:24s} {fmt(times[n])}   cars still driving: {alive[n]}")
        print(flush=True)


def step_loop():
    import time

    import torch
    from irbfn_amd import _lib, configs, planner, simulate
    from irbfn_amd.model import WCRBFNet
    z = np.load(os.path.join(ROOT, "tests", "golden", f"ckpt_{GOLDEN}.npz"))
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", f"ckpt_{GOLDEN}.json")))
    params = {"params": {"rbf_list": {"centers": z["centers"], "log_sigs": z["log_sigs"]},
                         "linear": {"kernel": z["kernel"], "bias": z["bias"]}}}
    net = WCRBFNet.from_config(cfg)
    wp = ellipse(N_WAY)
    p, ticks, mode = configs.DYN_PARAMS, 1000, _lib.ROLLOUT_ST_SELECT
    track = simulate.Track(wp, wrap=True, lookahead=1.5, max_reacquire=4.0, half_width=3.0)
    for B in (1024, 65536):
        st = torch.from_numpy(cars(wp, B)).cuda()

        def fused():
            t0 = time.perf_counter()
            res = simulate.closed_loop(net, params, track, st, ticks, dyn_params=p)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, res.state, res.status

        def composed():
            t0 = time.perf_counter()
            c = Composed(torch, track, st)
            c.tick(None, p, mode, 0)
            for k in range(ticks):
                ctrl, _ = planner.plan_tick(net, params, c.x, c.mirror, rollout=False, mode=mode)
                c.tick(ctrl, p, mode, k + 1)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, c.state, c.status
        fused(), composed()
        tf, tc = [], []
        for _ in range(3):
            a = fused()
            b = composed()
            tf.append(a[0])
            tc.append(b[0])
        same = bool(torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))) and bool(torch.equal(a[2], b[2]))
        med = lambda v: sorted(v)[1]
        print(f"loop     B = {B}, N = {N_WAY}, {ticks} ticks, golden net K = 1000")
        print(f"  fused    {med(tf) * 1e3:9.1f} ms [{min(tf) * 1e3:.1f} .. {max(tf) * 1e3:.1f}]   {med(tf) / ticks * 1e6:8.1f} us per tick")
        print(f"  composed {med(tc) * 1e3:9.1f} ms [{min(tc) * 1e3:.1f} .. {max(tc) * 1e3:.1f}]   {med(tc) / ticks * 1e6:8.1f} us per tick")
        print(f"  final states and statuses bit-equal: {same}; cars still driving: {int((a[2] == 0).sum())} of {B}")
        print(flush=True)


def main():
    args = sys.argv[1:]
    if "--step" in args:
        {"advance": step_advance, "loop": step_loop}[args[args.index("--step") + 1]]()
        return 0
    out = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "closed_loop.txt")
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
