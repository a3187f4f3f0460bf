"""The ST_SELECT adjoint on one lease -> profiles/st_select_vjp.txt.
  python tools/time_st_select_vjp.py [out.txt]                      timings (needs the GPU)
  python tools/time_st_select_vjp.py --resources-only [out.txt]     the kernel instances' registers and scratch (needs hipcc)

rollout_vjp_select next to the ST_KS VJP and the ST_SELECT forward at B = 262 144 (T = 5, 50) and B = 32 768 (T = 50), and
train_step_st_fullint next to train_step_fullint on the golden 1000-centre net at B = 80 000.  Device events around `reps`
back-to-back calls after a warm-up of every shape; the candidates of a shape alternate inside every round (A B C A B C ...), so
a drift of the machine hits them alike; median and spread of the rounds.  The register and scratch figures of the three kernel
instances are the metadata records of rollout_vjp.hip compiled to assembly with the build's flags (hipcc, no GPU needed)."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from irbfn_amd import _lib, configs, dynamics, train  # noqa: E402
from irbfn_amd.model import WCRBFNet  # noqa: E402
import _st_select_util as su  # noqa: E402  (tests/: the grid of the ST_SELECT tests)

DP = configs.DYN_PARAMS
ROUNDS, REPS = 7, 20
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def interleaved(cands):
    """cands: {name: fn} -> {name: (median us, min us, max us)} over ROUNDS rounds of REPS calls, the candidates alternating"""
    for fn in cands.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    got = {n: [] for n in cands}
    for _ in range(ROUNDS):
        for n, fn in cands.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                fn()
            e1.record()
            torch.cuda.synchronize()
            got[n].append(e0.elapsed_time(e1) / REPS * 1e3)
    return {n: (float(np.median(v)), min(v), max(v)) for n, v in got.items()}


def kernel_resources():
    """[(label, vgpr, sgpr, .vgpr_spill_count, .private_segment_fixed_size)] of the three ST_SELECT VJP instances: the metadata
    records of rollout_vjp.hip compiled to gfx950 assembly with the build's own flags"""
    from irbfn_amd import build
    src, _, extra = next(u for u in build.UNITS if u[0] == "rollout_vjp.hip")
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "rollout_vjp.s")
        r = subprocess.run(build.compile_cmd(src, extra, ["-S", "--cuda-device-only"], asm), capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(r.stderr[-2000:])
        text = open(asm).read()
    out = []
    for blk in re.findall(r"- \.agpr_count:.*?\.wavefront_size", text, re.S):
        g = lambda k: re.search(r"\.%s:\s*(\S+)" % k, blk).group(1)
        m = re.search(r"rollout_vjp_(regs|park)_kernelILi0E(?:Li(\d+)E)?", g("name"))
        if m:
            label = f"rollout_vjp_{m.group(1)}_kernel<ST_SELECT" + (f", {m.group(2)}>" if m.group(2) else ">")
            out.append((label,) + tuple(int(g(k)) for k in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "private_segment_fixed_size")))
    return out


def say_resources():
    say("kernel instance                                   vgpr  sgpr  .vgpr_spill_count  .private_segment_fixed_size")
    for label, vgpr, sgpr, spill, scratch in kernel_resources():
        say(f"{label:48s} {vgpr:5d} {sgpr:5d} {spill:18d} {scratch:28d}")


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    outp = args[0] if args else None
    if "--resources-only" in sys.argv:                                 # needs hipcc, no GPU
        say("# tools/time_st_select_vjp.py --resources-only")
        say_resources()
        if outp:
            open(outp, "w").write("\n".join(lines) + "\n")
        return
    _lib.require_gpu()
    rng = np.random.default_rng(0)
    say(f"# tools/time_st_select_vjp.py  ({ROUNDS} rounds x {REPS} calls per candidate, candidates interleaved; us = median [min .. max])")
    say()
    for B, T in ((262144, 5), (262144, 50), (32768, 50)):
        xu = torch.from_numpy(su.grid_rows(B, T, rng).astype(np.float32)).cuda()
        gs = torch.from_numpy(rng.normal(size=(B, T, 7)).astype(np.float32)).cuda()
        res = interleaved({
            "vjp ST_SELECT (rollout_vjp_select)": lambda: dynamics.rollout_vjp_select(xu, DP, gs, T),
            "vjp ST_KS     (rollout_vjp)": lambda: dynamics.rollout_vjp(_lib.ROLLOUT_ST_KS, xu, DP, gs, T),
            "forward ST_SELECT": lambda: dynamics.rollout_forward(_lib.ROLLOUT_ST_SELECT, xu, DP, T),
        })
        nb = {"v": 4 * B * (2 * (7 + 2 * T) + T * 7), "f": 4 * B * (7 + 2 * T + T * 7)}
        for n, (med, lo, hi) in res.items():
            by = nb["v" if n.startswith("vjp") else "f"]
            say(f"B={B:7d} T={T:3d}  {n:36s} {med:8.1f} us [{lo:8.1f} .. {hi:8.1f}]  {by / med / 1e6:5.2f} TB/s algorithmic")
        del xu, gs
    say()
    # the golden 1000-centre net (tests/golden), T = 5, at the reference's batch of 80 000
    from conftest import load_ckpt_fixture
    cfg, params, *_ = load_ckpt_fixture("dnmpc_1regions_newdata_oldintloss_nomirror_highk")
    B, T = 80000, cfg["out_features"] // 2
    x = rng.normal(size=(B, cfg["in_features"])).astype(np.float32) * 0.3
    x[:, 0] = 0.1 + 0.25 * (np.arange(B) % 27)
    y = su.grid_controls(B, T, rng).astype(np.float32)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    states = {n: train.TrainState.create(WCRBFNet.from_config(cfg), params, lr=1e-3) for n in ("select", "ks", "fullint")}
    res = interleaved({
        "train_step_st_fullint ST_SELECT": lambda: train.train_step_st_fullint(states["select"], xd, yd, DP),
        "train_step_st_fullint ST_KS": lambda: train.train_step_st_fullint(states["ks"], xd, yd, DP, mode=_lib.ROLLOUT_ST_KS),
        "train_step_fullint": lambda: train.train_step_fullint(states["fullint"], xd, yd),
    })
    say(f"# one training step, K = {cfg['num_kernels']} centres, D = {cfg['in_features']}, T = {T}, B = {B}")
    for n, (med, lo, hi) in res.items():
        say(f"{n:36s} {med:8.1f} us [{lo:8.1f} .. {hi:8.1f}]")
    if outp:
        open(outp, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
