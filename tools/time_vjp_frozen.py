"""Full K2g against K2g's frozen-leaf instances (irbfn_net_vjp_frozen) on the same net and batch: the fixed-centre net
(no_centres) and the fixed-width net (linear), interleaved A/B, median over rounds of the mean of `reps` VJPs each.
    python tools/time_vjp_frozen.py [--rounds 7] [--reps 20]
Sizes: 1 region x 500 centres, d = 8, O = 10, B = 80000 (the reference's fixed-centre checkpoint at its batch size);
1000 centres, same otherwise (its fixed-width checkpoint); config 3 (d = 7, 4096 centres, O = 10, B = 65536).

    python tools/time_vjp_frozen.py --libs <parent's libirbfn_hip.so> <the same again> <this tree's> [--rounds 7] [--reps 20]
compares builds of the library on what follows the main VJP kernels and on the multi-step loss seeds: one process per build
(IRBFN_LIB), all alive and asked in turn, case by case -- the 1000-centre net (all leaves, both frozen modes), config 3, the
128-region net under K2r, and the Frenet and single-track seed kernels at B = 80000 with T = 5 and 16.  Two columns of the same
build give the spread a difference has to beat.  (The cluster net through irbfn_net_vjp_gamma: tools/time_cluster_vjp_gram.py
--vjp-only under each build.)"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from irbfn_amd import _lib, configs, distributed  # noqa: E402
from irbfn_amd.model import WCRBFNet  # noqa: E402


def t_us(fn, reps):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def case_ref(K, B, D=8, O=10, seed=0):
    rng = np.random.default_rng(seed)
    card = {"in_features": D, "out_features": O, "num_kernels": K, "basis_func": "gaussian", "num_regions": 1,
            "lower_bounds": [[-1.0]] * D, "upper_bounds": [[2.0]] * D, "dimension_ranges": [[0] * D],
            "activation_idx": list(range(D)), "delta": [20.0] * D}
    P = {"params": {"rbf_list": {"centers": rng.uniform(-1.4, 2.4, size=(1, K, D)).astype(np.float32),
                                 "log_sigs": rng.uniform(-0.2, 0.9, size=(1, K)).astype(np.float32)},
                    "linear": {"kernel": rng.normal(size=(K, O)).astype(np.float32), "bias": rng.normal(size=(O,)).astype(np.float32)}}}
    x = rng.uniform(-1.0, 2.0, size=(B, D)).astype(np.float32)
    g = (rng.normal(size=(B, O)) * 1e-2).astype(np.float32)
    return card, P, x, g


def case_cfg3():
    return configs.model_card(3), configs.synth_params(3), configs.synth_queries(3), configs.synth_cotangent(3)


def frozen_runs(card, P):
    """{full, no_centres, linear}: (net, device parameters) of the plain, the fixed-centre and the fixed-width net, K2g forced"""
    c = P["params"]["rbf_list"]["centers"]
    fc = WCRBFNet(**card, centers=c, fixed_centers=True)
    fw = WCRBFNet(**card, centers=c, fixed_width=True, log_sigs=P["params"]["rbf_list"]["log_sigs"])
    runs = {"full": (WCRBFNet(**card), distributed.params_to_device(P)),
            "no_centres": (fc, distributed.params_to_device({"params": {"rbf_list": {"log_sigs": P["params"]["rbf_list"]["log_sigs"]},
                                                                       "linear": P["params"]["linear"]}})),
            "linear": (fw, distributed.params_to_device({"params": {"linear": P["params"]["linear"]}}))}
    for net, p in runs.values():
        net.set_options(vjp_kernel=_lib.VJP_K2G, gram_sticky=1)
        net.bind(p)
    return runs


# ---- --libs: the same calls on several builds of the library (IRBFN_LIB), e.g. the parent's twice and this tree's --------------
def lib_cases():
    """({name: call} of the slab-reduce and loss-seed paths at the sizes users run, what the seed calls point into)"""
    import ctypes as C
    import json
    from irbfn_amd.model import _ptr, _stream_ptr
    cases = {}

    def vjp_case(name, net, p, x, g):
        xt, gt = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()
        cases[name] = lambda: net.vjp(p, xt, gt)

    card, P, x, g = case_ref(1000, 80000)
    for k, (net, p) in frozen_runs(card, P).items():
        vjp_case(f"1x1000 B=80000 K2g {k}", net, p, x, g)
    card, P, x, g = case_cfg3()
    vjp_case("config 3 B=65536 auto", WCRBFNet(**card), distributed.params_to_device(P), x, g)
    gdir = os.path.join(ROOT, "tests", "golden")
    z, cfg = np.load(os.path.join(gdir, "ckpt_dnmpc_128regions.npz")), json.load(open(os.path.join(gdir, "ckpt_dnmpc_128regions.json")))
    P = {"params": {"rbf_list": {"centers": z["centers"].astype(np.float32), "log_sigs": z["log_sigs"].astype(np.float32)},
                    "linear": {"kernel": z["kernel"].astype(np.float32), "bias": z["bias"].astype(np.float32)}}}
    rng = np.random.default_rng(17)
    ns, D, B = len(cfg["activation_idx"]), cfg["in_features"], 80000
    lo = np.array([min(cfg["lower_bounds"][d]) for d in range(ns)])
    hi = np.array([max(cfg["upper_bounds"][d]) for d in range(ns)])
    x = np.hstack([rng.uniform(lo, hi, size=(B, ns)), rng.normal(size=(B, D - ns)) * 0.1]).astype(np.float32)
    vjp_case("128 regions B=80000 K2r", WCRBFNet.from_config(cfg).set_options(vjp_kernel=_lib.VJP_K2R), distributed.params_to_device(P), x,
             rng.normal(size=(B, cfg["out_features"])).astype(np.float32))
    # the multi-step loss seeds
    lib = _lib.load()
    host = np.array(configs.DYN_PARAMS, np.float32)
    keep = []
    for T in (5, 16):
        u = np.hstack([rng.normal(size=(B, T)) * 2, rng.normal(size=(B, T)) * 0.5]).astype(np.float32)
        yp, y = torch.from_numpy(u).cuda(), torch.from_numpy(u + rng.normal(size=u.shape).astype(np.float32) * 0.1).cuda()
        xf = rng.normal(size=(B, 8)).astype(np.float32) * 0.1
        xf[:, 2] = rng.uniform(1.0, 6.0, size=B)
        xs = rng.normal(size=(B, 7)).astype(np.float32) * 0.1
        xs[:, 0] = rng.uniform(0.5, 7.0, size=B)
        xf, xs = torch.from_numpy(xf).cuda(), torch.from_numpy(xs).cuda()
        gy, loss, part = torch.empty_like(yp), torch.empty(1, device="cuda"), torch.empty(lib.irbfn_train_loss_partials(), device="cuda")
        keep.append((yp, y, xf, xs, gy, loss, part))
        tail = (host.ctypes.data_as(C.c_void_p), 0.5, _ptr(gy), _ptr(loss), _ptr(part), B)
        cases[f"seeds frenet T={T} B=80000"] = (lambda xf=xf, yp=yp, y=y, tail=tail, T=T: _lib.check(lib.irbfn_train_seeds_frenet_fullint(
            _ptr(xf), _ptr(yp), _ptr(y), *tail, 8, T, _stream_ptr(torch)), "seeds"))
        for mname, mode in (("select", _lib.ROLLOUT_ST_SELECT), ("ks", _lib.ROLLOUT_ST_KS)):
            cases[f"seeds st {mname} T={T} B=80000"] = (lambda xs=xs, yp=yp, y=y, tail=tail, T=T, mode=mode: _lib.check(
                lib.irbfn_train_seeds_st_fullint(mode, _ptr(xs), _ptr(yp), _ptr(y), *tail, 7, T, _stream_ptr(torch)), "seeds"))
    return cases, (keep, host)


def lib_child(reps):
    """answers each case name on stdin with the mean time of `reps` calls (us)"""
    cases, _alive = lib_cases()
    print("READY " + "\t".join(cases), flush=True)
    for line in sys.stdin:
        print(f"{t_us(cases[line.rstrip(chr(10))], reps):.3f}", flush=True)


def lib_main(libs, rounds, reps):
    """One child process per library, all alive at once and asked in turn: rounds interleave at the level of one case."""
    import subprocess
    kids = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(reps)], stdin=subprocess.PIPE,
                             stdout=subprocess.PIPE, text=True, env=dict(os.environ, IRBFN_LIB=os.path.abspath(lib))) for lib in libs]
    names = None
    for k in kids:
        line = k.stdout.readline()
        while line and not line.startswith("READY "):
            line = k.stdout.readline()
        assert line, "a child ended before it was ready"
        names = line[6:].rstrip("\n").split("\t")
    print(f"# {rounds} interleaved rounds of the mean of {reps} calls, median [min .. max] in us; columns: " + ", ".join(libs))
    for name in names:
        t = [[] for _ in kids]
        for _ in range(rounds):
            for i, k in enumerate(kids):
                k.stdin.write(name + "\n"); k.stdin.flush()
                t[i].append(float(k.stdout.readline()))
        print(f"{name:42s} " + "   ".join(f"{np.median(v):8.1f} [{min(v):8.1f} .. {max(v):8.1f}]" for v in t), flush=True)
    for k in kids:
        k.stdin.close()
        k.wait()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--libs", nargs="+", help="builds of libirbfn_hip.so to compare on the reduce and seed paths (one process each)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return lib_child(a.reps)
    if a.libs:
        return lib_main(a.libs, a.rounds, a.reps)
    print(f"# {torch.cuda.get_device_name(0)}; median over {a.rounds} interleaved rounds of the mean of {a.reps} VJPs (us)")
    cases = (("1x500, d=8, O=10, B=80000", lambda: case_ref(500, 80000)),
             ("1x1000, d=8, O=10, B=80000", lambda: case_ref(1000, 80000)),
             ("config 3 (4096, d=7, O=10, B=65536)", case_cfg3))
    for title, mk in cases:
        card, P, x, g = mk()
        xt, gt = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()
        runs = frozen_runs(card, P)
        names = {}
        for k, (net, p) in runs.items():
            net.vjp(p, xt, gt)
            names[k] = net.last_launch()["kernel"]
        t = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, (net, p) in runs.items():
                t[k].append(t_us(lambda: net.vjp(p, xt, gt), a.reps))
        med = {k: float(np.median(v)) for k, v in t.items()}
        print(f"\n## {title}")
        for k in runs:
            spread = f"{min(t[k]):.1f}-{max(t[k]):.1f}"
            ratio = med[k] / med["full"]
            print(f"{k:11s} {med[k]:7.1f} us  (rounds {spread})  ratio to full {ratio:.3f}  [{names[k]}]", flush=True)


if __name__ == "__main__":
    main()
