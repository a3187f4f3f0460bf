"""Reference-scale timings (batch 80000, the reference's YAML default) of the model variants and training steps that the
BASELINE configs do not exercise: multi-region Frenet net, DeeperWCRBFNet VJP, ClusterWCRBFNet forward / VJP / training
step (R = 11, and the reference's R = 500 with K = 10 and 50).  Looks for cliffs (a path that is fine at test sizes and
serial at scale).  --cluster-only: the cluster rows alone.  GPU box."""
import os, sys
import numpy as np, torch
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
from conftest import load_ckpt_fixture, load_deeper_fixture
from irbfn_amd import configs, train
from irbfn_amd.model import WCRBFNet, DeeperWCRBFNet, ClusterWCRBFNet
DP = np.array(configs.DYN_PARAMS)
def timed(fn, n=10):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3
B = 80000
rng = np.random.default_rng(0)
CLUSTER_ONLY = "--cluster-only" in sys.argv
def other_rows():
    # 12-region Frenet net (D = 8, O = 2)
    cfg, P, x, *_ = load_ckpt_fixture("dnmpc_12regions_frenet_l1_bigdata")
    P = {"params": {g: {n: np.asarray(v, np.float32) for n, v in d.items()} for g, d in P["params"].items()}}
    ns = len(cfg["activation_idx"])
    lo = np.array([min(cfg["lower_bounds"][d]) for d in range(ns)]); hi = np.array([max(cfg["upper_bounds"][d]) for d in range(ns)])
    xq = rng.uniform(lo, hi, size=(B, 8)).astype(np.float32); xq[:, 7] = rng.normal(size=B) * 0.05; xq[:, 0] = rng.normal(size=B) * 0.2
    xt = torch.from_numpy(xq).cuda()
    net = WCRBFNet.from_config(cfg)
    g = torch.randn(B, cfg["out_features"], device="cuda")
    pd = {"params": {gk: {n: torch.from_numpy(v).cuda() for n, v in d.items()} for gk, d in P["params"].items()}}
    print(f"frenet 12 regions (N=1200, O=2) B={B}: forward {timed(lambda: net.apply(pd, xt)):.1f} us, VJP {timed(lambda: net.vjp(pd, xt, g)):.1f} us", flush=True)
    y = torch.from_numpy(rng.normal(size=(B, 2)).astype(np.float32)).cuda()
    st = [train.TrainState.create(net, P)]
    def step():
        st[0], _ = train.train_step_frenet_fullint(st[0], xt, y, DP)
    print(f"   train_step_frenet_fullint (T=1): {timed(step):.1f} us", flush=True)
    # Deeper net
    cfgd, Pd, xd, _ = load_deeper_fixture()
    Pd32 = {"params": {k: {n: torch.from_numpy(np.asarray(v, np.float32)).cuda() for n, v in d.items()} for k, d in Pd["params"].items()}}
    nsd = len(cfgd["activation_idx"])
    lod = np.array([min(cfgd["lower_bounds"][d]) for d in range(nsd)]); hid = np.array([max(cfgd["upper_bounds"][d]) for d in range(nsd)])
    xdq = torch.from_numpy(rng.uniform(lod, hid, size=(B, cfgd["in_features"])).astype(np.float32)).cuda()
    netd = DeeperWCRBFNet.from_config(cfgd)
    gd = torch.randn(B, cfgd["out_features"], device="cuda")
    print(f"deeper (R={cfgd['num_regions']}, K={cfgd['num_kernels']}, O={cfgd['out_features']}) B={B}: forward {timed(lambda: netd.apply(Pd32, xdq)):.1f} us, VJP {timed(lambda: netd.vjp(Pd32, xdq, gd)):.1f} us", flush=True)


# Cluster nets: 11 regions x 100 centres (all at B = 80 000), and the reference's R = 500 x K = 10 / K = 50 (forward at the
# planning batch 65 536, VJP and training step at 80 000).  A row that raises is printed as not measured.
def cluster_rows(R, K, B_fwd, O=10, D=8):
    cfgc = {"in_features": D, "out_features": O, "num_kernels": K, "basis_func": "gaussian", "num_regions": R}
    Pc = {"params": {"rbf_list": {"centers": rng.uniform(-2, 2, size=(R, K, D)).astype(np.float32), "log_sigs": rng.uniform(0.5, 1.5, size=(R, K)).astype(np.float32)},
                     "linear": {"kernel": (rng.normal(size=(K, O)) * 0.3).astype(np.float32), "bias": (rng.normal(size=(O,)) * 0.1).astype(np.float32)},
                     "cluster": {"kernel": rng.normal(size=(D, R)).astype(np.float32), "bias": rng.normal(size=(R,)).astype(np.float32)}}}
    Pcd = {"params": {k: {n: torch.from_numpy(v).cuda() for n, v in d.items()} for k, d in Pc["params"].items()}}
    xc = rng.uniform(-2, 2, size=(B, D)).astype(np.float32); xc[:, 7] = rng.normal(size=B) * 0.05; xc[:, 0] *= 0.1; xc[:, 2] = rng.uniform(1, 6, size=B)
    xct = torch.from_numpy(xc).cuda()
    netc = ClusterWCRBFNet(**cfgc)
    gc = torch.randn(B, O, device="cuda"); gl = torch.randn(B, R, device="cuda")
    yc = torch.from_numpy(np.hstack([rng.normal(size=(B, 5)) * 2, rng.normal(size=(B, 5)) * 0.5]).astype(np.float32)).cuda()
    ids = torch.from_numpy(np.eye(R, dtype=np.float32)[rng.integers(0, R, size=B)]).cuda()
    stc = [train.ClusterTrainState.create(netc, Pc)]
    def stepc():
        stc[0], _ = train.train_step_fullint_withcluster(stc[0], xct, yc, ids, DP)
    def row(what, fn):
        try:
            return f"{what} {timed(fn):.1f} us"
        except ValueError as e:
            torch.cuda.synchronize()
            return f"{what} not measured ({e})"
    print(f"cluster (R={R}, K={K}, O={O}): " + ", ".join([
        row(f"forward B={B_fwd}", lambda: netc.apply(Pcd, xct[:B_fwd])),
        row(f"VJP B={B}", lambda: netc.vjp(Pcd, xct, gc, glogits=gl)),
        row(f"train_step_fullint_withcluster B={B}", stepc)]), flush=True)
if not CLUSTER_ONLY:
    other_rows()
cluster_rows(11, 100, B)
cluster_rows(500, 10, 65536)
cluster_rows(500, 50, 65536)
