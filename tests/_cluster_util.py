"""ClusterWCRBFNet test helpers shared by test_gpu_train.py and test_gpu_cluster_scale.py: seeded synthetic parameters and
queries, the six gradient leaves, and the float64 restatement (oracle/irbfn_oracle.py) run in row chunks, so that its
[B, R, K, D] intermediate stays small at the reference's R * K = 25 000.  A plain module (no fixtures, no hooks)."""
import numpy as np
import torch

from oracle import irbfn_oracle as orc

LEAVES = (("rbf_list", "centers"), ("rbf_list", "log_sigs"), ("linear", "kernel"), ("linear", "bias"))
CLEAVES = LEAVES + (("cluster", "kernel"), ("cluster", "bias"))
CHUNK_ELEMS = 1 << 24          # float64 elements of one chunk's [rows, R, K, D] difference tensor


def cluster_case(seed, R=11, K=20, O=10, B=400, D=8, basis="gaussian"):
    """(rng, cfg, params, x): synthetic float32 parameters of a ClusterWCRBFNet and B queries in the centres' box.  The
    queries are drawn independently of the centres, so none sits on one (the restatement's sqrt has an infinite
    derivative at 0)."""
    rng = np.random.default_rng(seed)
    cfg = {"in_features": D, "out_features": O, "num_kernels": K, "basis_func": basis, "num_regions": R}
    params = {"params": {
        "rbf_list": {"centers": rng.uniform(-2, 2, size=(R, K, D)).astype(np.float32),
                     "log_sigs": rng.uniform(0.5, 1.5, size=(R, K)).astype(np.float32)},
        "linear": {"kernel": (rng.normal(size=(K, O)) * 0.3).astype(np.float32), "bias": (rng.normal(size=(O,)) * 0.1).astype(np.float32)},
        "cluster": {"kernel": rng.normal(size=(D, R)).astype(np.float32), "bias": rng.normal(size=(R,)).astype(np.float32)}}}
    x = rng.uniform(-2, 2, size=(B, D)).astype(np.float32)
    return rng, cfg, params, x


def t64(params, requires_grad=True):
    return {"params": {k: {n: torch.tensor(np.asarray(v, np.float64), requires_grad=requires_grad) for n, v in d.items()}
                       for k, d in params["params"].items()}}


def row_chunk(cfg):
    return max(1, CHUNK_ELEMS // (cfg["num_regions"] * cfg["num_kernels"] * cfg["in_features"]))


def oracle_apply(cfg, params, x):
    """(out, logits) of the float64 restatement, as float64 NumPy arrays, in row chunks."""
    tp = t64(params, requires_grad=False)
    xs = torch.tensor(np.asarray(x, np.float64))
    c = row_chunk(cfg)
    outs, logits = [], []
    with torch.no_grad():
        for i in range(0, xs.shape[0], c):
            o, lg = orc.cluster_wcrbfnet_apply(cfg, tp, xs[i:i + c])
            outs.append(o.numpy())
            logits.append(lg.numpy())
    return np.concatenate(outs), np.concatenate(logits)


def oracle_vjp(cfg, params, x, g, gl=None):
    """torch.autograd of the float64 restatement: the six leaves of d/dparams [sum(out * g) (+ sum(logits * gl))], the row
    chunks' gradients summed.  Returns (without_gl, with_gl); with_gl is None if gl is None.  The logits term reaches the
    cluster leaves only and is differentiated on its own graph, so one forward serves both."""
    tp = t64(params)
    leaves = [tp["params"][g_][n_] for g_, n_ in CLEAVES]
    xs = torch.tensor(np.asarray(x, np.float64))
    gs = torch.tensor(np.asarray(g, np.float64))
    gls = torch.tensor(np.asarray(gl, np.float64)) if gl is not None else None
    c = row_chunk(cfg)
    acc = [torch.zeros_like(t) for t in leaves]
    accl = [torch.zeros_like(t) for t in leaves[4:]]
    for i in range(0, xs.shape[0], c):
        out, logits = orc.cluster_wcrbfnet_apply(cfg, tp, xs[i:i + c])
        grads = torch.autograd.grad((out * gs[i:i + c]).sum(), leaves, retain_graph=gls is not None)
        acc = [a + b for a, b in zip(acc, grads)]
        if gls is not None:
            gl_grads = torch.autograd.grad((logits * gls[i:i + c]).sum(), leaves[4:])
            accl = [a + b for a, b in zip(accl, gl_grads)]
    base = {k: a.numpy() for k, a in zip(CLEAVES, acc)}
    if gls is None:
        return base, None
    with_gl = dict(base)
    for k, a in zip(CLEAVES[4:], accl):
        with_gl[k] = base[k] + a.numpy()
    return base, with_gl


def oracle_train_loss(cfg, params, x, y, ids, dyn_params, grad=True):
    """train_fullint_withcluster_loss of the float64 restatement over row chunks: every term of the loss is a mean over
    rows, so the chunk losses are added with weights rows / B.  Returns (loss, flat six-leaf gradient or None)."""
    tp = t64(params, requires_grad=grad)
    B = x.shape[0]
    c = row_chunk(cfg)
    total = 0.0
    with torch.set_grad_enabled(grad):
        for i in range(0, B, c):
            j = min(B, i + c)
            t = lambda a: torch.tensor(np.asarray(a[i:j], np.float64))
            lc = orc.train_fullint_withcluster_loss(cfg, tp, t(x), t(y), t(ids), dyn_params) * ((j - i) / B)
            if grad:
                lc.backward()
            total += float(lc.detach())
    if not grad:
        return total, None
    return total, np.concatenate([tp["params"][g_][n_].grad.numpy().reshape(-1) for g_, n_ in CLEAVES])
