"""ClusterWCRBFNet at the reference's sizes, and K1 past 2^21 rows.

The reference trains the cluster net at R = 500 regions, D = 8, O = 10 with K = 10 and K = 50 centres per region
(scripts/ckpts/dnmpc_500_clusters/checkpoint_0, dnmpc_500_clusters_numk50/checkpoint_100).  Those checkpoints are not in
this repository: every case here runs synthetic parameters at their shapes against the float64 restatement
(oracle/irbfn_oracle.py, torch.autograd for gradients), in row chunks (tests/_cluster_util.py).  At (D + 1) * R = 4 500
the gate VJP takes more outputs than one block holds, so its kernel splits them into region chunks.

The last test runs the gated / generic K1 from 2^21 rows, where the planner takes two queries per lane for the fast bases.

Bounds are those of tests/test_gpu_parity.py::test_cluster_wcrbfnet_forward (forward), tests/test_gpu_train.py::
test_cluster_wcrbfnet_vjp (5e-5 of each leaf's max) and ::test_train_step_fullint_withcluster (train step), the
cotangent-additivity bound of tests/test_gpu_fullsize.py::test_cfg3_vjp_full_batch (2e-5 of each leaf's max) for batch
additivity, and for the tanh-gated / single-region nets the 1e-5 |ref| + 3e-6 sum|terms| bound of test_gpu_fullsize.py.
"""
import numpy as np
import pytest
import torch

from _cluster_util import CLEAVES, cluster_case, oracle_apply, oracle_train_loss, oracle_vjp
from _rollout_util import assert_states_close
from conftest import load_ckpt_fixture
from irbfn_amd import _lib, configs, planner, train
from irbfn_amd.model import ClusterWCRBFNet, WCRBFNet
from oracle import c_oracle as co
from oracle import irbfn_oracle as orc

pytestmark = pytest.mark.gpu
DP = np.array(configs.DYN_PARAMS)
R_REF, D_REF, O_REF = 500, 8, 10
FAST = ("gaussian", "inverse_quadratic", "inverse_multiquadric")


def _forward_case(seed, R, K, basis, B):
    """The parameter scales of test_cluster_wcrbfnet_forward (log_sigs in [0, 1), unit Dense weights, gate weights x 2)."""
    rng, cfg, params, x = cluster_case(seed, R=R, K=K, O=O_REF, B=B, D=D_REF, basis=basis)
    p = params["params"]
    p["rbf_list"]["log_sigs"] = rng.uniform(0.0, 1.0, size=(R, K)).astype(np.float32)
    p["linear"]["kernel"] = rng.normal(size=(K, O_REF)).astype(np.float32)
    p["linear"]["bias"] = rng.normal(size=(O_REF,)).astype(np.float32)
    p["cluster"]["kernel"] = rng.normal(size=(D_REF, R)).astype(np.float32) * 2.0
    return cfg, params, x


def _assert_forward(out, logits, ref_out, ref_logits, what):
    out, logits = np.asarray(out, np.float64), np.asarray(logits, np.float64)
    assert np.isfinite(out).all() and np.isfinite(logits).all(), what
    el = np.abs(logits - ref_logits).max()
    eo = np.abs(out - ref_out).max()
    assert el <= 1e-5 * (1 + np.abs(ref_logits).max()), (what, el)
    assert eo <= 2e-5 * np.abs(ref_out).max() + 1e-5, (what, eo, np.abs(ref_out).max())


def _assert_leaves(a, ref, what, leaves=CLEAVES, tol=5e-5):
    for grp, name in leaves:
        got, r = a[grp][name].cpu().numpy().astype(np.float64), ref[(grp, name)]
        assert np.isfinite(got).all(), (what, grp, name)
        e = np.abs(got - r).max() / (np.abs(r).max() + 1e-300)
        assert e <= tol, (what, grp, name, e)


def _equal(a, b):
    return all(torch.equal(a[g][n], b[g][n]) for g, n in CLEAVES)


@pytest.mark.parametrize("K", [10, 50])
@pytest.mark.parametrize("basis", FAST)
def test_cluster_forward_reference_shapes(gpu, basis, K):
    """Row 1: gate + gated K1 with gamma at R = 500, D = 8, O = 10, for batches around a 64-row tile; bitwise repeat."""
    cfg, params, x = _forward_case(K + len(basis), R_REF, K, basis, 4097)
    net = ClusterWCRBFNet(**cfg)
    ref_out, ref_logits = oracle_apply(cfg, params, x)
    for B in (1, 63, 64, 65, 129, 4097):
        xt = torch.from_numpy(x[:B]).cuda()
        out, logits = net.apply(params, xt)
        assert net.stage.last_launch()["kernel"].startswith("rbf_fwd_qlane<D=8,OP=10,Q=1,"), net.stage.last_launch()
        _assert_forward(out.cpu().numpy(), logits.cpu().numpy(), ref_out[:B], ref_logits[:B], (basis, K, B))
        out2, logits2 = net.apply(params, xt)
        assert torch.equal(out, out2) and torch.equal(logits, logits2)


@pytest.mark.parametrize("B", [65536, 80000])
def test_cluster_forward_training_batch(gpu, B):
    """Row 2: R = 500, K = 50 at the planning (65 536) and training (80 000) batch: every 16th row and the last 77 rows
    against float64; the rest through a bitwise repeat and a row permutation that must give the same rows bit for bit."""
    cfg, params, x = _forward_case(B, R_REF, 50, "gaussian", B)
    net = ClusterWCRBFNet(**cfg)
    xt = torch.from_numpy(x).cuda()
    out, logits = net.apply(params, xt)
    rows = np.unique(np.concatenate([np.arange(0, B, 16), np.arange(B - 77, B)]))
    ref_out, ref_logits = oracle_apply(cfg, params, x[rows])
    _assert_forward(out.cpu().numpy()[rows], logits.cpu().numpy()[rows], ref_out, ref_logits, B)
    out2, logits2 = net.apply(params, xt)
    assert torch.equal(out, out2) and torch.equal(logits, logits2)
    perm = torch.from_numpy(np.random.default_rng(B).permutation(B)).cuda()
    out3, logits3 = net.apply(params, xt[perm])
    assert torch.equal(out3, out[perm]) and torch.equal(logits3, logits[perm])


@pytest.mark.parametrize("B", [129, 2049])
@pytest.mark.parametrize("K,basis", [(50, "gaussian"), (10, "inverse_quadratic"), (10, "inverse_multiquadric")])
def test_cluster_vjp_reference_shapes(gpu, K, basis, B):
    """Row 3: all six leaves at R = 500, D = 8, O = 10 with and without a logits cotangent against torch.autograd of the
    float64 restatement; bitwise repeat; exact power-of-two homogeneity vjp(4 g, 4 gl) = 4 vjp(g, gl)."""
    rng, cfg, params, x = cluster_case(K + B, R=R_REF, K=K, O=O_REF, B=B, D=D_REF, basis=basis)
    g = rng.normal(size=(B, O_REF)).astype(np.float32)
    gl = rng.normal(size=(B, R_REF)).astype(np.float32)
    ref, ref_gl = oracle_vjp(cfg, params, x, g, gl)
    net = ClusterWCRBFNet(**cfg)
    xt, gt, glt = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda(), torch.from_numpy(gl).cuda()
    for r, gl_in in ((ref, None), (ref_gl, glt)):
        a = net.vjp(params, xt, gt, glogits=gl_in)["params"]
        _assert_leaves(a, r, (K, basis, B, gl_in is not None))
        assert _equal(a, net.vjp(params, xt, gt, glogits=gl_in)["params"])
        a4 = net.vjp(params, xt, gt * 4.0, glogits=gl_in * 4.0 if gl_in is not None else None)["params"]
        for grp, name in CLEAVES:
            assert torch.equal(a4[grp][name], a[grp][name] * 4.0), (grp, name)


@pytest.mark.parametrize("D,R,B", [(8, 227, 1000), (8, 228, 1000), (8, 500, 1000), (8, 1024, 1000), (3, 512, 1000), (3, 513, 1000),
                                   (8, 500, 1), (8, 500, 63), (8, 500, 64), (8, 500, 16384), (8, 500, 16449)])
def test_cluster_gate_vjp_boundaries(gpu, D, R, B):
    """Row 4: d Wc, d bc around the old (D + 1) R <= 2048 cap (R = 227 / 228 at D = 8, 512 / 513 at D = 3), at R = 1024,
    and at R = 500 around one 64-row tile and 256 blocks x 64 rows (16 384: past it a block takes a second tile).  K = 2
    keeps the oracle cheap."""
    rng, cfg, params, x = cluster_case(R + B + D, R=R, K=2, O=O_REF, B=B, D=D)
    g = rng.normal(size=(B, O_REF)).astype(np.float32)
    gl = rng.normal(size=(B, R)).astype(np.float32)
    ref, ref_gl = oracle_vjp(cfg, params, x, g, gl)
    net = ClusterWCRBFNet(**cfg)
    xt, gt = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()
    for r, gl_in in ((ref, None), (ref_gl, torch.from_numpy(gl).cuda())):
        a = net.vjp(params, xt, gt, glogits=gl_in)["params"]
        _assert_leaves(a, r, (D, R, B, gl_in is not None), leaves=CLEAVES[4:])


def test_cluster_vjp_batch_additivity(gpu):
    """Row 5: R = 500, K = 10 at the training batch 80 000, split at a row that is not a multiple of 64: vjp(x) against
    vjp(x1) + vjp(x2) per leaf.  Both are float32 sums of the same per-row terms in another order; the bound is the one
    test_cfg3_vjp_full_batch uses for the same kind of identity (cotangent additivity), 2e-5 of the leaf's max."""
    B, split = 80000, 40037
    rng, cfg, params, x = cluster_case(5, R=R_REF, K=10, O=O_REF, B=B, D=D_REF)
    g = torch.from_numpy(rng.normal(size=(B, O_REF)).astype(np.float32)).cuda()
    gl = torch.from_numpy(rng.normal(size=(B, R_REF)).astype(np.float32)).cuda()
    xt = torch.from_numpy(x).cuda()
    net = ClusterWCRBFNet(**cfg)
    a = net.vjp(params, xt, g, glogits=gl)["params"]
    assert _equal(a, net.vjp(params, xt, g, glogits=gl)["params"])
    a1 = net.vjp(params, xt[:split], g[:split], glogits=gl[:split])["params"]
    a2 = net.vjp(params, xt[split:], g[split:], glogits=gl[split:])["params"]
    for grp, name in CLEAVES:
        full, parts = a[grp][name], a1[grp][name] + a2[grp][name]
        assert torch.isfinite(full).all()
        e = float((full - parts).abs().max() / full.abs().max())
        assert e <= 2e-5, (grp, name, e)


def _train_inputs(rng, x, R, T=5):
    """Frenet-layout queries (train_step_fullint_withcluster), as test_train_step_fullint_withcluster builds them."""
    B = x.shape[0]
    x[:, 7] = rng.normal(size=B).astype(np.float32) * 0.05
    x[:, 0] = rng.normal(size=B).astype(np.float32) * 0.2
    x[:, 2] = rng.uniform(1.0, 6.0, size=B).astype(np.float32)
    y = np.hstack([rng.normal(size=(B, T)) * 2, rng.normal(size=(B, T)) * 0.5]).astype(np.float32)
    ids = np.eye(R, dtype=np.float32)[rng.integers(0, R, size=B)]
    return x, y, ids


def test_cluster_softmax_edges(gpu):
    """Row 6, R = 500: (a) gamma exactly 0 in all regions but one (K1 skips them; the softmax backward meets
    0 * (dgamma - <gamma, dgamma>)); (b) all logits equal (gamma = 1 / R); (c) |logits| ~ 1e3: no inf or NaN in the
    outputs, the loss or the gradients."""
    R, K, B = R_REF, 10, 1000
    rng, cfg, params, x = cluster_case(6, R=R, K=K, O=O_REF, B=B, D=D_REF)
    g = rng.normal(size=(B, O_REF)).astype(np.float32)
    gl = rng.normal(size=(B, R)).astype(np.float32)
    net = ClusterWCRBFNet(**cfg)
    xt, gt, glt = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda(), torch.from_numpy(gl).cuda()
    p = params["params"]
    one_hot = np.full(R, -200.0, np.float32)
    one_hot[123] = 0.0                                              # exp(-200) underflows to 0 in float32 (and float64: 1e-87)
    for what, wc, bc in (("one region", np.zeros((D_REF, R), np.float32), one_hot),
                         ("equal logits", np.zeros((D_REF, R), np.float32), np.full(R, 0.5, np.float32))):
        p["cluster"] = {"kernel": wc, "bias": bc}
        out, logits = net.apply(params, xt)
        ref_out, ref_logits = oracle_apply(cfg, params, x)
        _assert_forward(out.cpu().numpy(), logits.cpu().numpy(), ref_out, ref_logits, what)
        ref, ref_gl = oracle_vjp(cfg, params, x, g, gl)
        _assert_leaves(net.vjp(params, xt, gt, glogits=glt)["params"], ref_gl, what)
        _assert_leaves(net.vjp(params, xt, gt)["params"], ref, what, leaves=CLEAVES[:4])
        if what == "one region":                                    # no logits cotangent: d Wc, d bc are exactly 0
            a = net.vjp(params, xt, gt)["params"]
            assert not a["cluster"]["kernel"].any() and not a["cluster"]["bias"].any()
    # (c) |logits| ~ 1e3, different leading regions per row
    p["cluster"] = {"kernel": (rng.normal(size=(D_REF, R)) * 300.0).astype(np.float32), "bias": np.zeros(R, np.float32)}
    out, logits = net.apply(params, xt)
    assert float(logits.abs().max()) > 500.0
    _, ref_logits = oracle_apply(cfg, params, x)
    assert torch.isfinite(out).all() and np.abs(logits.cpu().numpy() - ref_logits).max() <= 1e-5 * (1 + np.abs(ref_logits).max())
    a = net.vjp(params, xt, gt, glogits=glt)["params"]
    assert all(torch.isfinite(a[grp][name]).all() for grp, name in CLEAVES)
    xs, y, ids = _train_inputs(rng, x.copy(), R)
    state = train.ClusterTrainState.create(net, params, lr=1e-3, max_grad_norm=1.0)
    state, loss = train.train_step_fullint_withcluster(state, torch.from_numpy(xs).cuda(), torch.from_numpy(y).cuda(),
                                                       torch.from_numpy(ids).cuda(), DP)
    assert np.isfinite(float(loss)) and torch.isfinite(state.g).all() and torch.isfinite(state.flat).all()


def _unflat_like(params, flat):
    off, nxt = 0, {"params": {}}
    for g_, n_ in CLEAVES:
        shp = np.asarray(params["params"][g_][n_]).shape
        cnt = int(np.prod(shp))
        nxt["params"].setdefault(g_, {})[n_] = flat[off:off + cnt].reshape(shp)
        off += cnt
    return nxt


@pytest.mark.parametrize("K,B,steps", [(10, 4096, 2), (50, 1024, 1)])
def test_cluster_train_step_reference_shapes(gpu, K, B, steps):
    """Row 7: train_step_fullint_withcluster at R = 500: loss, six-leaf gradient and clip + Adam update against the
    restatement, with the bounds of test_train_step_fullint_withcluster."""
    rng, cfg, params, x = cluster_case(K * 7 + steps, R=R_REF, K=K, O=O_REF, B=B, D=D_REF)
    x, y, ids = _train_inputs(rng, x, R_REF)
    net = ClusterWCRBFNet(**cfg)
    state = train.ClusterTrainState.create(net, params, lr=1e-3, max_grad_norm=1.0)
    n = state.flat.numel()
    p_ref = np.concatenate([np.asarray(params["params"][g_][n_], np.float64).reshape(-1) for g_, n_ in CLEAVES])
    assert n == p_ref.size
    m, v, cur = np.zeros(n), np.zeros(n), params
    xt, yt, it = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(ids).cuda()
    for t in range(1, steps + 1):
        loss, g_ref = oracle_train_loss(cfg, cur, x, y, ids, DP)
        p_ref, m, v = orc.adam_update(p_ref, orc.clip_by_global_norm(g_ref, 1.0), m, v, t, lr=1e-3)
        state, l_gpu = train.train_step_fullint_withcluster(state, xt, yt, it, DP)
        assert abs(float(l_gpu) - loss) <= 3e-5 * abs(loss), (t, float(l_gpu), loss)
        g_gpu = state.g.cpu().numpy()
        assert np.abs(g_gpu - g_ref).max() <= 5e-4 * np.abs(g_ref).max(), (t, np.abs(g_gpu - g_ref).max() / np.abs(g_ref).max())
        assert np.abs(state.flat.cpu().numpy() - p_ref).max() <= 5e-5 + 1e-6 * np.abs(p_ref).max()
        cur = _unflat_like(params, p_ref)                           # the oracle's next step starts from its own parameters


def test_cluster_train_step_training_batch(gpu):
    """Row 8: one train step at R = 500, K = 10 and the reference's batch 80 000: loss against the float64 restatement
    (bound of test_train_step_fullint_withcluster), finite gradient, bitwise repeat from the same state."""
    B = 80000
    rng, cfg, params, x = cluster_case(8, R=R_REF, K=10, O=O_REF, B=B, D=D_REF)
    x, y, ids = _train_inputs(rng, x, R_REF)
    net = ClusterWCRBFNet(**cfg)
    xt, yt, it = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(ids).cuda()
    runs = []
    for _ in range(2):
        state = train.ClusterTrainState.create(net, params, lr=1e-3, max_grad_norm=1.0)
        state, loss = train.train_step_fullint_withcluster(state, xt, yt, it, DP)
        runs.append((loss.clone(), state.g.clone(), state.flat.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert torch.isfinite(runs[0][1]).all()
    ref, _ = oracle_train_loss(cfg, params, x, y, ids, DP, grad=False)
    assert abs(float(runs[0][0]) - ref) <= 3e-5 * abs(ref), (float(runs[0][0]), ref)


# --- K1 past 2^21 rows --------------------------------------------------------------------------------------------------
B_Q2 = 64 * 32768                                                   # plan_qlane takes Q = 2 from here (OP in {2, 5, 10})
BATCHES = (B_Q2 - 1, B_Q2, B_Q2 + 77)


def _check_rows(B):
    """The first 4 096 rows, the rows around 2^21 and the last tile."""
    return np.unique(np.concatenate([np.arange(4096), np.arange(B_Q2 - 192, min(B, B_Q2 + 192)), np.arange(B - 128, B)]))


def _single_region_net(basis, O, D=8, N=256, seed=0):
    rng = np.random.default_rng(seed)
    # one region whose tanh gate is exactly 1 in float64 for |x_0| <= 2 (tanh(100 * 98) == 1)
    card = {"in_features": D, "out_features": O, "num_kernels": N, "basis_func": basis, "num_regions": 1,
            "lower_bounds": [[-100.0]], "upper_bounds": [[100.0]], "dimension_ranges": [[0]], "activation_idx": [0],
            "delta": [100.0]}
    P = {"params": {"rbf_list": {"centers": rng.uniform(-2, 2, size=(1, N, D)).astype(np.float32),
                                 "log_sigs": rng.uniform(0.0, 1.0, size=(1, N)).astype(np.float32)},
                    "linear": {"kernel": (rng.normal(size=(N, O)) * 0.3).astype(np.float32),
                               "bias": (rng.normal(size=(O,)) * 0.1).astype(np.float32)}}}
    x = rng.uniform(-2, 2, size=(BATCHES[-1], D)).astype(np.float32)
    return card, P, x


def _in_range_queries(cfg, B, seed):
    rng = np.random.default_rng(seed)
    ns, D = len(cfg["activation_idx"]), cfg["in_features"]
    lo = np.array([min(cfg["lower_bounds"][d]) for d in range(ns)])
    hi = np.array([max(cfg["upper_bounds"][d]) for d in range(ns)])
    return np.hstack([rng.uniform(lo, hi, size=(B, ns)), rng.normal(size=(B, D - ns)) * 0.1]).astype(np.float32)


def _assert_wcrbf_rows(cfg, P, x, got, what):
    """1e-5 |ref| + 3e-6 sum_k |h_k W_ko| (+ |bias|) against the float64 C oracle (test_gpu_fullsize.py's bound)."""
    P64 = orc.cast_params(P, np.float64)
    ref = co.wcrbf_forward(cfg, P64, x.astype(np.float64), np.float64)
    _, h, _ = orc.wcrbfnet_apply(cfg, P64, x.astype(np.float64), return_aux=True)
    scale = np.abs(h) @ np.abs(P64["params"]["linear"]["kernel"]) + np.abs(P64["params"]["linear"]["bias"])
    err = np.abs(np.asarray(got, np.float64) - ref)
    bad = err > 1e-5 * np.abs(ref) + 3e-6 * scale
    assert not bad.any(), (what, int(bad.sum()), float(err.max()))


def _expect_q(kernel, B, fast, what):
    assert kernel.startswith("rbf_fwd_qlane<"), (what, kernel)
    q = 2 if (fast and B >= B_Q2) else 1
    assert f",Q={q}," in kernel, (what, B, kernel)


NETS_2P21 = ["frenet12", "cluster_gaussian", "cluster_matern52", "matern32_O2", "matern32_O5", "matern32_O10",
             "spline_O2", "spline_O5", "spline_O10", "gaussian_K1_O5", "tick_128regions"]


@pytest.mark.parametrize("kind", NETS_2P21)
def test_k1_past_2p21_rows(gpu, kind):
    """Row 9: the nets that reach K1 with a padded width OP in {2, 5, 10} at 2^21 - 1, 2^21 and 2^21 + 77 rows.  The kernel
    name shows Q = 1 below 2^21 and, from 2^21, Q = 2 for the fast bases and Q = 1 for the generic ones (which have no
    Q = 2 instance); then the first 4 096 rows, the rows around 2^21 and the last tile against float64."""
    if kind == "frenet12" or kind == "tick_128regions":
        cfg, P, *_ = load_ckpt_fixture("dnmpc_12regions_frenet_l1_bigdata" if kind == "frenet12" else "dnmpc_128regions")
        P = {"params": {g: {n: np.asarray(v, np.float32) for n, v in d.items()} for g, d in P["params"].items()}}
        net, fast = WCRBFNet.from_config(cfg), True
        x = _in_range_queries(cfg, BATCHES[-1], seed=9)
        if kind == "tick_128regions":
            net.set_options(fwd_kernel=_lib.FWD_K1)                 # the dense-gate tick, fused roll-out (ROLL=1)
            s0 = configs.initial_state_from_query(x)
    elif kind.startswith("cluster_"):
        basis = kind.split("_")[1]
        cfg, params, x = _forward_case(16, 16, 64, basis, BATCHES[-1])
        net, fast = ClusterWCRBFNet(**cfg), basis == "gaussian"
    else:
        basis, O = kind.split("_")[0], int(kind.split("_O")[1])
        cfg, P, x = _single_region_net(basis, O, seed=O)
        net, fast = WCRBFNet.from_config(cfg), basis == "gaussian"
        if basis == "gaussian":
            net.set_options(fwd_kernel=_lib.FWD_K1)
    xt_all = torch.from_numpy(x).cuda()
    for B in BATCHES:
        xt, rows = xt_all[:B], _check_rows(B)
        what = (kind, B)
        if kind.startswith("cluster_"):
            out, logits = net.apply(params, xt)
            _expect_q(net.stage.last_launch()["kernel"], B, fast, what)
            ref_out, ref_logits = oracle_apply(cfg, params, x[rows])
            _assert_forward(out.cpu().numpy()[rows], logits.cpu().numpy()[rows], ref_out, ref_logits, what)
        elif kind == "tick_128regions":
            ctrl, states = planner.plan_tick(net, P, xt, None, s0[:B], configs.DYN_PARAMS, mode=_lib.ROLLOUT_ST_KS)
            kern = net.last_launch()["kernel"]
            _expect_q(kern, B, fast, what)
            assert "ROLL=1" in kern, kern
            u = ctrl.cpu().numpy()[rows]
            _assert_wcrbf_rows(cfg, P, x[rows], u, what)
            xu = np.hstack([s0[rows], u])
            assert_states_close(states.cpu().numpy()[rows], orc.integrate_st_ks_mult(xu.astype(np.float64), DP),
                                orc.integrate_st_ks_mult(xu.astype(np.float32), DP.astype(np.float32)))
        else:
            out = net.apply(P, xt)
            kern = net.last_launch()["kernel"]
            _expect_q(kern, B, fast, what)
            if kind == "frenet12":
                assert "GATED=1" in kern, kern
            _assert_wcrbf_rows(cfg, P, x[rows], out.cpu().numpy()[rows], what)
