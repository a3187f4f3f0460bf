"""DeeperWCRBFNet training on the GPU: K2m (the stage VJP with hbar and dW on the f32 matrix cores) against the float64
oracle, the DeeperWCRBFNet.vjp keywords, and DeeperTrainState steps against torch.autograd of the restated losses."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_deeper_fixture
from irbfn_amd import _lib, checkpoint, configs, distributed, tables, train
from irbfn_amd.model import DeeperWCRBFNet, WCRBFNet
from oracle import irbfn_oracle as orc

pytestmark = pytest.mark.gpu

DP = np.array(configs.DYN_PARAMS)
STAGE = (("rbf_list", "centers"), ("rbf_list", "log_sigs"), ("linear", "kernel"), ("linear", "bias"))
LEAVES = DeeperWCRBFNet.LEAVES


def _card(D, O, K, basis, R=1):
    return {"in_features": D, "out_features": O, "num_kernels": K, "basis_func": basis, "num_regions": R,
            "lower_bounds": [[-10.0, -10.0]], "upper_bounds": [[10.0, 10.0]], "dimension_ranges": [[0], [1]][:max(R, 1)] if R <= 2
            else [[r % 2] for r in range(R)], "activation_idx": [0], "delta": [1.0]}


def _net_case(D, O, K, B, basis, seed):
    rng = np.random.default_rng(seed)
    P = {"params": {"rbf_list": {"centers": rng.uniform(-1, 1, size=(1, K, D)).astype(np.float32),
                                 "log_sigs": rng.uniform(-0.5, 0.5, size=(1, K)).astype(np.float32)},
                    "linear": {"kernel": (rng.normal(size=(K, O)) / np.sqrt(K)).astype(np.float32),
                               "bias": rng.normal(size=O).astype(np.float32)}}}
    x = rng.uniform(-1.2, 1.2, size=(B, D)).astype(np.float32)
    x[:min(B, 3)] = P["params"]["rbf_list"]["centers"][0, :min(B, 3)]          # queries on centres
    g = rng.normal(size=(B, O)).astype(np.float32)
    return _card(D, O, K, basis), P, x, g


def _k2m(cfg, P, x, g):
    net = WCRBFNet.from_config(cfg)
    net.set_options(vjp_kernel=_lib.VJP_K2M)
    got = net.vjp(P, torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda())["params"]
    return net, {k: v.cpu().numpy() for k, v in [(n, got[gr][n]) for gr, n in STAGE]}


def _check_leaves(got, ref, what):
    for grp, n in STAGE:
        a, b = got[n], np.asarray(ref[grp][n])
        assert a.shape == b.shape, (what, n)
        assert np.abs(a - b).max() <= 5e-5 * np.abs(b).max() + 1e-7, (what, n, np.abs(a - b).max() / np.abs(b).max())


# ------------------------------------------------------------------ K2m
SWEEP = [(O, D, basis) for O in (17, 32, 64, 100, 128) for D in (3, 4, 6, 8)
         for basis in ("gaussian", "inverse_quadratic", "inverse_multiquadric")]


@pytest.mark.parametrize("O,D,basis", SWEEP)
def test_k2m_matches_the_oracle(gpu, O, D, basis):
    """Every width, padded d in {3, 4, 7, 8} (D = 6 pads to 7) and fast basis; K and B cycle through 100 / 1000 centres and
    1 / 63 / 4096 queries; three queries sit on centres.  All four leaves at K2's bound, the launch is K2m, two calls agree
    bit for bit."""
    i = SWEEP.index((O, D, basis))
    K, B = (100, 1000)[i % 2], (1, 63, 4096)[i % 3]
    cfg, P, x, g = _net_case(D, O, K, B, basis, seed=i)
    net, got = _k2m(cfg, P, x, g)
    name = net.last_launch()["kernel"]
    assert name.startswith("rbf_vjp_mfma<"), name
    _check_leaves(got, orc.wcrbfnet_vjp(cfg, P, x.astype(np.float64), g.astype(np.float64))["params"], (O, D, basis, K, B))
    _, again = _k2m(cfg, P, x, g)
    for n in got:
        assert np.array_equal(got[n], again[n]), n


@pytest.mark.parametrize("K,B,O", [(4096, 4096, 64), (100, 80000, 64), (1000, 80000, 100), (4096, 63, 17)])
def test_k2m_large(gpu, K, B, O):
    cfg, P, x, g = _net_case(8, O, K, B, "gaussian", seed=K + B)
    _, got = _k2m(cfg, P, x, g)
    _check_leaves(got, orc.wcrbfnet_vjp(cfg, P, x.astype(np.float64), g.astype(np.float64))["params"], (K, B, O))


def test_k2m_refusals_and_auto_unchanged(gpu):
    lib = _lib.load()
    cases = {"regions": _card(8, 64, 100, "gaussian", R=2), "generic": _card(8, 64, 100, "multiquadric"),
             "narrow": _card(8, 16, 100, "gaussian")}
    for what, cfg in cases.items():
        _, P, x, g = _net_case(8, cfg["out_features"], 100, 300, "gaussian", seed=3)
        if cfg["num_regions"] == 2:
            P["params"]["rbf_list"] = {k: np.concatenate([v, v]) for k, v in P["params"]["rbf_list"].items()}
        net = WCRBFNet.from_config(cfg)
        net.bind(P)
        h = net._handle(torch)
        assert lib.irbfn_net_vjp_kernel_supported(h, _lib.VJP_K2M, 300) == 0, what
        assert lib.irbfn_net_vjp_kernel_supported(h, _lib.VJP_K2, 300) == 1, what
        net.set_options(vjp_kernel=_lib.VJP_K2M)
        with pytest.raises(ValueError, match="IRBFN_ERR_UNSUPPORTED"):
            net.vjp(P, x, g)
    # a 64-wide one-region net: supported, yet AUTO keeps K2 and its bits
    cfg, P, x, g = _net_case(8, 64, 100, 4096, "gaussian", seed=4)
    net = WCRBFNet.from_config(cfg)
    got = net.vjp(P, x, g)["params"]
    assert net.last_launch()["kernel"].startswith("rbf_vjp_kernel<"), net.last_launch()
    assert lib.irbfn_net_vjp_kernel_supported(net._handle(torch), _lib.VJP_K2M, 4096) == 1
    net.set_options(vjp_kernel=_lib.VJP_K2)
    forced = net.vjp(P, x, g)["params"]
    for grp, n in STAGE:
        assert np.array_equal(got[grp][n], forced[grp][n]), n
    assert lib.irbfn_net_vjp_kernel_supported(net._handle(torch), 6, 10) < 0


# ------------------------------------------------------------------ DeeperWCRBFNet.vjp keywords
def _golden(B=300, seed=9):
    cfg, P, _, _ = load_deeper_fixture()
    P = {"params": {g: {n: np.asarray(v, np.float32) for n, v in d.items()} for g, d in P["params"].items()}}
    rng = np.random.default_rng(seed)
    ns = len(cfg["activation_idx"])
    lo = np.array([min(cfg["lower_bounds"][d]) for d in range(ns)]); hi = np.array([max(cfg["upper_bounds"][d]) for d in range(ns)])
    x = rng.uniform(lo, hi, size=(B, 8)).astype(np.float32)
    x[:, 7] = rng.normal(size=B).astype(np.float32) * 0.05
    x[:, 0] = rng.normal(size=B).astype(np.float32) * 0.2
    T = cfg["out_features"] // 2
    y = np.hstack([rng.normal(size=(B, T)) * 2, rng.normal(size=(B, T)) * 0.5]).astype(np.float32)
    return cfg, P, x, y


def _dev(P):
    return {"params": {g: {n: torch.from_numpy(np.ascontiguousarray(v)).cuda() for n, v in d.items()} for g, d in P["params"].items()}}


def test_deeper_vjp_keywords(gpu):
    cfg, P, x, _ = _golden(B=2000)
    net = DeeperWCRBFNet.from_config(cfg)
    Pd, xd = _dev(P), torch.from_numpy(x).cuda()
    gout = torch.from_numpy(np.random.default_rng(2).normal(size=(2000, net.out_features)).astype(np.float32)).cuda()
    plain = net.vjp(Pd, xd, gout)["params"]
    again = net.vjp(Pd, xd, gout)["params"]
    out, h1 = net.apply_with_hidden(Pd, xd)
    assert torch.equal(out, net.apply(Pd, xd)) and tuple(h1.shape) == (2000, 64)
    flat = torch.zeros(distributed.flat_param_count(net), device="cuda")
    views = distributed.unflatten_params(net, flat)
    opts0 = [net.stage._handle(torch)]
    lib = _lib.load()

    def opt():
        v = __import__("ctypes").c_int(0)
        lib.irbfn_net_get_option(opts0[0], _lib.OPTIONS["vjp_kernel"], __import__("ctypes").byref(v))
        return v.value
    before = opt()
    res = net.vjp(Pd, xd, gout, out=views, h1=h1, stage_vjp_kernel=_lib.VJP_K2M)["params"]
    assert opt() == before
    assert net.stage.last_launch()["kernel"].startswith("rbf_vjp_mfma<")
    for g, n in LEAVES:
        assert torch.equal(plain[g][n], again[g][n]), (g, n)                     # no keyword: deterministic, as before
        assert res[g][n].data_ptr() == views["params"][g][n].data_ptr()
        a, b = res[g][n].cpu().numpy(), plain[g][n].cpu().numpy()
        assert np.abs(a - b).max() <= 5e-5 * np.abs(b).max() + 1e-7, (g, n)
    for g, n in (("linear_pre2", "kernel"), ("linear_pre2", "bias"), ("linear", "kernel"), ("linear", "bias")):
        assert torch.equal(res[g][n], plain[g][n]), (g, n)                       # the head's VJP is the same kernel
    with pytest.raises(ValueError):
        net.vjp(Pd, xd, gout, h1=h1[:10])


def test_deeper_vjp_unchanged_without_keywords(gpu):
    """The golden net's VJP without the new keywords equals the composition the previous version ran: stage forward, head
    VJP, stage VJP on the stage descriptor's automatic kernel."""
    cfg, P, x, _ = _golden(B=1500, seed=4)
    net = DeeperWCRBFNet.from_config(cfg)
    Pd, xd = _dev(P), torch.from_numpy(x).cuda()
    gout = torch.from_numpy(np.random.default_rng(5).normal(size=(1500, net.out_features)).astype(np.float32)).cuda()
    got = net.vjp(Pd, xd, gout)["params"]
    p = Pd["params"]
    stage_p = {"rbf_list": p["rbf_list"], "linear": p["linear_pre1"]}
    ref_net = DeeperWCRBFNet.from_config(cfg)
    h1 = ref_net.stage.apply(stage_p, xd)
    lib = _lib.load()
    from irbfn_amd.model import _ptr, _stream_ptr
    gh1 = torch.empty((1500, 64), device="cuda")
    gw2, gb2 = torch.empty((64, 64), device="cuda"), torch.empty(64, device="cuda")
    gw3, gb3 = torch.empty((64, net.out_features), device="cuda"), torch.empty(net.out_features, device="cuda")
    nb = int(lib.irbfn_mlp_head_vjp_workspace_bytes(64, 64, net.out_features))
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    _lib.check(lib.irbfn_mlp_head_vjp(_ptr(h1), _ptr(p["linear_pre2"]["kernel"]), _ptr(p["linear_pre2"]["bias"]),
                                      _ptr(p["linear"]["kernel"]), _ptr(gout), _ptr(gh1), _ptr(gw2), _ptr(gb2), _ptr(gw3), _ptr(gb3),
                                      1500, 64, 64, net.out_features, _ptr(ws), nb, _stream_ptr(torch)), "head")
    gs = ref_net.stage.vjp(stage_p, xd, gh1)["params"]
    ref = {"rbf_list": gs["rbf_list"], "linear_pre1": gs["linear"], "linear_pre2": {"kernel": gw2, "bias": gb2},
           "linear": {"kernel": gw3, "bias": gb3}}
    for g, n in LEAVES:
        assert torch.equal(got[g][n], ref[g][n]), (g, n)


# ------------------------------------------------------------------ DeeperTrainState
def _deeper_torch(cfg, tp, x):
    return orc.deeper_wcrbfnet_apply(cfg, tp, x)


def _frenet_loss(cfg, tp, x, y):
    """scripts/train_nmpc_frenet.py:394-421 with the Deeper net: L1 on the predictions + L1 on the Frenet roll-out."""
    y_pred = orc.deeper_wcrbfnet_apply(cfg, tp, x)
    init = x[:, [0, 0, 1, 2, 3, 5, 6, 7]]
    actual = orc.integrate_frenet_mult(torch.hstack((init, y)), DP)
    pred = orc.integrate_frenet_mult(torch.hstack((init, y_pred)), DP)
    return (y_pred - y).abs().mean() + (pred - actual).abs().mean()


def _tparams(P):
    return {"params": {g: {n: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True) for n, v in d.items()}
                       for g, d in P["params"].items()}}


def _oracle_step(P, loss_fn, lr=1e-3, max_norm=1.0):
    tp = _tparams(P)
    loss = loss_fn(tp)
    loss.backward()
    g = np.concatenate([tp["params"][g_][n].grad.numpy().reshape(-1) for g_, n in LEAVES])
    flat = np.concatenate([np.asarray(P["params"][g_][n], np.float64).reshape(-1) for g_, n in LEAVES])
    gc = orc.clip_by_global_norm(g, max_norm)
    p_new, _, _ = orc.adam_update(flat, gc, np.zeros_like(flat), np.zeros_like(flat), 1, lr=lr)
    return float(loss.detach()), g, p_new


def _check_step(state, loss, ref):
    loss_ref, g_ref, p_ref = ref
    assert abs(float(loss) - loss_ref) <= 3e-5 * abs(loss_ref), (float(loss), loss_ref)
    g_gpu = state.g.cpu().numpy()
    assert np.abs(g_gpu - g_ref).max() <= 5e-4 * np.abs(g_ref).max(), np.abs(g_gpu - g_ref).max() / np.abs(g_ref).max()
    off = 0
    for g_, n in LEAVES:                                   # every one of the eight gradients, each at the bound of its own scale
        cnt = int(np.prod(state.grads["params"][g_][n].shape))
        a, b = g_gpu[off:off + cnt], g_ref[off:off + cnt]
        assert np.abs(a - b).max() <= 5e-4 * np.abs(g_ref).max(), (g_, n)
        off += cnt
    assert np.abs(state.flat.cpu().numpy() - p_ref).max() <= 5e-5 + 1e-6 * np.abs(p_ref).max()


def test_deeper_train_step_frenet_fullint_golden(gpu):
    cfg, P, x, y = _golden()
    net = DeeperWCRBFNet.from_config(cfg)
    state = train.DeeperTrainState.create(net, P, lr=1e-3, max_grad_norm=1.0)
    assert state.stage_vjp_kernel(300) == _lib.VJP_K2M
    ref = _oracle_step(P, lambda tp: _frenet_loss(cfg, tp, torch.tensor(x, dtype=torch.float64), torch.tensor(y, dtype=torch.float64)))
    state, loss = train.train_step_frenet_fullint(state, torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), DP)
    assert net.stage.last_launch()["kernel"].startswith("rbf_vjp_mfma<")
    _check_step(state, loss, ref)


@pytest.mark.parametrize("kind", ["fullint", "oneint"])
def test_deeper_train_step_fullint_and_oneint(gpu, kind, monkeypatch):
    cfg, P, x, y = _golden(seed=11)
    stage_apply = orc.wcrbfnet_apply

    def deeper(c, p, xx, **kw):          # the oracle's losses with the Deeper net in place of the WCRBFNet
        q = p["params"]
        h = stage_apply(dict(c, out_features=64), {"rbf_list": q["rbf_list"], "linear": q["linear_pre1"]}, xx)
        h2 = torch.relu(h) @ q["linear_pre2"]["kernel"] + q["linear_pre2"]["bias"]
        return torch.relu(h2) @ q["linear"]["kernel"] + q["linear"]["bias"]
    xt, yt = torch.tensor(x, dtype=torch.float64), torch.tensor(y, dtype=torch.float64)
    monkeypatch.setattr(orc, "wcrbfnet_apply", deeper)
    if kind == "fullint":
        ref = _oracle_step(P, lambda tp: orc.train_fullint_loss(cfg, tp, xt, yt))
    else:
        ref = _oracle_step(P, lambda tp: orc.train_oneint_loss(cfg, tp, xt, yt, DP))
    monkeypatch.undo()
    net = DeeperWCRBFNet.from_config(cfg)
    state = train.DeeperTrainState.create(net, P, lr=1e-3, max_grad_norm=1.0)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    if kind == "fullint":
        state, loss = train.train_step_fullint(state, xd, yd)
    else:
        state, loss = train.train_step_oneint(state, xd, yd, DP)
    _check_step(state, loss, ref)


def test_deeper_training_behaviour(gpu, tmp_path):
    cfg, P, x, y = _golden(B=2048, seed=21)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    net = DeeperWCRBFNet.from_config(cfg)
    state = train.DeeperTrainState.create(net, P, lr=1e-3, max_grad_norm=1.0)
    lib = _lib.load()
    import ctypes

    def options():
        h, v, out = net.stage._handle(torch), ctypes.c_int(0), []
        for k in sorted(_lib.OPTIONS.values()):
            lib.irbfn_net_get_option(h, k, ctypes.byref(v))
            out.append(v.value)
        return out
    before = options()
    losses = []
    for _ in range(20):
        state, loss = train.train_step_frenet_fullint(state, xd, yd, DP)
        losses.append(loss)
    assert options() == before                               # the per-call kernel choice leaves no trace on the descriptor
    losses = torch.cat(losses).cpu().numpy()
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    # save after n steps, restore, continue == an uninterrupted run, bit for bit
    run = train.DeeperTrainState.create(DeeperWCRBFNet.from_config(cfg), P, lr=1e-3, max_grad_norm=1.0)
    for _ in range(3):
        run, _ = train.train_step_frenet_fullint(run, xd, yd, DP)
    path = checkpoint.save_checkpoint(str(tmp_path), run.params, 3, opt_state=run.opt_state())
    for _ in range(2):
        run, _ = train.train_step_frenet_fullint(run, xd, yd, DP)
    params, step = checkpoint.restore_checkpoint(path)
    assert step == 3
    res = train.DeeperTrainState.create(DeeperWCRBFNet.from_config(cfg), params, lr=1e-3, max_grad_norm=1.0,
                                        opt_state=checkpoint.restore_opt_state(path))
    for _ in range(2):
        res, _ = train.train_step_frenet_fullint(res, xd, yd, DP)
    assert torch.equal(res.flat, run.flat) and torch.equal(res.m, run.m) and torch.equal(res.v, run.v)
    assert int(res.step.item()) == int(run.step.item()) == 5
    # train_epoch over a synthetic DeviceTable
    tab = tables.DeviceTable(x, y)
    st = train.DeeperTrainState.create(DeeperWCRBFNet.from_config(cfg), P, lr=1e-3, max_grad_norm=1.0)
    st, ls = train.train_epoch(st, tab, batch_size=512)
    assert ls.numel() == 4 and bool(torch.isfinite(ls).all())


def test_deeper_train_two_ranks_unequal_shards(gpu, tmp_path):
    cfg, P, x, y = _golden(B=301, seed=8)
    inp, out = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(inp, x=x, y=y, **{f"{g}__{n}": P["params"][g][n] for g, n in LEAVES})
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", "29549", os.path.join(root, "tests", "_train_two_ranks_deeper.py"), inp, out],
                       cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    two = np.load(out)
    assert tuple(two["shard"]) == (0, 151)
    state = train.DeeperTrainState.create(DeeperWCRBFNet.from_config(cfg), P, lr=1e-3, max_grad_norm=1.0)
    losses = []
    for _ in range(2):
        state, loss = train.train_step_frenet_fullint(state, torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), DP)
        losses.append(float(loss))
    g1, f1 = state.g.cpu().numpy(), state.flat.cpu().numpy()
    assert np.abs(two["losses"] - np.array(losses)).max() <= 2e-6 * np.abs(losses).max(), (two["losses"], losses)
    assert np.abs(two["g"] - g1).max() <= 2e-5 * np.abs(g1).max()
    assert np.abs(two["flat"] - f1).max() <= 2e-6 + 1e-6 * np.abs(f1).max()
