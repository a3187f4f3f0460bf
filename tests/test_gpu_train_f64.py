"""float64 training (the reference under --use_float64, scripts/train_nmpc.py:41-42): a ``WCRBFNet(use_float64=True)`` gets a
float64 ``TrainState`` and its steps run the float64 forward / VJP and the ``*_f64`` seed and clip + Adam kernels.  Held to
float64 accuracy against torch.autograd of the restatement (loss 1e-12, gradient 1e-10 of max|g|) and against the oracle's
clip + Adam applied to the GPU's own gradient (1e-13 of max|p|: Adam amplifies gradient error in small components)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_ckpt_fixture
from irbfn_amd import checkpoint, configs, tables, train
from irbfn_amd.model import WCRBFNet
from oracle import irbfn_oracle as orc

pytestmark = pytest.mark.gpu
DP = np.array(configs.DYN_PARAMS, np.float64)
LEAVES = (("rbf_list", "centers"), ("rbf_list", "log_sigs"), ("linear", "kernel"), ("linear", "bias"))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host(state):
    return {"params": {g: {n: t.cpu().numpy() for n, t in d.items()} for g, d in state.params["params"].items()}}


def _check_steps(cfg, net, params, x, y, step_fn, loss_fn, max_norm, steps=2):
    """`steps` float64 train steps, each checked against the oracle at the GPU's own parameters before the step."""
    state = train.TrainState.create(net, params, lr=1e-3, max_grad_norm=max_norm)
    assert state.flat.dtype == torch.float64
    for buf in (state.m, state.v, state.gbuf, state.loss, state.partials):
        assert buf.dtype == torch.float64
    n = state.flat.numel()
    m, v = np.zeros(n), np.zeros(n)
    xt, yt = torch.tensor(x, dtype=torch.float64), torch.tensor(y, dtype=torch.float64)
    for t in range(1, steps + 1):
        cur = _host(state)
        p0 = state.flat.cpu().numpy()
        tp = orc.torch_params(cur, torch.float64, requires_grad=True)
        loss_ref = loss_fn(cfg, tp, xt, yt)
        loss_ref.backward()
        g_ref = np.concatenate([tp["params"][g_][n_].grad.numpy().reshape(-1) for g_, n_ in LEAVES])
        state, loss = step_fn(state, torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())
        assert loss.dtype == torch.float64 and tuple(loss.shape) == (1,)
        lr_ = float(loss_ref)
        assert abs(float(loss) - lr_) <= 1e-12 * abs(lr_), (t, float(loss), lr_)
        g_gpu = state.g.cpu().numpy()
        eg = np.abs(g_gpu - g_ref).max() / np.abs(g_ref).max()
        assert eg <= 1e-10, (t, eg)
        p_ref, m, v = orc.adam_update(p0, orc.clip_by_global_norm(g_gpu, max_norm), m, v, t, lr=1e-3)
        ep = np.abs(state.flat.cpu().numpy() - p_ref).max() / np.abs(p_ref).max()
        assert ep <= 1e-13, (t, ep)
        assert int(state.step.item()) == t
    return state


@pytest.mark.parametrize("max_norm", [1.0, 1e-3])
def test_train_step_oneint_f64(gpu, max_norm):
    cfg, params, x, *_ = load_ckpt_fixture("dnmpc_1regions_newnewdata_1stepst_l1_newarch_ksint_iq")
    params = orc.cast_params(params, np.float64)
    x = x.astype(np.float64)
    y = np.random.default_rng(2).normal(size=(x.shape[0], 2))
    net = WCRBFNet.from_config(cfg, use_float64=True)
    _check_steps(cfg, net, params, x, y, lambda s, a, b: train.train_step_oneint(s, a, b, DP),
                 lambda c, tp, xt, yt: orc.train_oneint_loss(c, tp, xt, yt, DP), max_norm)


def test_train_step_fullint_f64_on_the_float64_checkpoint(gpu):
    """dnmpc_128regions (trained with --use_float64: float64 centres / log_sigs), T = 5 (O = 10), 1280 jittered queries."""
    cfg, params, x, *_ = load_ckpt_fixture("dnmpc_128regions")
    assert params["params"]["rbf_list"]["centers"].dtype == np.float64 and cfg["out_features"] == 10
    rng = np.random.default_rng(11)
    xq = np.repeat(x.astype(np.float64), 20, axis=0) + rng.normal(size=(20 * len(x), x.shape[1])) * 0.05
    y = np.hstack([rng.normal(size=(len(xq), 5)) * 3, rng.normal(size=(len(xq), 5))])
    net = WCRBFNet.from_config(cfg, use_float64=True)
    _check_steps(cfg, net, orc.cast_params(params, np.float64), xq, y, train.train_step_fullint,
                 lambda c, tp, xt, yt: orc.train_fullint_loss(c, tp, xt, yt), 1.0)


def _frenet_case():
    cfg, params, _, *_ = load_ckpt_fixture("dnmpc_12regions_frenet_l1_bigdata")
    rng = np.random.default_rng(9)
    T = 5
    cfg = dict(cfg, out_features=2 * T)                      # the fixture net has O = 2: widen the Dense to 2T = 10
    K = cfg["num_kernels"]
    params = orc.cast_params(params, np.float64)
    params["params"]["linear"] = {"kernel": rng.normal(size=(K, 2 * T)) * 0.05, "bias": rng.normal(size=(2 * T,)) * 0.1}
    B = 300
    ns = len(cfg["activation_idx"])
    lo = np.array([min(cfg["lower_bounds"][d]) for d in range(ns)]); hi = np.array([max(cfg["upper_bounds"][d]) for d in range(ns)])
    x = rng.uniform(lo, hi, size=(B, 8))
    x[:, 7] = rng.normal(size=B) * 0.05                      # curvature of a race track: 1 - ey * cur stays away from 0
    x[:, 0] = rng.normal(size=B) * 0.2
    y = np.hstack([rng.normal(size=(B, T)) * 2, rng.normal(size=(B, T)) * 0.5])
    return cfg, params, x, y


def test_train_step_frenet_fullint_f64(gpu):
    cfg, params, x, y = _frenet_case()
    net = WCRBFNet.from_config(cfg, use_float64=True)
    _check_steps(cfg, net, params, x, y, lambda s, a, b: train.train_step_frenet_fullint(s, a, b, DP),
                 lambda c, tp, xt, yt: orc.train_frenet_fullint_loss(c, tp, xt, yt, DP), 1.0)


def test_checkpoint_resume_f64_is_bitwise(gpu, tmp_path):
    """two steps, save, restore into a fresh float64 state, two more steps == four uninterrupted steps, bit for bit."""
    cfg, params, x, y = _frenet_case()
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    net = WCRBFNet.from_config(cfg, use_float64=True)
    a = train.TrainState.create(net, params, lr=1e-3, max_grad_norm=1.0)
    for _ in range(4):
        a, la = train.train_step_frenet_fullint(a, xd, yd, DP)
    b = train.TrainState.create(net, params, lr=1e-3, max_grad_norm=1.0)
    for _ in range(2):
        b, _l = train.train_step_frenet_fullint(b, xd, yd, DP)
    path = checkpoint.save_checkpoint(str(tmp_path), b.params, 2, opt_state=b.opt_state())
    p2, step = checkpoint.restore_checkpoint(path)
    opt = checkpoint.restore_opt_state(path)
    assert step == 2 and opt[2] == 2
    for tree in (p2, opt[0], opt[1]):
        for g_, n_ in LEAVES:
            assert tree["params"][g_][n_].dtype == np.float64
    net2 = WCRBFNet.from_config(net.config())
    assert net2.use_float64
    c = train.TrainState.create(net2, p2, lr=1e-3, max_grad_norm=1.0, opt_state=opt)
    assert c.flat.dtype == torch.float64 and torch.equal(c.flat, b.flat) and torch.equal(c.m, b.m) and torch.equal(c.v, b.v)
    for _ in range(2):
        c, lc = train.train_step_frenet_fullint(c, xd, yd, DP)
    assert int(c.step.item()) == 4
    for u, w in ((c.flat, a.flat), (c.m, a.m), (c.v, a.v), (lc, la)):
        assert torch.equal(u, w)


def _epoch_case(seed=7):
    rng = np.random.default_rng(5)
    n = 3000
    inputs = rng.uniform([0, 0, 0, 0, 0, -0.6, -3.0], [7, 3.6, 3.6, 3.2, 7, 0.4, 2.5], size=(n, 7)).round(2)
    outputs = np.stack([np.sin(inputs[:, [1]]) * np.linspace(1, 2, 5), np.cos(inputs[:, [2]]) * np.linspace(0.2, 1, 5)], axis=-1)
    fx, fy = tables.mirror(inputs, outputs)
    fy = tables.flatten_outputs(fy)
    card = tables.model_card(fx, fy, [1] * 7, 128, "gaussian")
    net = WCRBFNet.from_config(card, use_float64=True)
    params = net.init(seed=1, dtype=np.float64)
    params["params"]["rbf_list"]["centers"] = rng.uniform(-4, 8, size=(1, 128, 7))
    table = tables.DeviceTable(fx, fy, seed=seed, dtype=np.float64)
    assert table.x.dtype == torch.float64 and table.y.dtype == torch.float64
    return net, params, table


def test_train_epoch_f64_over_device_table(gpu):
    """float64 DeviceTable -> train_epoch: float64 losses that decrease over the epochs; the same seed repeats bit for bit."""
    runs = []
    for _ in range(2):
        net, params, table = _epoch_case()
        state = train.TrainState.create(net, params, lr=5e-3, max_grad_norm=1.0)
        epochs = []
        for _ in range(8):
            state, losses = train.train_epoch(state, table, 1024)
            assert losses.dtype == torch.float64 and losses.shape == (5,)
            epochs.append(losses)
        runs.append((torch.cat(epochs), state.flat.clone()))
    means = [float(l.mean()) for l in runs[0][0].view(8, 5)]
    assert np.isfinite(means).all() and means[-1] < 0.95 * means[0], means
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_train_step_f64_two_ranks_unequal_shards(gpu, tmp_path):
    """Two ranks share cuda:0 over gloo with shards of 151 and 150 rows: the float64 all-reduce of [B_local * g, B_local *
    loss, B_local] gives the single-process float64 steps on the whole 301-row batch to 1e-13."""
    cfg = configs.model_card(3)
    P = orc.cast_params(configs.synth_params(3), np.float64)
    B = 301
    x = configs.synth_queries(3, B=B).astype(np.float64)
    y = np.random.default_rng(8).normal(size=(B, cfg["out_features"]))
    p = P["params"]
    inp, out = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(inp, x=x, y=y, centers=p["rbf_list"]["centers"], log_sigs=p["rbf_list"]["log_sigs"],
             kernel=p["linear"]["kernel"], bias=p["linear"]["bias"])
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", "29561", os.path.join(ROOT, "tests", "_train_two_ranks_f64.py"), inp, out],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    two = np.load(out)
    assert tuple(two["shard"]) == (0, 151) and two["flat"].dtype == np.float64
    net = WCRBFNet.from_config(cfg, use_float64=True)
    state = train.TrainState.create(net, P, lr=1e-3, max_grad_norm=1.0)
    losses = []
    for _ in range(2):
        state, loss = train.train_step_oneint(state, torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), DP)
        losses.append(float(loss))
    g1, f1 = state.g.cpu().numpy(), state.flat.cpu().numpy()
    assert np.abs(two["losses"] - np.array(losses)).max() <= 1e-13 * np.abs(losses).max(), (two["losses"], losses)
    assert np.abs(two["g"] - g1).max() <= 1e-13 * np.abs(g1).max()
    assert np.abs(two["flat"] - f1).max() <= 1e-13 * np.abs(f1).max()


def test_float32_state_stays_float32_and_f64_limits(gpu):
    cfg = dict(configs.model_card(2), num_kernels=64, out_features=2)
    net = WCRBFNet.from_config(cfg)
    state = train.TrainState.create(net, net.init(seed=0))
    for buf in (state.flat, state.m, state.v, state.gbuf, state.loss, state.partials):
        assert buf.dtype == torch.float32
    # the float64 VJP holds O <= 16: a wider float64 net's train step says so
    wide = WCRBFNet.from_config(dict(cfg, out_features=18), use_float64=True)
    st = train.TrainState.create(wide, wide.init(seed=0, dtype=np.float64))
    x = configs.synth_queries(2, B=64).astype(np.float64)
    with pytest.raises(ValueError, match="out_features <= 16"):
        train.train_step_oneint(st, x, np.zeros((64, 18)), DP)
    # the cluster model has no float64 mode
    from irbfn_amd.model import ClusterWCRBFNet
    cnet = ClusterWCRBFNet(in_features=8, out_features=10, num_kernels=8, basis_func="gaussian", num_regions=2)
    cnet.use_float64 = True
    with pytest.raises(ValueError, match="float64"):
        train.ClusterTrainState.create(cnet, {})
