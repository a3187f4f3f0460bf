"""GPU tests of the fixed-centre and fixed-width nets (WCRBFNet(centers=, fixed_centers= / fixed_width=)): the forward on the
reduced tree, irbfn_net_vjp_frozen on every VJP path (K2g's no-centres and Dense-only instances, K2, K2h, K2r, the K2g -> K2h
hand-over) against the full VJP of the plain net and the float64 oracle, and training on the live leaves."""
import numpy as np
import pytest
import torch

from irbfn_amd import _lib, checkpoint, configs, train
from irbfn_amd.model import WCRBFNet
from oracle import c_oracle
from oracle import irbfn_oracle as orc

pytestmark = pytest.mark.gpu

MODES = {"fixed_centers": "/no_centres", "fixed_width": "/linear"}
LEAVES = (("rbf_list", "centers"), ("rbf_list", "log_sigs"), ("linear", "kernel"), ("linear", "bias"))


def _card(D, K, O, basis="gaussian", R=1, lo=-1.0, hi=2.0):
    return {"in_features": D, "out_features": O, "num_kernels": K, "basis_func": basis, "num_regions": R,
            "lower_bounds": [[lo]] * D, "upper_bounds": [[hi]] * D, "dimension_ranges": [[0] * D] * R,
            "activation_idx": list(range(D)), "delta": [20.0] * D}


def _params(rng, D, K, O, R=1):
    return {"params": {"rbf_list": {"centers": rng.uniform(-1.4, 2.4, size=(R, K, D)).astype(np.float32),
                                    "log_sigs": rng.uniform(-0.2, 0.9, size=(R, K)).astype(np.float32)},
                       "linear": {"kernel": rng.normal(size=(K, O)).astype(np.float32), "bias": rng.normal(size=(O,)).astype(np.float32)}}}


def _frozen(cfg, P, mode):
    """The frozen net of `mode` whose constants are P's centres (and widths), and its reduced tree."""
    kw = {"log_sigs": P["params"]["rbf_list"]["log_sigs"]} if mode == "fixed_width" else {}
    net = WCRBFNet(**cfg, centers=P["params"]["rbf_list"]["centers"], **{mode: True}, **kw)
    red = {"params": {"linear": P["params"]["linear"]}}
    if mode == "fixed_centers":
        red["params"]["rbf_list"] = {"log_sigs": P["params"]["rbf_list"]["log_sigs"]}
    return net, red


def _live(mode):
    return [(g, n) for g, n in LEAVES if not (n == "centers" or (mode == "fixed_width" and n == "log_sigs"))]


def _err(a, r):
    a, r = np.asarray(a, np.float64), np.asarray(r, np.float64)
    return float(np.abs(a - r).max() / (np.abs(r).max() + 1e-30))


@pytest.mark.parametrize("mode", sorted(MODES))
def test_forward_on_the_reduced_tree_equals_the_plain_net(gpu, mode):
    rng = np.random.default_rng(1)
    cfg = dict(configs.model_card(2), num_kernels=300, out_features=10)
    P = {"params": {"rbf_list": {"centers": rng.uniform(-1, 8, size=(1, 300, 7)).astype(np.float32),
                                 "log_sigs": rng.uniform(0, 2, size=(1, 300)).astype(np.float32)},
                    "linear": {"kernel": (rng.normal(size=(300, 10)) * 0.3).astype(np.float32),
                               "bias": rng.normal(size=10).astype(np.float32)}}}
    plain = WCRBFNet.from_config(cfg)
    net, red = _frozen(cfg, P, mode)
    for B in (1, 64, 4096, 65536):
        x = torch.from_numpy(configs.synth_queries(2, B=B)).cuda()
        ref = plain.apply(P, x)
        got = net.apply(red, x)
        assert net.last_launch()["kernel"] == plain.last_launch()["kernel"]
        assert torch.equal(got, ref), (mode, B)
    with pytest.raises(ValueError, match="centers"):
        net.apply(P, x)


KERNELS = {"K2": _lib.VJP_K2, "K2H": _lib.VJP_K2H, "K2G": _lib.VJP_K2G, "AUTO": _lib.VJP_AUTO}


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_vjp_live_leaves_match_the_full_vjp_and_the_oracle(gpu, mode, kernel):
    rng = np.random.default_rng(7)
    D, K, O = 8, 500, 10
    cfg = _card(D, K, O)
    P = _params(rng, D, K, O)
    plain = WCRBFNet.from_config(cfg)
    net, red = _frozen(cfg, P, mode)
    for n in (plain, net):
        n.set_options(vjp_kernel=KERNELS[kernel])
    P64 = orc.cast_params(P, np.float64)
    for B in (0, 1, 2047, 2048, 8192, 80000):
        if kernel in ("K2H", "K2G") and B < 2048:
            continue                                  # the matrix-core VJPs start at 2048 queries
        x = rng.uniform(-1.05, 2.05, size=(B, D)).astype(np.float32)
        g = (rng.normal(size=(B, O)) * 1e-2).astype(np.float32)
        xt, gt = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()
        full = plain.vjp(P, xt, gt)["params"]
        runs = [net.vjp(red, xt, gt)["params"] for _ in range(2)]
        name = net.last_launch()["kernel"]
        if kernel == "K2G":
            assert name.startswith("rbf_vjp_f16gram" + MODES[mode] + "<"), name
        got = runs[0]
        assert set(got) == {g_ for g_, _ in _live(mode)}
        ref = c_oracle.wcrbf_vjp(cfg, P64, x.astype(np.float64), g.astype(np.float64))["params"] if B else None
        for grp, n in _live(mode):
            a = got[grp][n]
            assert torch.equal(a, runs[1][grp][n]), (mode, kernel, B, n)               # bitwise repeatable
            if B == 0:
                assert not a.any()
                continue
            f = full[grp][n]
            if kernel in ("K2", "K2H"):
                assert torch.equal(a, f), (mode, kernel, B, n)                        # same computation, live leaves written
            assert _err(a.cpu(), f.cpu()) <= 2e-5, (mode, kernel, B, n, _err(a.cpu(), f.cpu()))
            assert _err(a.cpu(), ref[grp][n]) <= 2e-5, (mode, kernel, B, n, _err(a.cpu(), ref[grp][n]))
    for n in (plain, net):
        n.set_options(vjp_kernel=_lib.VJP_AUTO)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_auto_takes_the_frozen_k2g_instance_at_the_reference_size(gpu, mode):
    rng = np.random.default_rng(11)
    D, K, O, B = 8, 500, 10, 80000
    cfg = _card(D, K, O)
    P = _params(rng, D, K, O)
    net, red = _frozen(cfg, P, mode)
    x = torch.from_numpy(rng.uniform(-1.0, 2.0, size=(B, D)).astype(np.float32)).cuda()
    g = torch.from_numpy(rng.normal(size=(B, O)).astype(np.float32)).cuda()
    net.vjp(red, x, g)
    assert net.last_launch()["kernel"].startswith("rbf_vjp_f16gram" + MODES[mode] + "<D=8"), net.last_launch()
    # dW / d bias against the full K2g of the plain net: report bitwise equality, require agreement
    plain = WCRBFNet.from_config(cfg)
    full = plain.vjp(P, x, g)["params"]
    got = net.vjp(red, x, g)["params"]
    same = {n: bool(torch.equal(got["linear"][n], full["linear"][n])) for n in ("kernel", "bias")}
    print(f"{mode}: dW / dbias bitwise equal to the full K2g: {same}")
    assert same["bias"]
    assert _err(got["linear"]["kernel"].cpu(), full["linear"]["kernel"].cpu()) <= 1e-6


@pytest.mark.parametrize("mode", sorted(MODES))
def test_hand_over_to_k2h_keeps_the_live_leaves_right(gpu, mode):
    rng = np.random.default_rng(13)
    D, K, O, B = 8, 500, 10, 9000
    cfg = _card(D, K, O)
    P = _params(rng, D, K, O)
    net, red = _frozen(cfg, P, mode)
    x = rng.uniform(-1.0, 2.0, size=(B, D)).astype(np.float32)
    x[100, 2] = 300.0                                          # outside K1g's box: K2g hands the call to K2h
    g = (rng.normal(size=(B, O)) * 1e-2).astype(np.float32)
    net.set_options(vjp_kernel=_lib.VJP_K2G)
    got = net.vjp(red, torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda())["params"]
    net.set_options(vjp_kernel=_lib.VJP_AUTO)
    ref = c_oracle.wcrbf_vjp(cfg, orc.cast_params(P, np.float64), x.astype(np.float64), g.astype(np.float64))["params"]
    for grp, n in _live(mode):
        assert _err(got[grp][n].cpu(), ref[grp][n]) <= 2e-5, (mode, n)


def test_k2r_with_fixed_centres(gpu):
    from conftest import load_ckpt_fixture
    cfg, P, *_ = load_ckpt_fixture("dnmpc_128regions")
    P = orc.cast_params(P, np.float32)
    net, red = _frozen(cfg, P, "fixed_centers")
    plain = WCRBFNet.from_config(cfg)
    rng = np.random.default_rng(17)
    ns, D = len(cfg["activation_idx"]), cfg["in_features"]
    lo = np.array([min(cfg["lower_bounds"][d]) for d in range(ns)])
    hi = np.array([max(cfg["upper_bounds"][d]) for d in range(ns)])
    for B in (0, 1, 2047, 2048, 8192, 80000):
        x = np.hstack([rng.uniform(lo, hi, size=(B, ns)), rng.normal(size=(B, D - ns)) * 0.1]).astype(np.float32)
        g = rng.normal(size=(B, cfg["out_features"])).astype(np.float32)
        xt, gt = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()
        for n in (plain, net):
            n.set_options(vjp_kernel=_lib.VJP_K2R)
        full = plain.vjp(P, xt, gt)["params"]
        got = net.vjp(red, xt, gt)["params"]
        if B:
            assert net.last_launch() == plain.last_launch()
        for grp, n in _live("fixed_centers"):
            assert torch.equal(got[grp][n], full[grp][n]), (B, n)
    for n in (plain, net):
        n.set_options(vjp_kernel=_lib.VJP_AUTO)
    ref = c_oracle.wcrbf_vjp(cfg, orc.cast_params(P, np.float64), x.astype(np.float64), g.astype(np.float64))["params"]
    for grp, n in _live("fixed_centers"):
        assert _err(got[grp][n].cpu(), ref[grp][n]) <= 2e-5, n


@pytest.mark.parametrize("D", [3, 4, 7, 8])
@pytest.mark.parametrize("basis", ["gaussian", "inverse_quadratic", "inverse_multiquadric"])
@pytest.mark.parametrize("O", [10, 16])
def test_every_frozen_instance_agrees_with_the_float32_kernel(gpu, D, basis, O):
    rng = np.random.default_rng(100 * D + O)
    K, B = 200, 2100
    cfg = _card(D, K, O, basis)
    P = _params(rng, D, K, O)
    x = torch.from_numpy(rng.uniform(-1.05, 2.05, size=(B, D)).astype(np.float32)).cuda()
    g = torch.from_numpy(rng.normal(size=(B, O)).astype(np.float32)).cuda()
    plain = WCRBFNet.from_config(cfg)
    plain.set_options(vjp_kernel=_lib.VJP_K2)
    ref = plain.vjp(P, x, g)["params"]
    for mode in sorted(MODES):
        if mode == "fixed_width" and O != 10:
            continue                                          # the Dense-only instance does not depend on O
        net, red = _frozen(cfg, P, mode)
        net.set_options(vjp_kernel=_lib.VJP_K2G)
        runs = [net.vjp(red, x, g)["params"] for _ in range(2)]
        assert net.last_launch()["kernel"].startswith("rbf_vjp_f16gram" + MODES[mode]), net.last_launch()
        for grp, n in _live(mode):
            a = runs[0][grp][n]
            assert torch.isfinite(a).all() and torch.equal(a, runs[1][grp][n]), (D, basis, O, mode, n)
            assert _err(a.cpu(), ref[grp][n].cpu()) <= 2e-5, (D, basis, O, mode, n)


def _flat_live(p, live):
    return np.concatenate([np.asarray(p["params"][g][n], np.float64).reshape(-1) for g, n in live])


@pytest.mark.parametrize("mode", sorted(MODES))
def test_training_on_the_live_leaves(gpu, mode, tmp_path):
    rng = np.random.default_rng(5)
    cfg = dict(configs.model_card(2), num_kernels=300, out_features=10)
    P = {"params": {"rbf_list": {"centers": rng.uniform(-1, 8, size=(1, 300, 7)).astype(np.float32),
                                 "log_sigs": rng.uniform(0, 2, size=(1, 300)).astype(np.float32)},
                    "linear": {"kernel": (rng.normal(size=(300, 10)) * 0.3).astype(np.float32),
                               "bias": np.zeros(10, np.float32)}}}
    net, red = _frozen(cfg, P, mode)
    consts = (net.centers.copy(), None if net.log_sigs is None else net.log_sigs.copy())
    live = _live(mode)
    state = train.TrainState.create(net, red, lr=1e-3, max_grad_norm=1.0)
    n = state.flat.numel()
    assert n == sum(np.asarray(P["params"][g][k]).size for g, k in live)
    m, v = np.zeros(n), np.zeros(n)
    p64 = orc.cast_params(P, np.float64)
    xs = [configs.synth_queries(2, B=500, seed=s) for s in range(4)]
    ys = [np.hstack([rng.normal(size=(500, 5)) * 3, rng.normal(size=(500, 5))]).astype(np.float32) for _ in range(4)]
    for t in range(1, 4):
        x, y = xs[t - 1], ys[t - 1]
        tp = orc.torch_params(p64, torch.float64)
        for g, k in live:
            tp["params"][g][k].requires_grad_(True)
        loss = orc.train_fullint_loss(cfg, tp, torch.tensor(x, dtype=torch.float64), torch.tensor(y, dtype=torch.float64))
        loss.backward()
        g_ref = np.concatenate([tp["params"][g][k].grad.numpy().reshape(-1) for g, k in live])
        p_new, m, v = orc.adam_update(_flat_live(p64, live), orc.clip_by_global_norm(g_ref, 1.0), m, v, t, lr=1e-3)
        off = 0
        for g, k in live:
            cnt = p64["params"][g][k].size
            p64["params"][g][k] = p_new[off:off + cnt].reshape(p64["params"][g][k].shape)
            off += cnt
        state, l_gpu = train.train_step_fullint(state, torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())
        assert abs(float(l_gpu) - float(loss)) <= 3e-5 * abs(float(loss)), (t, float(l_gpu), float(loss))
        assert np.abs(state.g.cpu().numpy() - g_ref).max() <= 5e-4 * np.abs(g_ref).max(), t
        assert np.abs(state.flat.cpu().numpy() - p_new).max() <= 5e-5 + 1e-6 * np.abs(p_new).max(), t
    np.testing.assert_array_equal(net.centers, consts[0])
    if consts[1] is not None:
        np.testing.assert_array_equal(net.log_sigs, consts[1])
    # checkpoint -> restore -> resume: the same next step
    path = checkpoint.save_checkpoint(str(tmp_path), state.params, 3, opt_state=state.opt_state())
    params2, step = checkpoint.restore_checkpoint(path)
    mu, nu, count = checkpoint.restore_opt_state(path)
    assert step == 3 and count == 3
    resumed = train.TrainState.create(net, params2, lr=1e-3, max_grad_norm=1.0, opt_state=(mu, nu, count))
    x, y = torch.from_numpy(xs[3]).cuda(), torch.from_numpy(ys[3]).cuda()
    state, _ = train.train_step_fullint(state, x, y)
    resumed, _ = train.train_step_fullint(resumed, x, y)
    assert torch.equal(state.flat, resumed.flat)
