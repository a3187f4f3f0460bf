"""The planning tick of DeeperWCRBFNet (``irbfn_mlp_head_tick``: head + sign flip + roll-out in one launch behind the RBF stage)
and of ClusterWCRBFNet (``irbfn_plan_tick_gamma``) through ``planner.plan_tick`` / ``plan_batch``.  The reference of the fused
kernels is the project's own separate launches, which carry the parity tests: every "equal" here is ``torch.equal``, bit for
bit (modelled on tests/test_gpu_planner.py::test_narrow_tick_in_one_launch).  The golden Deeper planner's controls are also
held against the float64 restatement under the bound of tests/test_gpu_parity.py::test_deeper_wcrbfnet_forward."""
import numpy as np
import pytest
import torch

from _cluster_util import cluster_case
from conftest import load_deeper_fixture
from irbfn_amd import _lib, configs, dynamics as dyn, planner
from irbfn_amd.model import ClusterWCRBFNet, DeeperWCRBFNet
from oracle import irbfn_oracle as orc

pytestmark = pytest.mark.gpu
MODES = {"st_ks": _lib.ROLLOUT_ST_KS, "st_select": _lib.ROLLOUT_ST_SELECT, "fullint": _lib.ROLLOUT_FULLINT,
         "frenet": _lib.ROLLOUT_FRENET_LS}


def _state0(rng, mode_name, B):
    """Initial states as in test_narrow_tick_in_one_launch."""
    if mode_name == "fullint":
        return rng.uniform(0.5, 6.0, size=(B, 1)).astype(np.float32)
    if mode_name == "frenet":
        return np.hstack([rng.normal(size=(B, 1)) * 0.2, rng.normal(size=(B, 1)) * 0.2, rng.normal(size=(B, 1)) * 0.1,
                          rng.uniform(1, 6, size=(B, 1)), rng.normal(size=(B, 3)) * 0.1, rng.normal(size=(B, 1)) * 0.05]).astype(np.float32)
    return np.hstack([rng.normal(size=(B, 3)) * 0.3, rng.uniform(0.5, 7.0, size=(B, 1)), rng.normal(size=(B, 3)) * 0.2]).astype(np.float32)


def _dynp(mode_name):
    return configs.DYN_PARAMS if mode_name != "fullint" else None


def _flip(u, mt, T):
    u = u.clone()
    u[:, T:] = torch.where(mt[:, None] != 0, -u[:, T:], u[:, T:])
    return u


def _check_tick(net, P, plain, xt, st, mt, mode_name, T):
    """The equalities of a tick against the separate launches; plain = the net's unflipped outputs [B, 2T] (device)."""
    mode, dp = MODES[mode_name], _dynp(mode_name)
    B = xt.shape[0]
    S = 5 if mode_name == "fullint" else (8 if mode_name == "frenet" else 7)
    ctrl, states = planner.plan_tick(net, P, xt, mt, st, dp, mode=mode)
    u = _flip(plain, mt, T)
    assert tuple(ctrl.shape) == (B, 2 * T) and torch.equal(ctrl, u)
    two = dyn.rollout_forward(mode, torch.cat([st, u], dim=1), dp, T)
    assert tuple(states.shape) == (B, T, S) == tuple(two.shape) and torch.equal(states, two)
    # no flags = the unflipped outputs and their roll-out
    c0, s0 = planner.plan_tick(net, P, xt, None, st, dp, mode=mode)
    plain_states = dyn.rollout_forward(mode, torch.cat([st, plain], dim=1), dp, T)
    assert torch.equal(c0, plain) and torch.equal(s0, plain_states)
    # controls only
    c1, none = planner.plan_tick(net, P, xt, mt, rollout=False)
    assert none is None and torch.equal(c1, u)
    # states only
    cn, s2 = planner.plan_batch(net, P, xt, st, dp, mode=mode, return_controls=False)
    assert cn is None and torch.equal(s2, plain_states)
    c3, s3 = planner.plan_batch(net, P, xt, st, dp, mode=mode)
    assert torch.equal(c3, plain) and torch.equal(s3, plain_states)
    return ctrl, states


def _synth_deeper(seed, D, O, K=256, basis="gaussian"):
    rng = np.random.default_rng(seed)
    cfg = {"in_features": D, "out_features": O, "num_kernels": K, "basis_func": basis, "num_regions": 1,
           "lower_bounds": [[-1.0]] * D, "upper_bounds": [[1.0]] * D, "dimension_ranges": [[0] * D],
           "activation_idx": list(range(D)), "delta": [5.0] * D}
    f = lambda *s, sc=1.0: (rng.normal(size=s) * sc).astype(np.float32)
    P = {"params": {"rbf_list": {"centers": rng.uniform(-1.2, 1.2, size=(1, K, D)).astype(np.float32),
                                 "log_sigs": rng.uniform(-0.5, 0.3, size=(1, K)).astype(np.float32)},
                    "linear_pre1": {"kernel": f(K, 64, sc=0.2), "bias": f(64, sc=0.1)},
                    "linear_pre2": {"kernel": f(64, 64, sc=0.2), "bias": f(64, sc=0.1)},
                    "linear": {"kernel": f(64, O, sc=0.2), "bias": f(O, sc=0.1)}}}
    return cfg, P


def _golden_queries(cfg, B, seed):
    ns = len(cfg["activation_idx"])
    lo = np.array([min(cfg["lower_bounds"][d]) for d in range(ns)])
    hi = np.array([max(cfg["upper_bounds"][d]) for d in range(ns)])
    return np.random.default_rng(seed).uniform(lo, hi, size=(B, cfg["in_features"])).astype(np.float32)


@pytest.mark.parametrize("B", [1, 31, 32, 33, 4099, 80000])
def test_golden_deeper_planner_tick(gpu, B):
    """IRBFNFrenetPlanner(deeper=True) on the reference's checkpoint (D = 8, O = 10: FRENET_LS, T = 5)."""
    cfg, params, *_ = load_deeper_fixture()
    T = cfg["out_features"] // 2
    assert (cfg["in_features"], cfg["out_features"]) == (8, 10)
    net = DeeperWCRBFNet.from_config(cfg)
    rng = np.random.default_rng(B)
    x = _golden_queries(cfg, B, B)
    mirror = (rng.random(B) < 0.5).astype(np.int32)
    xt, st, mt = torch.from_numpy(x).cuda(), torch.from_numpy(_state0(rng, "frenet", B)).cuda(), torch.from_numpy(mirror).cuda()
    assert _lib.load().irbfn_mlp_head_tick_needs_controls(MODES["frenet"], 10, T) == 0
    plain = net.apply(params, xt).clone()
    ctrl, _ = _check_tick(net, params, plain, xt, st, mt, "frenet", T)
    # the controls against the float64 restatement, under the bound of test_deeper_wcrbfnet_forward
    p64 = {"params": {k: {n: np.asarray(v, np.float64) for n, v in d.items()} for k, d in params["params"].items()}}
    p32 = {"params": {k: {n: np.asarray(v, np.float32) for n, v in d.items()} for k, d in params["params"].items()}}
    rows = lambda p, xs: np.concatenate([orc.deeper_wcrbfnet_apply(cfg, p, xs[i:i + 4096]) for i in range(0, B, 4096)])   # row-wise
    ref_plain = rows(p64, x.astype(np.float64))
    ref = orc.unmirror_controls(ref_plain, mirror, T)
    scale = np.abs(ref_plain).max()
    err32 = np.abs(rows(p32, x).astype(np.float64) - ref_plain).max()
    err = np.abs(ctrl.cpu().numpy() - ref).max()
    print(f"B={B}: controls err {err:.3e}, float32 restatement err {err32:.3e}, scale {scale:.3e}")
    assert err <= max(2e-5 * scale + 1e-5, 4 * err32), (err, err32, scale)


@pytest.mark.parametrize("B", [129, 2500, 70000])
@pytest.mark.parametrize("mode_name,D,T", [("st_ks", 7, 5), ("st_select", 7, 5), ("st_ks", 7, 1), ("st_ks", 7, 8),
                                           ("fullint", 7, 5), ("frenet", 8, 2)])
def test_all_four_models_on_synthetic_deeper_nets(gpu, mode_name, D, T, B):
    cfg, P = _synth_deeper(100 * T + D, D, 2 * T)
    net = DeeperWCRBFNet.from_config(cfg)
    rng = np.random.default_rng(B + T)
    x = rng.uniform(-1, 1, size=(B, D)).astype(np.float32)
    mirror = (rng.random(B) < 0.5).astype(np.int32)
    xt, st, mt = torch.from_numpy(x).cuda(), torch.from_numpy(_state0(rng, mode_name, B)).cuda(), torch.from_numpy(mirror).cuda()
    assert _lib.load().irbfn_mlp_head_tick_needs_controls(MODES[mode_name], 2 * T, T) == 0
    plain = net.apply(P, xt).clone()
    assert 0 < int(mt.sum()) < B and float(plain.abs().max()) > 0
    _check_tick(net, P, plain, xt, st, mt, mode_name, T)


def test_rows_do_not_depend_on_their_tile_or_wave(gpu):
    """Tiles are grid-strided over waves: the tick of a permuted batch is the permuted tick."""
    cfg, params, *_ = load_deeper_fixture()
    net = DeeperWCRBFNet.from_config(cfg)
    B, T = 70001, 5
    rng = np.random.default_rng(7)
    xt = torch.from_numpy(_golden_queries(cfg, B, 7)).cuda()
    st = torch.from_numpy(_state0(rng, "frenet", B)).cuda()
    mt = torch.from_numpy((rng.random(B) < 0.5).astype(np.int32)).cuda()
    perm = torch.from_numpy(rng.permutation(B)).cuda()
    c, s = planner.plan_tick(net, params, xt, mt, st, configs.DYN_PARAMS, mode=MODES["frenet"])
    cp, sp = planner.plan_tick(net, params, xt[perm].contiguous(), mt[perm].contiguous(), st[perm].contiguous(),
                               configs.DYN_PARAMS, mode=MODES["frenet"])
    assert torch.equal(cp, c[perm]) and torch.equal(sp, s[perm])


def test_wide_head_goes_through_the_controls_buffer(gpu):
    """O = 20 > 16: head forward -> flip -> split-row roll-out, the same equalities."""
    T, D, B = 10, 7, 3001
    cfg, P = _synth_deeper(20, D, 2 * T)
    net = DeeperWCRBFNet.from_config(cfg)
    assert _lib.load().irbfn_mlp_head_tick_needs_controls(MODES["st_ks"], 2 * T, T) == 1
    rng = np.random.default_rng(20)
    xt = torch.from_numpy(rng.uniform(-1, 1, size=(B, D)).astype(np.float32)).cuda()
    st = torch.from_numpy(_state0(rng, "st_ks", B)).cuda()
    mt = torch.from_numpy((rng.random(B) < 0.5).astype(np.int32)).cuda()
    _check_tick(net, P, net.apply(P, xt).clone(), xt, st, mt, "st_ks", T)


@pytest.mark.parametrize("B", [40, 5000])
@pytest.mark.parametrize("R,K", [(11, 100), (500, 10)])
def test_cluster_tick(gpu, R, K, B):
    T = 5
    rng, cfg, params, x = cluster_case(R + B, R=R, K=K, O=2 * T, B=B, D=8)
    net = ClusterWCRBFNet(**cfg)
    xt = torch.from_numpy(x).cuda()
    st = torch.from_numpy(_state0(rng, "frenet", B)).cuda()
    mt = torch.from_numpy((rng.random(B) < 0.5).astype(np.int32)).cuda()
    plain = net.apply(params, xt)[0].clone()
    _check_tick(net, params, plain, xt, st, mt, "frenet", T)
    kern = net.stage.last_launch()["kernel"]                 # the gated K1 with the roll-out in its epilogue: one launch
    assert kern.startswith("rbf_fwd_qlane<") and "GATED=1,ROLL=1" in kern, kern


def test_frenet_queries_to_deeper_tick_end_to_end(gpu):
    """build_queries_frenet -> plan_tick(DeeperWCRBFNet) equals the hand-composed chain on the same device tensors."""
    cfg, params, *_ = load_deeper_fixture()
    net = DeeperWCRBFNet.from_config(cfg)
    B, T = 777, 5
    rng = np.random.default_rng(3)
    fr = np.stack([rng.uniform(0, 100, B), rng.uniform(-0.8, 0.8, B), rng.uniform(-0.4, 0.4, B), rng.uniform(0.5, 7, B),
                   rng.uniform(-1, 1, B), rng.uniform(-2, 2, B), rng.uniform(-0.6, 0.6, B), rng.uniform(-0.5, 0.5, B)], axis=1)
    x, s0, mirror = planner.build_queries_frenet(fr, rng.uniform(0.5, 7, B))
    assert 0 < int(mirror.sum()) < B
    ctrl, states = planner.plan_tick(net, params, x, mirror, s0, configs.DYN_PARAMS, mode=MODES["frenet"])
    u = _flip(net.apply(params, x), mirror, T)
    assert torch.equal(ctrl, u)
    assert torch.equal(states, dyn.rollout_forward(MODES["frenet"], torch.cat([s0, u], dim=1), configs.DYN_PARAMS, T))
    assert bool(torch.isfinite(states).all())


def test_repeats_are_bit_identical(gpu):
    cfg, params, *_ = load_deeper_fixture()
    net = DeeperWCRBFNet.from_config(cfg)
    B = 33333
    rng = np.random.default_rng(11)
    xt = torch.from_numpy(_golden_queries(cfg, B, 11)).cuda()
    st = torch.from_numpy(_state0(rng, "frenet", B)).cuda()
    mt = torch.from_numpy((rng.random(B) < 0.5).astype(np.int32)).cuda()
    a = planner.plan_tick(net, params, xt, mt, st, configs.DYN_PARAMS, mode=MODES["frenet"])
    b = planner.plan_tick(net, params, xt, mt, st, configs.DYN_PARAMS, mode=MODES["frenet"])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_validation_messages_match_the_wcrbfnet_tick(gpu):
    cfg, P = _synth_deeper(1, 7, 10)
    net = DeeperWCRBFNet.from_config(cfg)
    xt = torch.zeros((5, 7), device="cuda")
    with pytest.raises(ValueError, match="mirror must be"):
        planner.plan_tick(net, P, xt, np.zeros(4, np.int32), rollout=False)
    with pytest.raises(ValueError, match="state0 must be"):
        planner.plan_tick(net, P, xt, None, torch.zeros((5, 8), device="cuda"), configs.DYN_PARAMS, mode=MODES["st_ks"])
    with pytest.raises(ValueError, match="x must be"):
        planner.plan_batch(net, P, xt, torch.zeros((5, 8), device="cuda"), configs.DYN_PARAMS, mode=MODES["st_ks"])
    bad = {"params": dict(P["params"], linear_pre2={"kernel": np.zeros((64, 32), np.float32), "bias": np.zeros(32, np.float32)})}
    with pytest.raises(ValueError):
        planner.plan_tick(net, bad, xt, None, rollout=False)
