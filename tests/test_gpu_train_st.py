"""irbfn_train_seeds_st_fullint (train_step.hip: seeds_multistep_kernel<ST_SELECT / ST_KS, 5 / 16, float>) through its C ABI, y_pred given as data,
against the float64 statement of _st_select_util.py under the project's float32 rule (_train_step_util.ratio32 <= 1 with the
float32 statement as twin), and one train_step_st_fullint on a small net.  gy, the loss and `partials` are NaN before every call.
Rows the float64 statement flags as ambiguous (within MARGIN = 1e-5 of a kink or of the switch at V = 3) are checked for finiteness
only; at most AMBIGUOUS_CAP = 5 % of a case's rows may be."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _st_select_util as su
import _train_step_util as tu
from irbfn_amd import _lib, configs, train
from irbfn_amd import dynamics as dyn
from irbfn_amd.model import WCRBFNet, _ptr, _stream_ptr
from oracle import irbfn_oracle as orc

pytestmark = pytest.mark.gpu
HOST = np.array(configs.DYN_PARAMS, np.float32)
DP = HOST.astype(np.float64)
MODES = {"select": _lib.ROLLOUT_ST_SELECT, "ks": _lib.ROLLOUT_ST_KS}
BIG = 262144 + 257                       # the seed kernels stride from 1024 x 256 rows


def _nan(shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def call_seeds(mode, x, yp, y, tie=0.5, T=None, D=None, gy=None):
    """-> (status, gy, loss) of one call on NaN-filled gy / loss / partials"""
    lib = _lib.load()
    B, O = yp.shape
    xd, ypd, yd = _dev(x), _dev(yp), _dev(y)
    gy = _nan((B, O)) if gy is None else gy
    loss, partials = _nan((1,)), _nan((lib.irbfn_train_loss_partials(),))
    st = lib.irbfn_train_seeds_st_fullint(MODES[mode], _ptr(xd), _ptr(ypd), _ptr(yd), HOST.ctypes.data_as(C.c_void_p), float(tie),
                                          _ptr(gy), _ptr(loss), _ptr(partials), B, x.shape[1] if D is None else D,
                                          O // 2 if T is None else T, _stream_ptr(torch))
    torch.cuda.synchronize()
    return st, gy.cpu().numpy(), float(loss.item())


@functools.lru_cache(maxsize=None)
def case(mode, T, D, B):
    x, yp, y = su.seed_case(B, T, D, seed=1000 * T + 10 * D + B % 1000)
    if B >= 3:
        yp[B - 1] = y[B - 1]                                           # a row whose every L1 difference is exactly 0
    sel = mode == "select"
    loss, gy, amb = su.seeds_st_fullint(x, yp, y, DP, 0.5, sel)
    loss32, gy32, _ = su.seeds_st_fullint(x, yp, y, HOST, 0.5, sel, ft=np.float32)
    for a in (x, yp, y, gy, amb, gy32):
        a.setflags(write=False)
    return dict(x=x, yp=yp, y=y, loss=loss, gy=gy, amb=amb, loss32=loss32, gy32=gy32)


CASES = [(m, T, D, B) for m in ("select", "ks") for T, D, B in
         ((1, 7, 1), (1, 9, 257), (5, 7, 255), (5, 9, 256), (5, 7, 1000), (6, 7, 257), (6, 9, 1000), (16, 7, 256), (16, 9, 1),
          (16, 7, 1000))] + [("select", 5, 7, BIG)]


@pytest.mark.parametrize("mode,T,D,B", CASES, ids=lambda v: str(v))
def test_seeds_match_the_float64_statement(gpu, mode, T, D, B):
    c = case(mode, T, D, B)
    st, gy, loss = call_seeds(mode, c["x"], c["yp"], c["y"])
    assert st == 0 and np.isfinite(gy).all()
    amb, cap = c["amb"], tu.AMBIGUOUS_CAP
    print(f"[train_st] {mode} T={T} D={D} B={B}: ambiguous rows {100 * amb.mean():.2f} % (cap {100 * cap:.0f} %)")
    assert amb.mean() <= cap
    keep = ~amb
    if keep.any():
        e32 = np.abs(c["gy32"][keep].astype(np.float64) - c["gy"][keep]).max() / np.abs(c["gy"][keep]).max()
        assert e32 <= tu.TWIN_CAP, e32                                 # the twin took no other side of a kink on the rows kept
        r_gy = tu.ratio32(gy[keep], c["gy"][keep], c["gy32"][keep])
        r_loss = tu.ratio32([loss], [c["loss"]], [c["loss32"]])
        print(f"[train_st] {mode} T={T} D={D} B={B}: twin {e32:.2e}, gy err/bound {r_gy:.3g}, loss err/bound {r_loss:.3g}")
        assert r_gy <= 1.0 and r_loss <= 1.0, (r_gy, r_loss)
    if B >= 3:
        assert (gy[B - 1] == 0).all()                                  # y_pred == y: sgn(0) = 0 everywhere
    st2, gy2, loss2 = call_seeds(mode, c["x"], c["yp"], c["y"])
    assert st2 == 0 and loss2 == loss
    np.testing.assert_array_equal(gy2, gy)                             # repeats are bit-equal


def test_bad_arguments_and_empty_batch(gpu):
    c = case("select", 5, 7, 255)
    x, yp, y = c["x"], c["yp"], c["y"]
    z17 = np.zeros((255, 34))
    assert call_seeds("select", x, z17, z17)[0] == -1                  # T = 17
    assert call_seeds("ks", x, z17, z17)[0] == -1
    assert call_seeds("select", x, yp, y, D=6)[0] == -1                # D = 6
    assert call_seeds("select", x, yp, y, T=0)[0] == -1
    lib = _lib.load()
    loss, partials, gy = _nan((1,)), _nan((lib.irbfn_train_loss_partials(),)), _nan((4, 10))
    st = lib.irbfn_train_seeds_st_fullint(_lib.ROLLOUT_FULLINT, _ptr(gy), _ptr(gy), _ptr(gy), HOST.ctypes.data_as(C.c_void_p), 0.5,
                                          _ptr(gy), _ptr(loss), _ptr(partials), 4, 7, 5, _stream_ptr(torch))
    assert st == -1                                                    # a mode without a single-track roll-out
    for mode in MODES.values():                                        # B = 0: ok, loss 0, gy untouched, row pointers may be NULL
        st = lib.irbfn_train_seeds_st_fullint(mode, None, None, None, HOST.ctypes.data_as(C.c_void_p), 0.5, _ptr(gy), _ptr(loss),
                                              _ptr(partials), 0, 7, 5, _stream_ptr(torch))
        torch.cuda.synchronize()
        assert st == 0 and float(loss.item()) == 0.0 and torch.isnan(gy).all()
        loss.fill_(float("nan"))


def test_kinematic_single_step_is_the_one_step_rollout(gpu):
    """mode = ST_KS, T = 1: the roll-out part of the loss is taken on the final states of dynamic_st_onestep_aux, the step
    seeds_oneint differentiates -- mean|S_pred - S_act| over [0, 1, 3, 4] of the states the forward kernel gives."""
    c = case("ks", 1, 9, 257)
    x, yp, y = c["x"], c["yp"], c["y"]
    _, gy, loss = call_seeds("ks", x, yp, y)
    init = tu.oneint_init(x)
    sp = np.asarray(dyn.dynamic_st_onestep_aux(np.hstack([init, yp]).astype(np.float32), HOST), np.float64)
    sa = np.asarray(dyn.dynamic_st_onestep_aux(np.hstack([init, y]).astype(np.float32), HOST), np.float64)
    want = np.abs(yp - y).mean() + np.abs(sp[:, su.STATE_IDX] - sa[:, su.STATE_IDX]).mean()
    assert abs(loss - want) <= 2e-6 * want
    # the step's only control paths at T = 1 are v' = v + a dt and delta' = delta + sv dt: the seeds on v and delta times dt
    d = sp - sa
    ma = tu._clipgrad(yp[:, 0], -DP[10], DP[10], 0.5, np.float64)      # a predicted acceleration beyond a_max moves nothing
    ga = np.sign(yp - y) / yp.size + np.stack([ma * np.sign(d[:, 3]), np.zeros(257)], -1) * DP[8] / (257 * 4)
    keep = ~c["amb"]
    assert np.abs(gy[keep] - ga[keep]).max() <= 1e-6 * np.abs(ga).max()


def _small_net(K=64, O=10):
    """A net that is alive on _queries: centres uniform over the model card's bounds, widths 1.6 .. 4.5, predictions of order
    0.5 -- generic controls, far from the labels' grid (no row of the step's batch is ambiguous)."""
    rng = np.random.default_rng(31)
    cfg = dict(configs.model_card(2), num_kernels=K, out_features=O)
    centers = rng.uniform(np.array(configs._LO7), np.array(configs._HI7), size=(1, K, 7))
    params = {"params": {"rbf_list": {"centers": centers.astype(np.float32),
                                      "log_sigs": rng.uniform(0.5, 1.5, size=(1, K)).astype(np.float32)},
                         "linear": {"kernel": (rng.normal(size=(K, O)) * 0.3).astype(np.float32),
                                    "bias": (rng.normal(size=O) * 0.5).astype(np.float32)}}}
    return cfg, params


def _queries(B, T, seed):
    """queries inside the model card's bounds (the net's gate closes outside them) with the speed on the grid, and grid labels"""
    x = configs.synth_queries(2, B=B).astype(np.float64)
    x[:, 0] = 0.1 + 0.25 * (np.arange(B) % 27)
    return su._f32(x), su._f32(su.grid_controls(B, T, np.random.default_rng(seed)))


LEAVES = (("rbf_list", "centers"), ("rbf_list", "log_sigs"), ("linear", "kernel"), ("linear", "bias"))


def _flat(p):
    return np.concatenate([np.asarray(p["params"][g][n], np.float64).reshape(-1) for g, n in LEAVES])


@pytest.mark.parametrize("mode", ["select", "ks"])
def test_train_step_on_a_small_net(gpu, mode):
    """loss and updated flat parameters against: float64 forward -> float64 statement of the seeds -> the oracle's net VJP ->
    adam_clip, at the tolerances of test_gpu_train.test_train_step_oneint_two_steps for the same comparison."""
    cfg, params = _small_net()
    B, T = 500, 5
    x, y = _queries(B, T, seed=41)
    net = WCRBFNet.from_config(cfg)
    state = train.TrainState.create(net, params, lr=1e-3, max_grad_norm=1.0)
    p64 = orc.cast_params(params, np.float64)
    y_pred = orc.wcrbfnet_apply(cfg, p64, x)
    loss_ref, gy, amb = su.seeds_st_fullint(x, y_pred, y, DP, 0.5, mode == "select")
    g_ref = _flat(orc.wcrbfnet_vjp(cfg, p64, x, gy))
    n = g_ref.size
    p_ref, _, _ = tu.adam_clip(_flat(p64), g_ref, np.zeros(n), np.zeros(n), 1, 1e-3, 0.9, 0.999, 1e-8, 1.0)
    assert amb.mean() <= 0.01                  # the predictions are far from the labels: hardly an L1 term near its kink
    state, loss = train.train_step_st_fullint(state, _dev(x), _dev(y), HOST, mode=MODES[mode])
    g_gpu, p_gpu = state.g.cpu().numpy(), state.flat.cpu().numpy()
    print(f"[train_st] step {mode}: loss {float(loss):.6g} ref {loss_ref:.6g}; g err {np.abs(g_gpu - g_ref).max() / np.abs(g_ref).max():.2e}; "
          f"p err {np.abs(p_gpu - p_ref).max():.2e}")
    assert abs(float(loss) - loss_ref) <= 3e-5 * abs(loss_ref)
    assert np.abs(g_gpu - g_ref).max() <= 2e-4 * np.abs(g_ref).max()
    assert np.abs(p_gpu - p_ref).max() <= 2e-5 + 1e-6 * np.abs(p_ref).max()
    assert int(state.step.item()) == 1


def test_train_step_on_a_deeper_net(gpu):
    """DeeperTrainState (the golden DeeperWCRBFNet, D = 8, T = 5): the step's loss is the seed call's on the step's own forward,
    and the float64 statement's on it; its gradient is net.vjp of those seeds."""
    from conftest import load_deeper_fixture
    from irbfn_amd import distributed
    from irbfn_amd.model import DeeperWCRBFNet
    cfg, P, *_ = load_deeper_fixture()
    P = {"params": {g: {n: np.asarray(v, np.float32) for n, v in d.items()} for g, d in P["params"].items()}}
    B, T = 300, cfg["out_features"] // 2
    x, _, y = su.seed_case(B, T, 8, seed=47)
    net = DeeperWCRBFNet.from_config(cfg)
    state = train.DeeperTrainState.create(net, P, lr=1e-3, max_grad_norm=1.0)
    xd, yd = _dev(x), _dev(y)
    y_gpu = net.apply(state.params, xd).cpu().numpy()
    st, gy_gpu, loss_gpu = call_seeds("select", x, y_gpu, y)
    assert st == 0
    want = distributed.flatten_params(net.vjp(state.params, xd, _dev(gy_gpu))).cpu().numpy().astype(np.float64)
    loss_ref = su.seeds_st_fullint(x, y_gpu, y, DP, 0.5, True)[0]
    state, loss = train.train_step_st_fullint(state, xd, yd, HOST)
    assert float(loss) == loss_gpu and abs(loss_gpu - loss_ref) <= 3e-5 * abs(loss_ref)
    assert np.abs(state.g.cpu().numpy() - want).max() <= 2e-4 * np.abs(want).max()      # the step's stage VJP may be another kernel
    assert int(state.step.item()) == 1


def test_train_step_refusals(gpu):
    cfg, params = _small_net()
    x, _, y = su.seed_case(32, 5, 7, seed=43)
    f64 = train.TrainState.create(WCRBFNet.from_config(cfg, use_float64=True), params)
    assert f64.flat.dtype == torch.float64
    with pytest.raises(ValueError, match="float32"):
        train.train_step_st_fullint(f64, x, y, HOST)
    from _cluster_util import cluster_case
    from irbfn_amd.model import ClusterWCRBFNet
    _, ccfg, cparams, _ = cluster_case(3, R=3, K=8, B=8)
    cstate = train.ClusterTrainState.create(ClusterWCRBFNet(**ccfg), cparams)
    with pytest.raises(ValueError, match="cluster"):
        train.train_step_st_fullint(cstate, x, y, HOST)
    state = train.TrainState.create(WCRBFNet.from_config(cfg), params)
    with pytest.raises(ValueError):
        train.train_step_st_fullint(state, x, y, HOST, mode=_lib.ROLLOUT_FULLINT)
    with pytest.raises(ValueError):
        train.train_step_st_fullint(state, x[:, :6], y, HOST)
