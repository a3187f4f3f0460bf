"""GPU tests of K1g's folded distances (`gram_fold_slot`, `gram_query_operands_fold`, `gram_distances_at`,
irbfn_amd/csrc/rbf_forward_gram.h): two v_mfma_f32_16x16x32_f16 per 16 x 16 tile, the exact head sum in k 0..15 of the first.
K1g is forced and compared with the float64 oracle under the bounds the existing K1g tests assert (BOUND of
tests/test_gpu_gram_launch.py: |got - ref| over sum_k |phi_k W_k|; the relative bounds of
tests/test_gpu_gram.py::test_gram_ill_conditioned_columns where the weights are positive; the bounds of
tests/test_gpu_cluster_gram.py for the region-weighted instance).  Every case that is about the matrix-core distances asserts
from the expansion's header -- restated on the CPU from the centres as pack_all.hip's gram_header computes it; ok = 1 is what a
forced launch that is not refused says -- that every query lies inside the box, so that no wave takes the VALU distances.
A net of ONE centre has a box of zero width, which the pack refuses (ok = 0): that case asserts the refusal."""
import functools

import numpy as np
import pytest

from test_gpu_gram import _card
from test_gpu_gram_launch import BOUND, _net, _run, _terms_scale
from test_gpu_gram_setup import _forward_guarded, _inbox
from irbfn_amd import _lib, configs
from irbfn_amd.model import WCRBFNet
from oracle import irbfn_oracle as orc

pytestmark = pytest.mark.gpu

BASES = ("gaussian", "inverse_quadratic", "inverse_multiquadric")
NS = (1, 31, 32, 33, 64, 65, 330)
BS = (1, 31, 33, 95, 2048 + 5)
GEOS = ((1, 8), (1, 4), (2, 4), (2, 8), (4, 2))             # what gram_geometry can choose (rbf_forward.hip)


def _header_ex(centers):
    """Origin r and exponent ex of the box of representable queries, as gram_header: float32 midpoint of the centres' box, the
    larger of its two sides, a quarter to spare."""
    c = np.asarray(centers, np.float32).reshape(-1, centers.shape[-1])
    hi, nlo = c.max(axis=0), (-c).max(axis=0)
    r = np.float32(0.5) * hi - np.float32(0.5) * nlo
    hw = np.maximum(hi - r, r + nlo) * np.float32(1.0000005)
    ex = int(np.frexp(1.25 * float(hw.max()) * 1.0000002)[1])
    return r, ex


def _assert_on_the_matrix_cores(params, x):
    """No query of x makes its wave take the VALU distances: |x - r| < 0.999 2^ex in the kernel's own float32 arithmetic."""
    r, ex = _header_ex(params["params"]["rbf_list"]["centers"])
    assert (np.abs(np.asarray(x, np.float32) - r) < np.float32(0.999 * 2.0 ** ex)).all()


def _params(rng, D, K, O, lo, hi):
    return {"params": {"rbf_list": {"centers": rng.uniform(lo - 0.5, hi + 0.5, size=(1, K, D)).astype(np.float32),
                                    "log_sigs": rng.uniform(-0.5, 1.0, size=(1, K)).astype(np.float32)},
                       "linear": {"kernel": (rng.normal(size=(K, O)) * rng.choice([1e-2, 1.0, 30.0], size=(1, O))).astype(np.float32),
                                  "bias": rng.normal(size=(O,)).astype(np.float32)}}}


def _check(cfg, params, x, **opts):
    net = WCRBFNet.from_config(cfg)
    got, name = _run(net, params, x, **opts)
    assert name.startswith("rbf_fwd_f16gram<"), name
    p64, x64 = orc.cast_params(params, np.float64), x.astype(np.float64)
    ref, scale = orc.wcrbfnet_apply(cfg, p64, x64), _terms_scale(cfg, p64, x64) + 1e-30
    err = (np.abs(got - ref) / scale).max()
    assert err <= BOUND, (name, err)
    return got, name


@pytest.mark.parametrize("basis", BASES)
@pytest.mark.parametrize("D", [3, 4, 7, 8])
def test_every_instance_at_the_chunk_and_batch_edges(gpu, D, basis):
    """N on both sides of one and two 32-centre chunks and 330 (ten chunks and ten centres), each with the batches 1, 31, 33, 95
    (inside a wave, inside a block) in turn and with 2048 + 5.  The queries lie inside the centres' box, and that box half a unit
    inside the gate's: the gate factors stay at 1 - 5e-5 and above, so that the bound is about the RBF sums (a factor of 1e-5 and
    its float32 error belong to tests/test_gpu_gram_launch.py::test_partial_gates_and_every_instance)."""
    rng = np.random.default_rng(10 * D + len(basis))
    lo, hi = -np.ones(D) * 2, np.ones(D) * 3
    O = {3: 5, 4: 16, 7: 10, 8: 2}[D]
    for i, N in enumerate(NS):
        cfg = _card(D, N, O, basis, lo - 1.0, hi + 1.0)
        params = _params(rng, D, N, O, lo, hi)
        if N == 1:                                        # a box of zero width: refused by the pack, whatever is forced
            with pytest.raises(ValueError, match="UNSUPPORTED"):
                _run(WCRBFNet.from_config(cfg), params, rng.uniform(lo, hi, size=(33, D)).astype(np.float32))
            continue
        c = params["params"]["rbf_list"]["centers"][0]
        for B in (BS[i % 4], BS[4]):
            x = rng.uniform(c.min(axis=0), c.max(axis=0), size=(B, D)).astype(np.float32)
            _assert_on_the_matrix_cores(params, x)
            _check(cfg, params, x)


@functools.lru_cache(maxsize=None)
def _geo_case():
    cfg, params = _net(7, 330, 10, "gaussian")
    x = _inbox(2048 + 5, 7, seed=330)
    p64, x64 = orc.cast_params(params, np.float64), x.astype(np.float64)
    ref, scale = orc.wcrbfnet_apply(cfg, p64, x64), _terms_scale(cfg, p64, x64)
    for a in (x, ref, scale):
        a.setflags(write=False)
    return cfg, params, x, ref, scale


@pytest.mark.parametrize("S,QG", GEOS)
def test_every_geometry_the_planner_can_choose(gpu, S, QG):
    """N = 330 is eleven chunks: slices of 5 | 6 at S = 2 and 2 3 3 3 at S = 4.  The geometry enters no distance: the rows agree bit
    for bit with S = 1, QG = 8 wherever the slice sums are the same, i.e. at S = 1."""
    cfg, params, x, ref, scale = _geo_case()
    _assert_on_the_matrix_cores(params, x)
    net = WCRBFNet.from_config(cfg)
    got, guard, name = _forward_guarded(net, params, np.array(x), S, QG)
    assert name.startswith("rbf_fwd_f16gram<D=7,BC=0") and f"S={S},QG={QG}" in name, name
    assert (np.abs(got - ref) / scale).max() <= BOUND and np.isnan(guard).all()
    if S == 1:
        base, _, _ = _forward_guarded(net, params, np.array(x), 1, 8)
        assert np.array_equal(got, base)


@pytest.mark.parametrize("basis", BASES)
def test_queries_exactly_on_centres(gpu, basis):
    """Every head sum cancels completely (u = beta): positive weights, so |ref| is the scale -- the bounds of
    tests/test_gpu_gram.py::test_gram_ill_conditioned_columns: 1e-5 of |ref|, and float32-grade beside K1."""
    rng = np.random.default_rng(len(basis))
    D, K, O, B = 7, 330, 10, 95
    lo, hi = -np.ones(D) * 2, np.ones(D) * 3
    cfg = _card(D, K, O, basis, lo - 1.0, hi + 1.0)     # the gate's box half a unit around the centres': factors of 1 - 5e-5 and above
    params = _params(rng, D, K, O, lo, hi)
    params["params"]["linear"]["kernel"] = (np.abs(rng.normal(size=(K, O))) + 0.05).astype(np.float32)
    params["params"]["linear"]["bias"] = np.zeros(O, np.float32)
    x = np.ascontiguousarray(params["params"]["rbf_list"]["centers"][0, rng.integers(0, K, size=B)])
    _assert_on_the_matrix_cores(params, x)
    net = WCRBFNet.from_config(cfg)
    got, name = _run(net, params, x)
    assert name.startswith("rbf_fwd_f16gram<"), name
    k1, _ = _run(net, params, x, kernel=_lib.FWD_K1)
    ref = orc.wcrbfnet_apply(cfg, orc.cast_params(params, np.float64), x.astype(np.float64))
    assert (ref > 0).all()
    rel, rel_k1 = np.abs(got - ref) / ref, np.abs(k1 - ref) / ref
    assert rel.max() <= 1e-5 and rel.max() <= max(3e-6, 2.5 * rel_k1.max()), (rel.max(), rel_k1.max())


@pytest.mark.parametrize("D", [7, 8])
def test_corners_of_the_box(gpu, D):
    """Centres on the corners of [-1.5, 1.5]^D and queries on the corners of 0.998 x the box of representable queries (ex = 1:
    |x'| < 2): every coordinate's head is as large as the table lets it be and the heads of a query and the opposite centre all
    have one sign -- the largest head sums the budget of the pack admits for this net."""
    rng = np.random.default_rng(D)
    K, O, B = 64, 10, 95
    cfg = _card(D, K, O, "gaussian", -2.5 * np.ones(D), 2.5 * np.ones(D), delta=100.0)      # the gate: 1 on every query
    centers = (1.5 * rng.choice([-1.0, 1.0], size=(1, K, D))).astype(np.float32)
    centers[0, 0], centers[0, 1] = 1.5, -1.5              # both ends of every coordinate are there
    params = {"params": {"rbf_list": {"centers": centers, "log_sigs": rng.uniform(1.0, 1.6, size=(1, K)).astype(np.float32)},
                         "linear": {"kernel": (np.abs(rng.normal(size=(K, O))) + 0.1).astype(np.float32), "bias": np.zeros(O, np.float32)}}}
    r, ex = _header_ex(centers)
    assert ex == 1 and not r.any()
    x = (0.998 * 0.999 * 2.0 * rng.choice([-1.0, 1.0], size=(B, D))).astype(np.float32)
    x[0], x[1] = x[0] * 0 + np.float32(1.99), x[1] * 0 - np.float32(1.99)      # opposite to centres 1 and 0 in every coordinate
    _assert_on_the_matrix_cores(params, x)
    net = WCRBFNet.from_config(cfg)
    got, name = _run(net, params, x)
    assert name.startswith(f"rbf_fwd_f16gram<D={D}"), name
    ref = orc.wcrbfnet_apply(cfg, orc.cast_params(params, np.float64), x.astype(np.float64))
    keep = ref > 1e-3                                     # outputs that see a centre, as test_gram_narrow_widths_far_from_the_origin
    rel = (np.abs(got - ref) / np.where(keep, ref, 1.0))[keep]
    assert keep.any() and rel.max() <= 1e-5, rel.max()


@pytest.mark.parametrize("basis", ["inverse_quadratic", "inverse_multiquadric"])
def test_far_centre_outlier(gpu, basis):
    """tests/test_gpu_gram.py::test_gram_ill_conditioned_columns[outlier_far_centre] at B = 95: one centre at 60 widens the box and
    coarsens every head; the heavy column must come out to 1e-5 of |ref|.  (The gaussian net leaves the budget and is refused
    there, as that test asserts.)"""
    from test_gpu_f16 import _cond_net
    K, O, B = 512, 10, 95
    rng, cfg, centers, log_sigs = _cond_net(K, O, basis, seed=len("outlier_far_centre"))
    x = rng.uniform(0.0, 4.0, size=(B, 7)).astype(np.float32)
    W = np.abs(rng.normal(size=(K, O))) + 0.05
    centers[0, 3] = 60.0
    log_sigs[0, 3] = -0.5
    W[3, :] = 1.0e4
    params = {"params": {"rbf_list": {"centers": centers, "log_sigs": log_sigs},
                         "linear": {"kernel": W.astype(np.float32), "bias": np.zeros(O, np.float32)}}}
    _assert_on_the_matrix_cores(params, x)
    net = WCRBFNet.from_config(cfg)
    got, name = _run(net, params, x)
    assert name.startswith("rbf_fwd_f16gram<"), name
    k1, _ = _run(net, params, x, kernel=_lib.FWD_K1)
    ref = orc.wcrbfnet_apply(cfg, orc.cast_params(params, np.float64), x.astype(np.float64))
    rel, rel_k1 = np.abs(got - ref) / ref, np.abs(k1 - ref) / ref
    assert (ref > 0).all() and rel.max() <= 1e-5 and rel.max() <= max(3e-6, 2.5 * rel_k1.max()), (rel.max(), rel_k1.max())


def test_one_query_outside_the_box_takes_the_fallback_as_before(gpu):
    """One query outside the box: its wave's 32 rows come from the VALU distances, inside BOUND; every other row is the clean
    launch's, bit for bit."""
    cfg, params, x, ref, scale = _geo_case()
    B = 95
    x = np.array(x[:B])
    net = WCRBFNet.from_config(cfg)
    clean, _ = _run(net, params, x)
    xb = x.copy()
    xb[40, 2] = 50.0
    r, ex = _header_ex(params["params"]["rbf_list"]["centers"])
    assert abs(xb[40, 2] - r[2]) >= 2.0 ** ex
    got, name = _run(net, params, xb)
    assert name.startswith("rbf_fwd_f16gram<"), name
    rest = np.r_[0:32, 64:B]
    assert np.array_equal(got[rest], clean[rest])
    p64, x64 = orc.cast_params(params, np.float64), xb[32:64].astype(np.float64)
    err = np.abs(got[32:64] - orc.wcrbfnet_apply(cfg, p64, x64)) / (_terms_scale(cfg, p64, x64) + 1e-30)
    assert err.max() <= BOUND


def test_one_launch_tick(gpu):
    """rbf_tick_f16gram (the planner gives it the tick from 12288 queries): the forward followed by the stand-alone roll-out, bit
    for bit, and the controls inside BOUND of the oracle on the first and last 300 rows."""
    import torch
    from irbfn_amd import dynamics as dyn
    from irbfn_amd.planner import plan_tick
    T, mode, B = 5, _lib.ROLLOUT_ST_KS, 12288 + 33
    cfg, params = _net(7, 330, 10, "gaussian")
    rng = np.random.default_rng(B)
    x = _inbox(B, 7, seed=B)
    _assert_on_the_matrix_cores(params, x)
    st0 = np.hstack([rng.normal(size=(B, 3)) * 0.3, rng.uniform(0.5, 7.0, size=(B, 1)), rng.normal(size=(B, 3)) * 0.2]).astype(np.float32)
    mirror = (rng.random(B) < 0.5).astype(np.int32)
    net = WCRBFNet.from_config(cfg)
    xt, st, mt = torch.from_numpy(x).cuda(), torch.from_numpy(st0).cuda(), torch.from_numpy(mirror).cuda()
    ctrl, states = plan_tick(net, params, xt, mt, st, configs.DYN_PARAMS, mode=mode)
    assert net.last_launch()["kernel"].startswith("rbf_tick_f16gram<D=7,BC=0"), net.last_launch()
    u = net.apply(params, xt).clone()
    u[:, T:] = torch.where(mt[:, None] != 0, -u[:, T:], u[:, T:])
    assert torch.equal(ctrl, u)
    assert torch.equal(states, dyn.rollout_forward(mode, torch.cat([st, u], dim=1), configs.DYN_PARAMS, T))
    rows = np.r_[0:300, B - 300:B]
    p64, x64 = orc.cast_params(params, np.float64), x[rows].astype(np.float64)
    ref, scale = orc.wcrbfnet_apply(cfg, p64, x64), _terms_scale(cfg, p64, x64)
    ref[:, T:] = np.where(mirror[rows, None] != 0, -ref[:, T:], ref[:, T:])
    assert (np.abs(ctrl.cpu().numpy()[rows] - ref) / scale).max() <= BOUND


def test_one_region_weighted_instance(gpu):
    """rbf_fwd_f16gram_gamma: R = 3, K = 40 (a region's second chunk padded), the case and the bounds of
    tests/test_gpu_gram_setup.py::test_region_weights_of_the_shared_body at the planner's own geometry."""
    import torch
    from _cluster_gram_util import gamma_forward64, softmax_gamma
    from test_gpu_cluster_gram import _case, _check as _check_gamma, _fwd, _rbf
    from irbfn_amd.model import ClusterWCRBFNet
    _, cfg, params, x = _case(341, 3, 40, "inverse_quadratic", 95)
    gamma = softmax_gamma(params, x).astype(np.float32)
    ref, scale = gamma_forward64(cfg, params, x, gamma)
    stage = ClusterWCRBFNet(**cfg).stage.set_options(fwd_gamma_kernel=_lib.FWDG_K1G)
    stage.bind(_rbf(params))
    xt, gt = torch.from_numpy(x).cuda(), torch.from_numpy(gamma).cuda()
    out = _fwd(stage, xt, gt)
    assert stage.last_launch()["kernel"].startswith("rbf_fwd_f16gram_gamma<"), stage.last_launch()
    _check_gamma(out.cpu().numpy(), ref, scale, "R=3 K=40")
    assert torch.equal(out, _fwd(stage, xt, gt))


def test_one_wide_instance(gpu):
    """rbf_fwd_f16gram_wide at O = 100 (seven column tiles), N = 256, B = 2048 + 5: the bound of
    tests/test_gpu_gram.py::test_gram_wide_d8_like_the_deeper_frenet_stage (BOUND)."""
    rng = np.random.default_rng(100)
    D, K, O, B = 7, 256, 100, 2048 + 5
    lo, hi = -np.ones(D), 2.0 * np.ones(D)
    cfg = _card(D, K, O, "gaussian", lo, hi)
    params = {"params": {"rbf_list": {"centers": rng.uniform(lo - 0.5, hi + 0.5, size=(1, K, D)).astype(np.float32),
                                      "log_sigs": rng.uniform(0.0, 1.0, size=(1, K)).astype(np.float32)},
                         "linear": {"kernel": rng.normal(0, 0.3, size=(K, O)).astype(np.float32), "bias": rng.normal(size=(O,)).astype(np.float32)}}}
    x = rng.uniform(lo, hi, size=(B, D)).astype(np.float32)
    _assert_on_the_matrix_cores(params, x)
    net = WCRBFNet.from_config(cfg)
    got, name = _run(net, params, x)
    assert name.startswith("rbf_fwd_f16gram_wide<D=7"), name
    p64, x64 = orc.cast_params(params, np.float64), x.astype(np.float64)
    err = np.abs(got - orc.wcrbfnet_apply(cfg, p64, x64)) / (_terms_scale(cfg, p64, x64) + 1e-30)
    assert err.max() <= BOUND
