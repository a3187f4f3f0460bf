"""GPU tests of K1g's narrow kernel body (`gram_body`, rbf_forward_gram_body.h; instances `rbf_fwd_f16gram`, `rbf_tick_f16gram`,
`rbf_fwd_f16gram_gamma`) at the edges of its launch geometries, and of the planner's rule that gives S = 2 blocks of sixteen waves
(QG = 8) above 1024 query groups (`gram_default_qg`, rbf_forward.hip) -- the one thing here that is new in the code: the forward, the
one-launch tick and the region-weighted instance at the planner's own geometry on both sides of 1024 groups.  Every other case
runs code that stands as it was and pins what it does today at shapes no other test file has, so that later work on the body's
prologue, ring refills and epilogue has them to hold on to:
  * N = 32 is ONE chunk (forced S = 2 and S = 4: the planner falls back to one slice); N = 64 at S = 2 and N = 128 at S = 4 have
    one chunk per slice, fewer than the prologue's requests, which therefore end at the slice's end; N = 96 at S = 2 walks slices
    of 1 and 2 chunks, N = 160 at S = 4 slices of 1, 1, 1, 2; N = 32 x 13 at S = 2 slices of 6 and 7 chunks -- the ring of five
    wraps and every slot is refilled;
  * B = 1, 33, 127, 128 x 3 + 17: a last block with whole query groups past B; the output buffer has guard rows behind row B,
    prefilled with NaN, which must stay NaN;
  * a query outside the expansion's box in query tile 0 only, in tile 1 only, +-Inf and NaN, at S = 1, 2, 4;
  * every compiled width D in {3, 4, 7, 8} x the three basis classes at B = 160, N = 96, gates on nsplit in {0, 1, D}
    coordinates and a gate table without ranges (the output is the bias);
  * IRBFN_OPT_GRAM_STICKY with parameters whose header exponents differ from the first bind's: the kernel reads the exponents
    from the device header, which the re-bind's pack has rewritten, whatever the host has read back;
  * the one-launch tick and the region-weighted instance at a forced S = 2, QG = 4.
Geometries are forced with fwd_f16_s / fwd_f16_qg unless a case says otherwise.
Error measure and bound: those of tests/test_gpu_gram.py as tests/test_gpu_gram_launch.py states them (BOUND, imported):
|got - ref| over sum_k |phi_k W_k| against the float64 oracle."""
import functools

import numpy as np
import pytest

from test_gpu_gram import _run, _terms_scale
from test_gpu_gram_launch import BOUND, _net
from irbfn_amd import _lib
from irbfn_amd.model import WCRBFNet, _ptr, _stream_ptr
from oracle import irbfn_oracle as orc

pytestmark = pytest.mark.gpu

BATCHES = (1, 33, 127, 128 * 3 + 17)


def _inbox(B, D, seed):
    """Queries inside the box the expansion represents (the centres of _net lie in [-1.2, 1.2]^D), so that their waves stay on the
    matrix-core distances; a third of them outside the gate's box [-1, 1]^D in some coordinate (delta = 2: factors between 0 and 1)."""
    return np.random.default_rng(seed).uniform(-1.15, 1.15, size=(B, D)).astype(np.float32)


def _forward_guarded(net, params, x, S, QG):
    """irbfn_net_forward into a buffer with a block's rows and 32 more as guard rows of NaN behind row B (QG = 0: the planner's geometry, at most eight groups per block) -> (out[B, O], guard rows, kernel name)."""
    import torch
    lib = _lib.load()
    B, guard = x.shape[0], 32 * max(QG, 8) + 32
    net.set_options(fwd_kernel=_lib.FWD_K1G, fwd_f16_s=S, fwd_f16_qg=QG)
    try:
        net.bind(params)
        xt = torch.from_numpy(x).cuda()
        buf = torch.full((B + guard, net.out_features), float("nan"), dtype=torch.float32, device=xt.device)
        st = lib.irbfn_net_forward(net._handle(torch), _ptr(xt), _ptr(buf), B, _stream_ptr(torch))
        _lib.check(st, "irbfn_net_forward")
        name = net.last_launch()["kernel"]
        out = buf.cpu().numpy()
    finally:
        net.set_options(fwd_kernel=0, fwd_f16_s=0, fwd_f16_qg=0)
    return out[:B], out[B:], name


@functools.lru_cache(maxsize=None)
def _chunk_case(K):
    cfg, params = _net(7, K, 10, "gaussian")
    p64 = orc.cast_params(params, np.float64)
    x = _inbox(max(BATCHES), 7, seed=K)
    x64 = x.astype(np.float64)
    ref, scale = orc.wcrbfnet_apply(cfg, p64, x64), _terms_scale(cfg, p64, x64)
    for a in (x, ref, scale):
        a.setflags(write=False)
    return cfg, params, x, ref, scale


@pytest.mark.parametrize("K,S,QG", [(32, 2, 4), (32, 4, 2), (64, 2, 4), (128, 4, 2), (96, 2, 4), (160, 4, 2), (32 * 13, 2, 4)])
def test_chunk_counts_batch_tails_and_guard_rows(gpu, K, S, QG):
    """The planner gives no slice an empty range: more slices than chunks are asked for in vain (gram_geometry: S > nchunks -> 1), so
    N = 32 runs as ONE slice whatever is forced -- asserted by name.  The shortest slices a launch can have are those of N = 64 at
    S = 2 and N = 128 at S = 4: one chunk each, fewer than the three requests the body makes in front of its first barrier."""
    cfg, params, x, ref, scale = _chunk_case(K)
    net = WCRBFNet.from_config(cfg)
    s_run = S if S <= K // 32 else 1
    for B in BATCHES:
        got, guard, name = _forward_guarded(net, params, np.ascontiguousarray(x[:B]), S, QG)
        assert name.startswith("rbf_fwd_f16gram<D=7,BC=0") and f"S={s_run},QG={QG}" in name, name
        err = np.abs(got - ref[:B]) / scale[:B]
        print(f"K={K} S={S} QG={QG} B={B}: max err {err.max():.2e}")
        assert err.max() <= BOUND, (K, S, QG, B)
        assert np.isnan(guard).all(), (K, S, QG, B)                  # nothing is written behind row B
        again, guard2, _ = _forward_guarded(net, params, np.ascontiguousarray(x[:B]), S, QG)
        assert np.array_equal(got, again) and np.isnan(guard2).all()


@functools.lru_cache(maxsize=None)
def _outside_case():
    """K = 160, B = 200.  Wave w holds rows 32 w .. 32 w + 31, its query tile 0 the first 16 of them."""
    cfg, params = _net(7, 160, 10, "gaussian")
    x = _inbox(200, 7, seed=200).copy()
    rows = {"tile0": 3, "tile1": 32 + 20, "+inf": 64 + 5, "-inf": 96 + 18, "nan": 128 + 9}
    x[rows["tile0"], 2] = 1.0e3
    x[rows["tile1"], 6] = -1.0e3
    x[rows["+inf"], 0] = np.inf
    x[rows["-inf"], 5] = -np.inf
    x[rows["nan"], 4] = np.nan
    fin = np.flatnonzero(np.isfinite(x).all(axis=1))
    p64, x64 = orc.cast_params(params, np.float64), x[fin].astype(np.float64)
    ref, scale = orc.wcrbfnet_apply(cfg, p64, x64), _terms_scale(cfg, p64, x64)
    for a in (x, ref, scale):
        a.setflags(write=False)
    return cfg, params, x, rows, fin, ref, scale


@pytest.mark.parametrize("S,QG", [(1, 4), (2, 4), (4, 2)])
def test_queries_outside_the_box_in_one_tile_only(gpu, S, QG):
    """A wave with one query outside the box -- in its first tile only, in its second only, infinite, NaN -- takes the VALU
    distances in every slice (the block's barriers would not meet otherwise); its 31 neighbours and the clean waves stay inside
    the oracle bound, NaN comes out exactly where the all-float32 kernel K1 gives NaN, an infinite coordinate gives the bias."""
    cfg, params, x, rows, fin, ref, scale = _outside_case()
    net = WCRBFNet.from_config(cfg)
    got, guard, name = _forward_guarded(net, params, np.array(x), S, QG)
    assert name.startswith("rbf_fwd_f16gram<") and f"S={S},QG={QG}" in name, name
    assert np.isnan(guard).all()
    err = np.abs(got[fin] - ref) / scale
    print(f"outside the box S={S} QG={QG}: max err {err.max():.2e}")
    assert err.max() <= BOUND
    k1, nm = _run(net, params, np.array(x), kernel=_lib.FWD_K1)
    assert nm.startswith("rbf_fwd_qlane")
    assert np.array_equal(np.isnan(got), np.isnan(k1)) and np.isnan(got[rows["nan"]]).all()
    assert not np.isnan(np.delete(got, rows["nan"], axis=0)).any()
    bias = np.asarray(params["params"]["linear"]["bias"], np.float32)
    for r in ("tile0", "tile1", "+inf", "-inf"):                  # delta = 2: the gate factor of these rows is 0
        assert np.allclose(got[rows[r]], bias, atol=1e-6), r


def _gate_variant(D, basis, gate):
    if gate == "no_ranges":
        cfg, params = _net(D, 96, 10, basis, nsplit=D)
        cfg = dict(cfg, dimension_ranges=[])
    else:
        cfg, params = _net(D, 96, 10, basis, nsplit={"nsplit=0": 0, "nsplit=1": 1, "nsplit=D": D}[gate])
    return cfg, params


@pytest.mark.parametrize("gate", ["nsplit=0", "nsplit=1", "nsplit=D", "no_ranges"])
@pytest.mark.parametrize("basis", ["gaussian", "inverse_quadratic", "inverse_multiquadric"])
@pytest.mark.parametrize("D", [3, 4, 7, 8])
def test_every_instance_and_gate_shape(gpu, D, basis, gate):
    B = 160
    cfg, params = _gate_variant(D, basis, gate)
    x = _inbox(B, D, seed=10 * D + len(gate))
    net = WCRBFNet.from_config(cfg)
    got, guard, name = _forward_guarded(net, params, x, 2, 4)
    assert name.startswith(f"rbf_fwd_f16gram<D={D},") and "S=2,QG=4" in name, name
    assert np.isnan(guard).all()
    p64, x64 = orc.cast_params(params, np.float64), x.astype(np.float64)
    if gate == "nsplit=0":                                        # no gated coordinate: the activation is 1 (model.py:70), the net is phi W + bias
        pp = p64["params"]
        phi = orc.rbf_layer(x64, pp["rbf_list"]["centers"], pp["rbf_list"]["log_sigs"], cfg["basis_func"])[:, 0, :]
        ref = phi @ pp["linear"]["kernel"] + pp["linear"]["bias"]
        scale = np.abs(phi) @ np.abs(pp["linear"]["kernel"]) + np.abs(pp["linear"]["bias"])
    else:
        ref, scale = orc.wcrbfnet_apply(cfg, p64, x64), _terms_scale(cfg, p64, x64)
    err = np.abs(got - ref) / scale
    print(f"D={D} {basis} {gate}: max err {err.max():.2e}")
    assert err.max() <= BOUND
    if gate == "no_ranges":                                       # model.py:70: no range, no activation
        assert np.array_equal(got, np.broadcast_to(np.asarray(params["params"]["linear"]["bias"], np.float32), got.shape))


def test_sticky_verdict_and_changed_exponents(gpu):
    """gram_sticky = 1 (training loops): the host does not read the header back after the first bind.  Parameters whose centres
    span a box 8 x larger change the header's exponents; the kernel takes them from the device header, so the second result must be
    that of the new parameters.  (tests/test_gpu_gram.py has the sticky case whose new parameters stop fitting; this is the one
    whose parameters still fit with other exponents.)"""
    cfg, params = _net(7, 96, 10, "gaussian", delta=200.0)
    cfg = dict(cfg, lower_bounds=[[-100.0 * v for v in row] for row in np.abs(cfg["lower_bounds"]).tolist()],
               upper_bounds=[[100.0 * v for v in row] for row in np.abs(cfg["upper_bounds"]).tolist()])   # both batches deep inside the box: gate 1
    rl = params["params"]["rbf_list"]
    wide = {"params": {"rbf_list": {"centers": (rl["centers"] * 8.0).astype(np.float32),
                                    "log_sigs": (rl["log_sigs"] + np.log(8.0)).astype(np.float32)},
                       "linear": params["params"]["linear"]}}
    B = 160
    x = _inbox(B, 7, seed=5)
    net = WCRBFNet.from_config(cfg)
    net.set_options(gram_sticky=1)
    try:
        for p, xs in ((params, x), (wide, (x * 8.0).astype(np.float32))):
            got, guard, name = _forward_guarded(net, p, xs, 2, 4)
            assert name.startswith("rbf_fwd_f16gram<D=7,"), name
            p64, x64 = orc.cast_params(p, np.float64), xs.astype(np.float64)
            ref, scale = orc.wcrbfnet_apply(cfg, p64, x64), _terms_scale(cfg, p64, x64)
            assert (orc.region_activation(x64, 1, 7, cfg["lower_bounds"], cfg["upper_bounds"], cfg["delta"], cfg["dimension_ranges"]) > 0.99).all()
            err = np.abs(got - ref) / scale
            print(f"sticky, box x {xs.max() / x.max():.0f}: max err {err.max():.2e}")
            assert err.max() <= BOUND and np.isnan(guard).all()
    finally:
        net.set_options(gram_sticky=0)


@pytest.mark.parametrize("B", [200, 12288 + 200])
def test_tick_of_the_shared_body(gpu, B):
    """The one-launch tick against the forward followed by the stand-alone roll-out, bit for bit.  The planner gives the tick to
    rbf_tick_f16gram from 12288 queries only (gram_preferred, rbf_forward.hip), so B = 12488 is the case that runs it (asserted by
    name); at B = 200 the same equality holds for the kernel the tick takes there."""
    import torch
    from irbfn_amd import configs, dynamics as dyn
    from irbfn_amd.planner import plan_tick
    T, mode = 5, _lib.ROLLOUT_ST_KS
    cfg, params = _net(7, 96, 10, "gaussian")
    rng = np.random.default_rng(B)
    x = _inbox(B, 7, seed=B)
    st0 = np.hstack([rng.normal(size=(B, 3)) * 0.3, rng.uniform(0.5, 7.0, size=(B, 1)), rng.normal(size=(B, 3)) * 0.2]).astype(np.float32)
    mirror = (rng.random(B) < 0.5).astype(np.int32)
    net = WCRBFNet.from_config(cfg)
    xt, st, mt = torch.from_numpy(x).cuda(), torch.from_numpy(st0).cuda(), torch.from_numpy(mirror).cuda()
    net.set_options(fwd_f16_s=2, fwd_f16_qg=4)
    try:
        ctrl, states = plan_tick(net, params, xt, mt, st, configs.DYN_PARAMS, mode=mode)
        tick_kernel = net.last_launch()["kernel"]
        if B >= 12288:
            assert tick_kernel.startswith("rbf_tick_f16gram<D=7,BC=0") and "S=2,QG=4" in tick_kernel, tick_kernel
        u = net.apply(params, xt).clone()
    finally:
        net.set_options(fwd_f16_s=0, fwd_f16_qg=0)
    u[:, T:] = torch.where(mt[:, None] != 0, -u[:, T:], u[:, T:])
    assert torch.equal(ctrl, u)
    two = dyn.rollout_forward(mode, torch.cat([st, u], dim=1), configs.DYN_PARAMS, T)
    assert tuple(states.shape) == tuple(two.shape) and torch.equal(states, two)
    x64 = x.astype(np.float64)
    p64 = orc.cast_params(params, np.float64)
    ref, scale = orc.wcrbfnet_apply(cfg, p64, x64), _terms_scale(cfg, p64, x64)
    ref[:, T:] = np.where(mirror[:, None] != 0, -ref[:, T:], ref[:, T:])
    assert (np.abs(ctrl.cpu().numpy() - ref) / scale).max() <= BOUND


def test_sixteen_wave_blocks_above_1024_query_groups(gpu):
    """The planner's own geometry at S = 2: QG = 4 up to 1024 query groups of 32, QG = 8 (one block of sixteen waves per CU) above.
    N = 512 is the smallest net the planner cuts into two slices (eight chunks per wave).  Forward against the oracle with guard
    rows at 1025 groups + 5 rows (the last block holds one whole group and a ragged one, six groups are past B); the one-launch
    tick at the same batch against the forward followed by the stand-alone roll-out, bit for bit."""
    import torch
    from irbfn_amd import configs, dynamics as dyn
    from irbfn_amd.planner import plan_tick
    cfg, params = _net(7, 512, 10, "gaussian")
    net = WCRBFNet.from_config(cfg)
    p64 = orc.cast_params(params, np.float64)
    for B, geo in ((32 * 1024, "S=2,QG=4"), (32 * 1025 + 5, "S=2,QG=8")):
        x = _inbox(B, 7, seed=B)
        got, guard, name = _forward_guarded(net, params, x, 0, 0)
        assert name.startswith("rbf_fwd_f16gram<D=7,BC=0") and geo in name, name
        x64 = x.astype(np.float64)
        ref, scale = orc.wcrbfnet_apply(cfg, p64, x64), _terms_scale(cfg, p64, x64)
        err = np.abs(got - ref) / scale
        print(f"B={B} {geo}: max err {err.max():.2e}")
        assert err.max() <= BOUND and np.isnan(guard).all()
    T, mode = 5, _lib.ROLLOUT_ST_KS
    rng = np.random.default_rng(B)
    st0 = np.hstack([rng.normal(size=(B, 3)) * 0.3, rng.uniform(0.5, 7.0, size=(B, 1)), rng.normal(size=(B, 3)) * 0.2]).astype(np.float32)
    mirror = (rng.random(B) < 0.5).astype(np.int32)
    xt, st, mt = torch.from_numpy(x).cuda(), torch.from_numpy(st0).cuda(), torch.from_numpy(mirror).cuda()
    ctrl, states = plan_tick(net, params, xt, mt, st, configs.DYN_PARAMS, mode=mode)
    tick_kernel = net.last_launch()["kernel"]
    assert tick_kernel.startswith("rbf_tick_f16gram<D=7,BC=0") and "S=2,QG=8" in tick_kernel, tick_kernel
    u = net.apply(params, xt).clone()
    assert "S=2,QG=8" in net.last_launch()["kernel"], net.last_launch()
    assert np.array_equal(u.cpu().numpy(), got)
    u[:, T:] = torch.where(mt[:, None] != 0, -u[:, T:], u[:, T:])
    assert torch.equal(ctrl, u)
    two = dyn.rollout_forward(mode, torch.cat([st, u], dim=1), configs.DYN_PARAMS, T)
    assert tuple(states.shape) == tuple(two.shape) and torch.equal(states, two)


def test_region_weights_at_the_planner_s_geometry_around_1024_groups(gpu):
    """rbf_fwd_f16gram_gamma with no geometry forced: R = 3, K = 176 is 18 chunks, enough for two slices; 1024 groups run at
    S = 2, QG = 4, 1025 groups + 5 rows at S = 2, QG = 8 (plan_gram_gamma takes gram_geometry's rule).  The float64 statement is
    evaluated on the first and the last 300 rows; the whole output must be finite and the same from run to run."""
    import torch
    from _cluster_gram_util import assert_elementwise, gamma_forward64, softmax_gamma
    from test_gpu_cluster_gram import _case, _fwd, _rbf
    from irbfn_amd.model import ClusterWCRBFNet
    Bmax = 32 * 1025 + 5
    _, cfg, params, x = _case(176, 3, 176, "gaussian", Bmax)
    gamma = softmax_gamma(params, x).astype(np.float32)
    stage = ClusterWCRBFNet(**cfg).stage.set_options(fwd_gamma_kernel=_lib.FWDG_K1G)
    stage.bind(_rbf(params))
    for B, geo in ((32 * 1024, "S=2,QG=4>"), (Bmax, "S=2,QG=8>")):
        xt, gt = torch.from_numpy(x[:B]).cuda(), torch.from_numpy(gamma[:B]).cuda()
        out = _fwd(stage, xt, gt)
        ll = stage.last_launch()
        assert ll["kernel"].startswith("rbf_fwd_f16gram_gamma<") and ll["kernel"].endswith(geo), ll
        assert torch.equal(out, _fwd(stage, xt, gt)) and bool(torch.isfinite(out).all())
        rows = np.r_[0:300, B - 300:B]
        ref, scale = gamma_forward64(cfg, params, x[rows], gamma[rows])
        assert_elementwise(out.cpu().numpy()[rows], ref, scale, f"gamma R=3 K=176 B={B} {geo}")


def test_region_weights_of_the_shared_body(gpu):
    """R = 3, K = 40 (two chunks per region, the second padded) on rbf_fwd_f16gram_gamma at S = 2, QG = 4: the weights travel by
    the same LDS-DMA requests as the chunk images.  Bounds of tests/test_gpu_cluster_gram.py."""
    import torch
    from _cluster_gram_util import gamma_forward64, softmax_gamma
    from test_gpu_cluster_gram import _case, _check, _fwd, _rbf
    from irbfn_amd.model import ClusterWCRBFNet
    _, cfg, params, x = _case(340, 3, 40, "gaussian", 333)
    gamma = softmax_gamma(params, x).astype(np.float32)
    ref, scale = gamma_forward64(cfg, params, x, gamma)
    stage = ClusterWCRBFNet(**cfg).stage.set_options(fwd_gamma_kernel=_lib.FWDG_K1G, fwd_f16_s=2, fwd_f16_qg=4)
    stage.bind(_rbf(params))
    xt, gt = torch.from_numpy(x).cuda(), torch.from_numpy(gamma).cuda()
    out = _fwd(stage, xt, gt)
    kern = stage.last_launch()["kernel"]
    assert kern.startswith("rbf_fwd_f16gram_gamma<") and kern.endswith("S=2,QG=4>"), kern
    _check(out.cpu().numpy(), ref, scale, "R=3 K=40 S=2 QG=4")
    assert torch.equal(out, _fwd(stage, xt, gt))
