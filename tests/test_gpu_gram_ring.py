"""GPU tests of the chunk loop of K1g's narrow kernels (`gram_body`, rbf_forward_gram_body.h) in the one-region instances
`rbf_fwd_f16gram` / `rbf_tick_f16gram`: trips of ten steps whose ring slots are constants, taken while the wave's own slice
reaches past the trip, a rolled loop of two steps per trip for the steps that are left, and a refill address that is carried
from chunk to chunk instead of being rebuilt from the chunk number.  What can go wrong there depends on the LENGTH OF A SLICE (chunks per slice, `na`), not on the batch, so the shapes are
small nets at every slice length on both sides of one and two trips with remainders of either parity, at each S in {1, 2, 4} and
each QG in {2, 4, 8}; slices of unequal length (the shorter one walks the steps of the longer and must not stage past its end); a
wave on the VALU distances (its rolled loop) in one block with waves on the unrolled loop, whose barriers and refills it shares;
the batch edges B = 33 and 1025 query groups + 5 rows; and the bit identities the loop must keep: QG enters no sum, two runs
agree, a net gives the same bits after a launch with another step count, the one-launch tick is the forward followed by the
stand-alone roll-out.  The region-weighted instances keep the rolled loop for all their steps and are covered where they were.
Error measure and bound: those of tests/test_gpu_gram.py as tests/test_gpu_gram_launch.py states them (BOUND, imported):
|got - ref| over sum_k |phi_k W_k| against the float64 oracle.  Geometries are forced unless a case says otherwise."""
import functools

import numpy as np
import pytest

from test_gpu_gram_launch import BOUND, _net, _run, _terms_scale
from test_gpu_gram_setup import _forward_guarded, _inbox
from irbfn_amd.model import WCRBFNet
from oracle import irbfn_oracle as orc

pytestmark = pytest.mark.gpu

NA = (1, 2, 3, 4, 5, 6, 9, 10, 11, 19, 20, 21, 23)          # chunks per slice: a trip is 10 steps
GEOS = ((1, 8), (2, 4), (4, 2), (2, 8))


@functools.lru_cache(maxsize=None)
def _case(nchunks, B, rows=None):
    """D = 7, O = 10, gaussian, 32 x nchunks centres; B queries inside the expansion's box; the float64 reference and its scale on
    `rows` (default: all)."""
    cfg, params = _net(7, 32 * nchunks, 10, "gaussian")
    x = _inbox(B, 7, seed=1000 * nchunks + B)
    p64 = orc.cast_params(params, np.float64)
    x64 = x.astype(np.float64) if rows is None else x[np.r_[0:rows, B - rows:B]].astype(np.float64)
    ref, scale = orc.wcrbfnet_apply(cfg, p64, x64), _terms_scale(cfg, p64, x64)
    for a in (x, ref, scale):
        a.setflags(write=False)
    return cfg, params, x, ref, scale


def _check_forward(nchunks, S, QG, B=33):
    cfg, params, x, ref, scale = _case(nchunks, B)
    net = WCRBFNet.from_config(cfg)
    got, guard, name = _forward_guarded(net, params, np.array(x), S, QG)
    assert name.startswith("rbf_fwd_f16gram<D=7,BC=0") and f"S={S},QG={QG}" in name, name
    err = np.abs(got - ref) / scale
    print(f"chunks={nchunks} S={S} QG={QG} B={B}: max err {err.max():.2e}")
    assert err.max() <= BOUND, (nchunks, S, QG, B)
    assert np.isnan(guard).all()                                      # nothing is written behind row B
    again, guard2, _ = _forward_guarded(net, params, np.array(x), S, QG)
    assert np.array_equal(got, again) and np.isnan(guard2).all()


@pytest.mark.parametrize("S,QG", GEOS)
@pytest.mark.parametrize("na", NA)
def test_every_slice_length_around_the_trips(gpu, na, S, QG):
    """S equal slices of na chunks.  A wave takes a ten-step trip while its slice reaches past the trip: na <= 10 runs the rolled
    loop only, 11 one trip and a step, 19 and 20 one trip and 9 / 10 rolled steps (the ring wraps twice there), 21 and 23 two
    trips and 1 / 3 steps.  B = 33 is one whole and one ragged query group."""
    _check_forward(na * S, S, QG)


@pytest.mark.parametrize("nchunks,S,QG", [(13, 2, 4), (21, 4, 2), (21, 2, 8), (41, 4, 2), (39, 2, 4), (43, 4, 2)])
def test_slices_of_unequal_length(gpu, nchunks, S, QG):
    """nchunks is no multiple of S: slices of 6 | 7; 5 5 5 6; 10 | 11; 10 10 10 11; 19 | 20; 10 11 11 11 chunks.  Every wave walks the
    steps of the longest slice; the waves of a shorter one stop staging at its end, inside a trip or in the rolled loop."""
    _check_forward(nchunks, S, QG)


def test_1025_query_groups_plus_five_rows(gpu):
    """The planner's own geometry above 1024 query groups (S = 2, QG = 8: sixteen waves per block) at slices of 21 chunks: two trips
    and one step.  The float64 reference is evaluated on the first and the last 300 rows; every row must equal, bit for bit, the
    forced S = 2, QG = 4 launch (QG enters no sum), which holds each row in another wave of another block."""
    B = 32 * 1025 + 5
    cfg, params, x, ref, scale = _case(42, B, rows=300)
    net = WCRBFNet.from_config(cfg)
    got, guard, name = _forward_guarded(net, params, np.array(x), 0, 0)
    assert name.startswith("rbf_fwd_f16gram<D=7,BC=0") and "S=2,QG=8" in name, name
    assert np.isnan(guard).all() and np.isfinite(got).all()
    err = np.abs(got[np.r_[0:300, B - 300:B]] - ref) / scale
    print(f"B={B} S=2 QG=8: max err {err.max():.2e}")
    assert err.max() <= BOUND
    other, guard4, name4 = _forward_guarded(net, params, np.array(x), 2, 4)
    assert "S=2,QG=4" in name4, name4
    assert np.array_equal(got, other) and np.isnan(guard4).all()


@pytest.mark.parametrize("S,QG", [(1, 8), (2, 4), (4, 2)])
def test_a_wave_on_the_valu_distances_beside_waves_on_the_unrolled_loop(gpu, S, QG):
    """Row 3 lies outside the expansion's box, so the waves of query group 0 (one per slice) take the VALU distances in their
    rolled loop of one step per trip, in the block of the waves that run the ten-step trips: slices of 11 chunks, one trip and a
    step.  Every row inside the bound (row 3: the gate factor is 0, the output the bias); the rows of the OTHER waves are, bit for
    bit, what they are when row 3 lies inside the box."""
    B = 200
    cfg, params, x, _, _ = _case(11 * S, B)
    xo = np.array(x)
    xo[3, 2] = 1.0e3
    p64, x64 = orc.cast_params(params, np.float64), xo.astype(np.float64)
    ref, scale = orc.wcrbfnet_apply(cfg, p64, x64), _terms_scale(cfg, p64, x64)
    net = WCRBFNet.from_config(cfg)
    got, guard, name = _forward_guarded(net, params, xo, S, QG)
    assert name.startswith("rbf_fwd_f16gram<D=7,BC=0") and f"S={S},QG={QG}" in name, name
    assert np.isnan(guard).all()
    err = np.abs(got - ref) / scale
    print(f"outside the box S={S} QG={QG}: max err {err.max():.2e}")
    assert err.max() <= BOUND
    assert np.allclose(got[3], np.asarray(params["params"]["linear"]["bias"], np.float32), atol=1e-6)
    clean, _, _ = _forward_guarded(net, params, np.array(x), S, QG)
    assert np.array_equal(got[32:], clean[32:])


@pytest.mark.parametrize("nchunks", [22, 42])
def test_query_groups_per_block_enter_no_sum(gpu, nchunks):
    """S = 2 with QG = 2, 4 and 8 (one, two and -- at QG = 2 -- up to four 1 KiB pieces of a chunk image per wave): the same bits."""
    cfg, params, x, ref, scale = _case(nchunks, 300)
    net = WCRBFNet.from_config(cfg)
    outs = {}
    for QG in (2, 4, 8):
        outs[QG], guard, name = _forward_guarded(net, params, np.array(x), 2, QG)
        assert f"S=2,QG={QG}" in name and np.isnan(guard).all(), name
    assert (np.abs(outs[8] - ref) / scale).max() <= BOUND
    assert np.array_equal(outs[4], outs[8]) and np.array_equal(outs[2], outs[8])


def test_a_net_reused_after_a_launch_with_another_step_count(gpu):
    """One bound net, 42 chunks: 21 steps (S = 2), 42 steps (S = 1), 11 steps (S = 4: slices of 10 11 10 11), then 21 again."""
    import torch
    cfg, params, x, ref, scale = _case(42, 300)
    net = WCRBFNet.from_config(cfg)
    xt = torch.from_numpy(np.array(x)).cuda()
    outs = []
    for S, QG in ((2, 4), (1, 8), (4, 2), (2, 4)):
        got, name = _run(net, params, xt, fwd_f16_s=S, fwd_f16_qg=QG)
        assert name.startswith("rbf_fwd_f16gram<D=7,BC=0") and f"S={S},QG={QG}" in name, name
        outs.append(got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got))
        assert (np.abs(outs[-1] - ref) / scale).max() <= BOUND, (S, QG)
    assert np.array_equal(outs[0], outs[3])


@pytest.mark.parametrize("na", [9, 11])
def test_one_launch_tick_on_either_side_of_a_trip(gpu, na):
    """rbf_tick_f16gram (the planner gives it the tick from 12288 queries on) at S = 2, QG = 4 and slices of 9 and 11 chunks: controls
    and states equal, bit for bit, the forward followed by the sign flip and the stand-alone roll-out; the controls of the first and
    the last 300 rows inside the bound."""
    import torch
    from irbfn_amd import _lib, configs, dynamics as dyn
    from irbfn_amd.planner import plan_tick
    T, mode, B = 5, _lib.ROLLOUT_ST_KS, 12288 + 200
    cfg, params, x, ref, scale = _case(2 * na, B, rows=300)
    rng = np.random.default_rng(na)
    st0 = np.hstack([rng.normal(size=(B, 3)) * 0.3, rng.uniform(0.5, 7.0, size=(B, 1)), rng.normal(size=(B, 3)) * 0.2]).astype(np.float32)
    mirror = (rng.random(B) < 0.5).astype(np.int32)
    net = WCRBFNet.from_config(cfg)
    xt, st, mt = torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(st0).cuda(), torch.from_numpy(mirror).cuda()
    net.set_options(fwd_f16_s=2, fwd_f16_qg=4)
    try:
        ctrl, states = plan_tick(net, params, xt, mt, st, configs.DYN_PARAMS, mode=mode)
        tick_kernel = net.last_launch()["kernel"]
        assert tick_kernel.startswith("rbf_tick_f16gram<D=7,BC=0") and "S=2,QG=4" in tick_kernel, tick_kernel
        u = net.apply(params, xt).clone()
        assert net.last_launch()["kernel"].startswith("rbf_fwd_f16gram<D=7,BC=0"), net.last_launch()
    finally:
        net.set_options(fwd_f16_s=0, fwd_f16_qg=0)
    u[:, T:] = torch.where(mt[:, None] != 0, -u[:, T:], u[:, T:])
    assert torch.equal(ctrl, u)
    two = dyn.rollout_forward(mode, torch.cat([st, u], dim=1), configs.DYN_PARAMS, T)
    assert tuple(states.shape) == tuple(two.shape) and torch.equal(states, two)
    rows = np.r_[0:300, B - 300:B]
    want = np.where(mirror[rows, None] != 0, np.c_[ref[:, :T], -ref[:, T:]], ref)
    assert (np.abs(ctrl.cpu().numpy()[rows] - want) / scale).max() <= BOUND
