"""GPU tests of what K1g's narrow kernels (`rbf_fwd_f16gram` / `rbf_tick_f16gram`) do around their chunk loop: the gate evaluated
in the prologue from region 0's row of the tables (passed by value) and parked in LDS across the steps, the chunk range cut into
slices in 32-bit arithmetic with the step count from the host, the query loads issued in one round.  Smallest shapes at which
these can go wrong: K = 160 is five chunks, so S = 2 walks slices of 2 and 3 chunks and S = 4 slices of 1, 1, 1 and 2; batches
end inside a wave and inside a block; the gate tables have several ranges per coordinate, of which region 0 picks one.
Error measure and bound of test_gpu_gram.py::test_gram_is_the_default_at_config_2...: |got - ref| over sum_k |phi_k W_k| <= 3e-6
against the float64 oracle."""
import functools

import numpy as np
import pytest

from irbfn_amd import _lib
from irbfn_amd.model import WCRBFNet
from oracle import irbfn_oracle as orc

pytestmark = pytest.mark.gpu

DEFAULTS = {"fwd_kernel": 0, "fwd_f16_s": 0, "fwd_f16_qg": 0}
BOUND = 3e-6


def _run(net, params, x, kernel=None, **opts):
    net.set_options(fwd_kernel=_lib.FWD_K1G if kernel is None else kernel, **opts)
    try:
        got = net.apply(params, x)
        name = net.last_launch()["kernel"]
    finally:
        net.set_options(**{k: DEFAULTS[k] for k in ["fwd_kernel", *opts]})
    return got, name


def _terms_scale(cfg, p64, x):
    pa = {"params": {"rbf_list": p64["params"]["rbf_list"],
                     "linear": {"kernel": np.abs(p64["params"]["linear"]["kernel"]), "bias": np.abs(p64["params"]["linear"]["bias"])}}}
    return orc.wcrbfnet_apply(cfg, pa, x)


def _net(D, K, O, basis, nsplit=None, delta=2.0, seed=0):
    """One region, box [-1, 1]^D, gate on the first nsplit coordinates.  Every gated coordinate has three ranges in the tables;
    region 0 uses range (d + 1) % 3, the other two are decoys a wrong index would pick up."""
    nsplit = D if nsplit is None else nsplit
    rng = np.random.default_rng(1000 * D + K + seed)
    lows, highs, ranges = [], [], []
    for d in range(nsplit):
        r = (d + 1) % 3
        lo_row, hi_row = [-7.0, 3.0, -30.0], [-3.0, 9.0, 30.0]
        lo_row[r], hi_row[r] = -1.0, 1.0
        lows.append(lo_row); highs.append(hi_row); ranges.append(r)
    cfg = {"in_features": D, "out_features": O, "num_kernels": K, "basis_func": basis, "num_regions": 1,
           "lower_bounds": lows, "upper_bounds": highs, "dimension_ranges": [ranges],
           "activation_idx": list(range(nsplit)), "delta": [delta] * nsplit}
    params = {"params": {"rbf_list": {"centers": rng.uniform(-1.2, 1.2, size=(1, K, D)).astype(np.float32),
                                      "log_sigs": rng.uniform(-0.5, 0.3, size=(1, K)).astype(np.float32)},
                         "linear": {"kernel": (rng.normal(size=(K, O)) * 0.2).astype(np.float32),
                                    "bias": (0.05 + np.abs(rng.normal(size=(O,))) * 0.1).astype(np.float32)}}}
    return cfg, params


def _queries(B, D, seed):
    """Rows in turn: inside the box, on its faces (one to three coordinates exactly -1 or 1), outside by 0.2 .. 1.5 (gate
    factors between 0 and 1), outside by 5 .. 6 in one coordinate (delta = 2: the factor is exactly 0)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.95, 0.95, size=(B, D))
    for b in range(B):
        kind = b % 4
        dims = rng.choice(D, size=min(D, 1 + b % 3), replace=False)
        sign = rng.choice([-1.0, 1.0], size=len(dims))
        if kind == 1:
            x[b, dims] = sign
        elif kind == 2:
            x[b, dims] = sign * (1.0 + rng.uniform(0.2, 1.5, size=len(dims)))
        elif kind == 3:
            x[b, dims[0]] = sign[0] * (1.0 + rng.uniform(5.0, 6.0))
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _k160():
    cfg, params = _net(7, 160, 10, "gaussian")
    return cfg, params, orc.cast_params(params, np.float64)


@functools.lru_cache(maxsize=None)
def _k160_reference(B):
    cfg, _, p64 = _k160()
    x = _queries(B, 7, seed=B)
    x64 = x.astype(np.float64)
    ref, scale = orc.wcrbfnet_apply(cfg, p64, x64), _terms_scale(cfg, p64, x64)
    for a in (x, ref, scale):
        a.setflags(write=False)
    return x, ref, scale


@pytest.mark.parametrize("tail", ["B=1", "B=33", "B=32QG+5"])
@pytest.mark.parametrize("S,QG", [(1, 1), (1, 8), (2, 4), (4, 2)])
def test_uneven_slices_and_ragged_batches(gpu, S, QG, tail):
    B = {"B=1": 1, "B=33": 33, "B=32QG+5": 32 * QG + 5}[tail]
    cfg, params, _ = _k160()
    x, ref, scale = _k160_reference(B)
    gam = orc.region_activation(x.astype(np.float64), 1, 7, cfg["lower_bounds"], cfg["upper_bounds"], cfg["delta"], cfg["dimension_ranges"])
    if B >= 33:
        assert gam.min() < 1e-7 and gam.max() > 0.3 and ((gam > 0.01) & (gam < 0.3)).any()      # the gate is exercised (inside the box: 0.3 .. 0.5 at delta = 2)
    net = WCRBFNet.from_config(cfg)
    got, name = _run(net, params, x, fwd_f16_s=S, fwd_f16_qg=QG)
    assert name.startswith("rbf_fwd_f16gram<D=7,BC=0") and f"S={S},QG={QG}" in name, name
    err = np.abs(got - ref) / scale
    print(f"S={S} QG={QG} B={B}: max err {err.max():.2e}")
    assert err.max() <= BOUND
    again, _ = _run(net, params, x, fwd_f16_s=S, fwd_f16_qg=QG)
    assert np.array_equal(got, again)


@pytest.mark.parametrize("D,basis,nsplit", [(7, "gaussian", 3), (3, "gaussian", 3), (4, "gaussian", 4), (8, "gaussian", 8),
                                            (7, "inverse_quadratic", 7), (7, "inverse_multiquadric", 7)])
def test_partial_gates_and_every_instance(gpu, D, basis, nsplit):
    K, B = 64, 65
    cfg, params = _net(D, K, 10, basis, nsplit=nsplit)
    x = _queries(B, D, seed=D + nsplit)
    x[5, D - 1] = 1.9                                      # nsplit < D: an ungated coordinate outside the box changes nothing in the gate
    net = WCRBFNet.from_config(cfg)
    got, name = _run(net, params, x)
    assert name.startswith(f"rbf_fwd_f16gram<D={D},"), name
    p64, x64 = orc.cast_params(params, np.float64), x.astype(np.float64)
    ref, scale = orc.wcrbfnet_apply(cfg, p64, x64), _terms_scale(cfg, p64, x64)
    err = np.abs(got - ref) / scale
    print(f"D={D} {basis} nsplit={nsplit}: max err {err.max():.2e}")
    assert err.max() <= BOUND
    again, _ = _run(net, params, x)
    assert np.array_equal(got, again)


def test_waves_on_the_valu_distances_read_the_parked_gate(gpu):
    """A row 1e3 outside the box and a row with a NaN in a gated coordinate in a batch forced onto K1g: whichever path their waves
    take (the kernel does not report it; 1e3 lies far outside the 1.25 x box the expansion represents), the gate values of those
    waves are the parked ones.  The check that carries weight is the oracle bound on the 31 neighbours of each of the two rows.
    The far row itself only says bias == bias (its gate factor is exactly 0 in every kernel: rbf_forward.h, half_tanh_plus_one),
    the NaN row that NaN comes out where K1 gives NaN."""
    cfg, params, p64 = _k160()
    S, QG = 2, 4
    B = 32 * QG + 5
    x = _queries(B, 7, seed=B).copy()
    far, nan = 37, B - 2                                   # second wave of the block; the ragged tail wave of the next block
    x[far, 2] = 1.0e3
    x[nan, 4] = np.nan
    net = WCRBFNet.from_config(cfg)
    got, name = _run(net, params, x, fwd_f16_s=S, fwd_f16_qg=QG)
    assert name.startswith("rbf_fwd_f16gram<") and f"S={S},QG={QG}" in name, name
    k1, nm = _run(net, params, x, kernel=_lib.FWD_K1)
    assert nm.startswith("rbf_fwd_qlane")
    assert np.array_equal(np.isnan(got), np.isnan(k1)) and np.isnan(got[nan]).all() and not np.isnan(np.delete(got, nan, axis=0)).any()
    assert np.array_equal(got[[far, nan]], k1[[far, nan]], equal_nan=True)
    rest = np.setdiff1d(np.arange(B), [nan])
    x64 = x[rest].astype(np.float64)
    ref, scale = orc.wcrbfnet_apply(cfg, p64, x64), _terms_scale(cfg, p64, x64)
    err = np.abs(got[rest] - ref) / scale
    print(f"wave_bad: max err {err.max():.2e}")
    assert err.max() <= BOUND
    again, _ = _run(net, params, x, fwd_f16_s=S, fwd_f16_qg=QG)
    assert np.array_equal(got, again, equal_nan=True)


@pytest.mark.parametrize("B", [100, 12288 + 100])          # 12388: the tick takes K1g from gram_preferred's batch floor (12288 queries)
def test_one_launch_tick_on_uneven_slices(gpu, B):
    """O = 10, T = 5, ROLLOUT_ST_KS on the K = 160 net: controls and states of the tick equal, bit for bit, the forward followed
    by the stand-alone roll-out (as tests/test_gpu_planner.py::test_narrow_tick_in_one_launch compares).  B = 12388 is the case that
    runs rbf_tick_f16gram (asserted by name, with slices of 2 and 3 chunks); at B = 100 the planner keeps the tick off K1g
    (gram_preferred's floor of 12288 queries), so that case only holds the same equality for whatever kernel the tick takes there."""
    import torch
    from irbfn_amd import configs, dynamics as dyn
    from irbfn_amd.planner import plan_tick
    T, mode = 5, _lib.ROLLOUT_ST_KS
    cfg, params, _ = _k160()
    rng = np.random.default_rng(B)
    x = _queries(B, 7, seed=B)
    st0 = np.hstack([rng.normal(size=(B, 3)) * 0.3, rng.uniform(0.5, 7.0, size=(B, 1)), rng.normal(size=(B, 3)) * 0.2]).astype(np.float32)
    mirror = (rng.random(B) < 0.5).astype(np.int32)
    net = WCRBFNet.from_config(cfg)
    xt, st, mt = torch.from_numpy(x).cuda(), torch.from_numpy(st0).cuda(), torch.from_numpy(mirror).cuda()
    net.set_options(fwd_f16_s=2, fwd_f16_qg=4)             # slices of 2 and 3 chunks
    try:
        ctrl, states = plan_tick(net, params, xt, mt, st, configs.DYN_PARAMS, mode=mode)
        tick_kernel = net.last_launch()["kernel"]
        if B >= 12288:
            assert tick_kernel.startswith("rbf_tick_f16gram<D=7,BC=0") and "S=2,QG=4" in tick_kernel, tick_kernel
        u = net.apply(params, xt).clone()
        fwd_kernel = net.last_launch()["kernel"]
        if B >= 12288:
            assert fwd_kernel.startswith("rbf_fwd_f16gram<") and "S=2,QG=4" in fwd_kernel, fwd_kernel
    finally:
        net.set_options(fwd_f16_s=0, fwd_f16_qg=0)
    u[:, T:] = torch.where(mt[:, None] != 0, -u[:, T:], u[:, T:])
    assert torch.equal(ctrl, u)
    two = dyn.rollout_forward(mode, torch.cat([st, u], dim=1), configs.DYN_PARAMS, T)
    assert tuple(states.shape) == tuple(two.shape) and torch.equal(states, two)
