"""GPU tests of K1g's operand split with the 2^11 gain as one 64-bit add per value pair (split_pair_mix, rbf_forward_gram.h) in
every kernel that calls it: the narrow forward and tick (rbf_fwd_f16gram / rbf_tick_f16gram), the region-weighted instance
(rbf_fwd_f16gram_gamma) and the wide forward (rbf_fwd_f16gram_wide).  What the split can get wrong shows in the VALUES it is fed,
not in the batch, so the shapes are the smallest of each instance and the nets are chosen for their basis values: ordinary ones,
one that underflows to exactly 0 beside others at 1 (P = 2^14: the top of the split's range), rows whose every basis value lies
in 2^-27 .. 2^-20 (P below the normal f16 numbers: the lo half carries the precision), region weights 0, +-1 and -2^-20 (negative
P, P = -0).  Every case against the float64 oracle under the bound the existing K1g tests use for the same nets: |got - ref| over
sum_k |phi_k W_k| <= BOUND (tests/test_gpu_gram_launch.py); 1e-5 of |ref| with positive weights where the values are tiny
(tests/test_gpu_gram.py::test_gram_ill_conditioned_columns); the per-element bound of tests/test_gpu_cluster_gram.py for the
region-weighted instance.  The host side of the same change: tests/test_split_gain_cpu.py."""
import numpy as np
import pytest

from test_gpu_gram_launch import BOUND, _net, _run, _terms_scale
from test_gpu_gram_ring import _case
from test_gpu_gram_setup import _forward_guarded, _inbox
from irbfn_amd import _lib
from irbfn_amd.model import WCRBFNet
from oracle import irbfn_oracle as orc

pytestmark = pytest.mark.gpu


def _assert_forward(cfg, params, x, S, QG, kernel="rbf_fwd_f16gram<"):
    net = WCRBFNet.from_config(cfg)
    got, guard, name = _forward_guarded(net, params, np.array(x), S, QG)
    assert name.startswith(kernel) and (S == 0 or f"S={S},QG={QG}" in name), name
    assert np.isnan(guard).all()
    return got


@pytest.mark.parametrize("nchunks,B,S,QG", [(1, 32, 1, 8), (23, 96, 1, 8), (23, 96, 2, 4)])
def test_gaussian_net_single_chunk_and_ten_step_trips(gpu, nchunks, B, S, QG):
    """D = 7, K = 32, O = 10, B = 32: one chunk, one step of the rolled loop.  K = 32 x 23, B = 96: S = 1 walks two ten-step trips
    and three steps, S = 2 slices of 11 and 12 chunks, one trip each."""
    cfg, params, x, ref, scale = _case(nchunks, B)
    got = _assert_forward(cfg, params, x, S, QG, "rbf_fwd_f16gram<D=7,BC=0")
    err = np.abs(got - ref) / scale
    print(f"chunks={nchunks} B={B} S={S} QG={QG}: max err {err.max():.2e}")
    assert err.max() <= BOUND


@pytest.mark.parametrize("basis", ["gaussian", "inverse_quadratic", "inverse_multiquadric"])
def test_d8_instance(gpu, basis):
    cfg, params = _net(8, 96, 10, basis)
    x = _inbox(96, 8, seed=8)
    p64, x64 = orc.cast_params(params, np.float64), x.astype(np.float64)
    ref, scale = orc.wcrbfnet_apply(cfg, p64, x64), _terms_scale(cfg, p64, x64)
    got = _assert_forward(cfg, params, x, 1, 8, "rbf_fwd_f16gram<D=8")
    assert (np.abs(got - ref) / scale).max() <= BOUND


def test_a_basis_value_of_exactly_zero_beside_values_of_one(gpu):
    """Centre 0 sits in the corner (-1.2, ...) with a width of e^-0.7; for the queries near the opposite corner its basis value
    is below 2^-170, so P = 2^14 phi underflows in v_exp_f32 to exactly 0 (shown from the float64 values below).  Eight centres lie
    in the opposite corner and eight queries ON them: phi = 1, P = 2^14 exactly, the top of the split's range."""
    cfg, params = _net(7, 64, 10, "gaussian")
    rng = np.random.default_rng(3)
    c, ls = params["params"]["rbf_list"]["centers"], params["params"]["rbf_list"]["log_sigs"]
    c[0, 0], ls[0, 0] = -1.2, -0.7
    c[0, 1:9] = rng.uniform(0.9, 1.15, size=(8, 7)).astype(np.float32)
    B = 64
    x = _inbox(B, 7, seed=31)
    x[:24] = rng.uniform(0.9, 1.15, size=(24, 7)).astype(np.float32)
    x[:8] = c[0, 1:9]
    p64, x64 = orc.cast_params(params, np.float64), x.astype(np.float64)
    phi = orc.rbf_layer(x64, p64["params"]["rbf_list"]["centers"], p64["params"]["rbf_list"]["log_sigs"], "gaussian")[:, 0, :]
    assert (phi[:24, 0] < 2.0 ** -170).all() and (phi[24:, 0] > 2.0 ** -100).any()      # exactly 0 for some queries, not for others
    assert (phi[np.arange(8), 1 + np.arange(8)] == 1.0).all()
    ref, scale = orc.wcrbfnet_apply(cfg, p64, x64), _terms_scale(cfg, p64, x64)
    for S, QG in ((1, 8), (2, 4)):
        got = _assert_forward(cfg, params, x, S, QG)
        assert (np.abs(got - ref) / scale).max() <= BOUND, (S, QG)


def test_rows_whose_every_basis_value_is_tiny(gpu):
    """64 centres within 0.02 of (-0.46, ...) with one width e^-0.5, and 32 queries within 0.01 of (0.46, ...): d^2 = 16 +- 1, every
    basis value of those rows in 2^-27 .. 2^-20 (asserted on the float64 values), so P = 2^14 phi lies in 2^-13 .. 2^-6 -- hi holds
    the few bits the f16 subnormals leave and lo the rest.  Positive weights and no bias: |ref| is the error scale, 1e-5 of it the
    bound, as in test_gram_ill_conditioned_columns.  The other 32 queries sit among the centres (phi near 1)."""
    cfg, params = _net(7, 64, 10, "gaussian")
    rng = np.random.default_rng(4)
    p = params["params"]
    p["rbf_list"]["centers"][0] = (-0.46 + rng.uniform(-0.02, 0.02, size=(64, 7))).astype(np.float32)
    p["rbf_list"]["log_sigs"][0] = -0.5
    p["linear"]["kernel"] = (np.abs(rng.normal(size=(64, 10))) + 0.05).astype(np.float32)
    p["linear"]["bias"] = np.zeros(10, np.float32)
    B = 64
    x = np.empty((B, 7), np.float32)
    x[:32] = (0.46 + rng.uniform(-0.01, 0.01, size=(32, 7))).astype(np.float32)
    x[32:] = (-0.46 + rng.uniform(-0.05, 0.05, size=(32, 7))).astype(np.float32)
    p64, x64 = orc.cast_params(params, np.float64), x.astype(np.float64)
    phi = orc.rbf_layer(x64, p64["params"]["rbf_list"]["centers"], p64["params"]["rbf_list"]["log_sigs"], "gaussian")[:, 0, :]
    assert (phi[:32] > 2.0 ** -27).all() and (phi[:32] < 2.0 ** -20).all() and (phi[32:] > 0.9).all()
    ref = orc.wcrbfnet_apply(cfg, p64, x64)
    assert (ref > 0).all()
    for S, QG in ((1, 8), (2, 4)):
        got = _assert_forward(cfg, params, x, S, QG)
        rel = np.abs(got - ref) / ref
        print(f"tiny basis values S={S} QG={QG}: max rel {rel[:32].max():.2e} (tiny rows) {rel[32:].max():.2e} (rows among the centres)")
        assert rel.max() <= 1e-5, (S, QG, rel.max())


def test_region_weights_zero_plus_minus_one_and_minus_2_to_the_minus_20(gpu):
    """The region-weighted instance at R = 2, K = 32 (one chunk per region).  Rows of gamma in turn: (0, 1), (1, 0), (-1, 1),
    (-2^-20, 1), (0, 0), (1, -1), (-2^-20, -2^-20), (-1, 0): the products gamma P in front of the split are +0, negative, and --
    centre 0 of region 0 sits in the corner (-2, ...) and four queries with the weight -2^-20 near the opposite one, so that
    2^-20 x 2^14 phi is below 2^-151 (asserted on the float64 values) -- a float product that rounds to -0."""
    import torch
    from _cluster_gram_util import gamma_forward64
    from test_gpu_cluster_gram import NAME, _case as _cluster_case, _check, _fwd, _rbf
    from irbfn_amd.model import ClusterWCRBFNet
    R, K, B = 2, 32, 200
    rng, cfg, params, x = _cluster_case(220, R, K, "gaussian", B, D=7)
    rows = np.array([[0.0, 1.0], [1.0, 0.0], [-1.0, 1.0], [-2.0 ** -20, 1.0], [0.0, 0.0], [1.0, -1.0], [-2.0 ** -20, -2.0 ** -20], [-1.0, 0.0]],
                    np.float32)
    gamma = rows[np.arange(B) % len(rows)]
    params["params"]["rbf_list"]["centers"][0, 0] = -2.0
    params["params"]["rbf_list"]["log_sigs"][0, 0] = 0.0
    far = np.array([3, 6, 11, 14])
    x[far] = rng.uniform(1.85, 2.0, size=(4, 7)).astype(np.float32)
    phi = orc.rbf_layer(x[far].astype(np.float64), np.asarray(params["params"]["rbf_list"]["centers"], np.float64),
                        np.asarray(params["params"]["rbf_list"]["log_sigs"], np.float64), "gaussian")
    assert (gamma[far, 0] < 0).all() and (-gamma[far, 0] * 2.0 ** 14 * phi[:, 0, 0] < 2.0 ** -151).all()
    ref, scale = gamma_forward64(cfg, params, x, gamma)
    stage = ClusterWCRBFNet(**cfg).stage.set_options(fwd_gamma_kernel=_lib.FWDG_K1G)
    stage.bind(_rbf(params))
    xt, gt = torch.from_numpy(x).cuda(), torch.from_numpy(gamma).cuda()
    out = _fwd(stage, xt, gt)
    assert stage.last_launch()["kernel"].startswith(NAME["k1g"] + "D=7"), stage.last_launch()
    _check(out.cpu().numpy(), ref, scale, ("split gain", R, K, B))
    assert torch.equal(out, _fwd(stage, xt, gt))


def test_wide_instance_at_its_smallest_net(gpu):
    """O = 32 (two column tiles), 256 centres, B = 64: rbf_fwd_f16gram_wide, forced (the planner takes it from 2048 queries)."""
    D, K, O, B = 7, 256, 32, 64
    cfg, params = _net(D, K, O, "gaussian")
    x = _inbox(B, D, seed=32)
    got, name = _run(WCRBFNet.from_config(cfg), params, x)
    assert name.startswith("rbf_fwd_f16gram_wide<D=7"), name
    p64, x64 = orc.cast_params(params, np.float64), x.astype(np.float64)
    ref, scale = orc.wcrbfnet_apply(cfg, p64, x64), _terms_scale(cfg, p64, x64)
    assert got.shape == (B, O) and (np.abs(got - ref) / scale).max() <= BOUND


def test_tick_at_the_single_chunk_net(gpu):
    """rbf_tick_f16gram on the net of the first case (K = 32).  The planner gives the tick to K1g from 12288 queries on, so that plus
    one query group is the smallest batch that runs the kernel (asserted by name): controls and states equal, bit for bit, the
    forward followed by the sign flip and the stand-alone roll-out; the controls of the first and last 300 rows inside the bound."""
    import torch
    from irbfn_amd import configs, dynamics as dyn
    from irbfn_amd.planner import plan_tick
    T, mode, B = 5, _lib.ROLLOUT_ST_KS, 12288 + 32
    cfg, params, x, ref, scale = _case(1, B, rows=300)
    rng = np.random.default_rng(1)
    st0 = np.hstack([rng.normal(size=(B, 3)) * 0.3, rng.uniform(0.5, 7.0, size=(B, 1)), rng.normal(size=(B, 3)) * 0.2]).astype(np.float32)
    mirror = (rng.random(B) < 0.5).astype(np.int32)
    net = WCRBFNet.from_config(cfg)
    xt, st, mt = torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(st0).cuda(), torch.from_numpy(mirror).cuda()
    ctrl, states = plan_tick(net, params, xt, mt, st, configs.DYN_PARAMS, mode=mode)
    assert net.last_launch()["kernel"].startswith("rbf_tick_f16gram<D=7,BC=0"), net.last_launch()
    u = net.apply(params, xt).clone()
    assert net.last_launch()["kernel"].startswith("rbf_fwd_f16gram<D=7,BC=0"), net.last_launch()
    u[:, T:] = torch.where(mt[:, None] != 0, -u[:, T:], u[:, T:])
    assert torch.equal(ctrl, u)
    two = dyn.rollout_forward(mode, torch.cat([st, u], dim=1), configs.DYN_PARAMS, T)
    assert tuple(states.shape) == tuple(two.shape) and torch.equal(states, two)
    rows = np.r_[0:300, B - 300:B]
    want = np.where(mirror[rows, None] != 0, np.c_[ref[:, :T], -ref[:, T:]], ref)
    assert (np.abs(ctrl.cpu().numpy()[rows] - want) / scale).max() <= BOUND


def test_qg_2_and_qg_8_give_the_same_bits(gpu):
    """S = 2 at QG = 2 and QG = 8 (a row sits in another wave of another block): identical bits, which the existing suite relies on."""
    cfg, params, x, ref, scale = _case(23, 96)
    outs = {QG: _assert_forward(cfg, params, x, 2, QG, "rbf_fwd_f16gram<D=7,BC=0") for QG in (2, 8)}
    assert (np.abs(outs[8] - ref) / scale).max() <= BOUND
    assert np.array_equal(outs[2], outs[8])
