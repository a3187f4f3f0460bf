"""GPU tests of K1s, the centre-lane latency kernel `rbf_fwd_clane` (irbfn_amd/csrc/rbf_forward_small.hip): what WCRBFNet.apply and
pred_step run for every batch of 64 queries or fewer, the closed-loop planner's B = 1 call among them.  The only forward that sums
across workgroups: part[NB][B][OP] and one ticket word per query in the descriptor, which the last workgroup to arrive hands back
as zero.  The cases, each at the smallest shapes at which it can go wrong:
  1. the hand-over to the other kernels at B = 65 and at a gate table of more than 256 entries (256 itself is still K1s);
  2. every compiled width: D padded to {3, 4, 7, 8}, O padded to {2, 4, 5, 8, 10, 16, 32, 64, 100, 128}, at B = 1, 3, 64;
  3. all 13 bases, one query exactly on a centre;
  4. centre counts around the 256-centre block (nb = 1, 2, 3, 64 blocks, the last one partly empty) and the geometries with
     more than one centre per lane (cpl = 2, 4), region borders inside a lane's stride;
  5. several regions (the gate evaluated per centre): regions without a range, a card without ranges, no gated coordinate;
  6. NaN and +-Inf queries;
  7. a query's result does not depend on its batch; one descriptor through batches, parameter sets and K1 in turn, on another
     stream and inside a captured graph: tickets and partial sums are clean for the next launch.
Every case states the kernel name, grid and block it expects (tests/_small_util.py restates the planner's rule) and launches into a
buffer with NaN rows behind row B.  Bounds: tests/_small_util.py."""
import functools

import numpy as np
import pytest

import _small_util as su
from test_gpu_gram_launch import _net, _queries
from irbfn_amd import _lib
from irbfn_amd.model import WCRBFNet
from oracle import c_oracle as co
from oracle import irbfn_oracle as orc

pytestmark = pytest.mark.gpu


def _run_small(net, cfg, params, x, N=None):
    """AUTO forward of x (B <= 64), asserted to be K1s with the planner's geometry for N centres."""
    B = x.shape[0]
    D, O = cfg["in_features"], cfg["out_features"]
    N = cfg["num_regions"] * cfg["num_kernels"] if N is None else N
    got, launch = su.forward_guarded(net, params, x)
    cpl, nb, grid = su.small_plan(N, B, su.padded_O(O))
    assert launch == {"kernel": su.small_name(D, O, cfg["basis_func"]), "grid": grid, "block": 256}, (launch, cpl, nb)
    return got


# ------------------------------------------------------------------------------------------------ 1. hand-over
def test_hand_over_at_64_queries(gpu):
    cfg, params = _net(7, 70, 10, "gaussian")
    x = _queries(65, 7, seed=65)
    net = WCRBFNet.from_config(cfg)
    got = _run_small(net, cfg, params, x[:64])
    su.check("K1s hand-over B=64", cfg, params, x[:64], got, net)
    other, launch = su.forward_guarded(net, params, x)
    assert launch["kernel"] and not launch["kernel"].startswith("rbf_fwd_clane<"), launch
    su.check(f"K1s hand-over B=65 ({launch['kernel'].split('<')[0]})", cfg, params, x, other, net)


def _table_net(nsplit, per_dim, ranges):
    """D = 3, `per_dim` overlapping ranges of width 1 per gated coordinate; the regions pick ranges from both ends of the table."""
    step = 3.8 / per_dim
    lows = [[-2.0 + step * i for i in range(per_dim)] for _ in range(nsplit)]
    highs = [[v + 1.0 for v in row] for row in lows]
    cfg, params = su.region_net(3, 20, 5, "gaussian", lows, highs, ranges, [4.0] * nsplit)
    x = su.region_queries(64, 3, lows, highs, ranges, [4.0] * nsplit, seed=per_dim)
    return cfg, params, x


def test_gate_table_of_256_entries_is_k1s_and_257_is_not(gpu):
    cfg, params, x = _table_net(2, 128, [(0, 127), (127, 0), (64, 63), (1, 126)])
    assert len(cfg["lower_bounds"]) * len(cfg["lower_bounds"][0]) == 256
    net = WCRBFNet.from_config(cfg)
    got = _run_small(net, cfg, params, x)
    su.check("K1s gate table 2 x 128", cfg, params, x, got, net)
    cfg, params, x = _table_net(3, 86, [(0, 85, 0), (85, 0, 85), (43, 42, 41), (1, 84, 2)])
    assert len(cfg["lower_bounds"]) * len(cfg["lower_bounds"][0]) == 258
    net = WCRBFNet.from_config(cfg)
    got, launch = su.forward_guarded(net, params, x)
    assert launch["kernel"] and not launch["kernel"].startswith("rbf_fwd_clane<"), launch
    su.check(f"K1s gate table 3 x 86 ({launch['kernel'].split('<')[0]})", cfg, params, x, got)


# ------------------------------------------------------------------------------------------------ 2. padding of D and O
PADDING = [(1, 1, "gaussian"), (2, 3, "inverse_quadratic"), (3, 2, "inverse_multiquadric"), (4, 4, "gaussian"), (5, 5, "gaussian"),
           (6, 6, "inverse_quadratic"), (7, 9, "gaussian"), (8, 10, "inverse_multiquadric"), (7, 11, "gaussian"), (8, 16, "gaussian"),
           (7, 17, "gaussian"), (3, 33, "inverse_quadratic"), (7, 65, "gaussian"), (7, 100, "gaussian"), (8, 101, "gaussian"),
           (4, 128, "gaussian")]


def test_the_padding_table_covers_every_compiled_width():
    assert {su.padded_D(D) for D, _, _ in PADDING} == {3, 4, 7, 8}
    assert {su.padded_O(O) for _, O, _ in PADDING} == set(su.COMPILED_OP)
    for _, O, _ in PADDING:                                  # at O = OP or one past the previous compiled width
        op = su.padded_O(O)
        prev = max([0] + [v for v in su.COMPILED_OP if v < op])
        assert O in (op, prev + 1), O


@pytest.mark.parametrize("D,O,basis", PADDING)
def test_padded_inputs_and_outputs(gpu, D, O, basis):
    cfg, params = _net(D, 70, O, basis)
    x = _queries(64, D, seed=100 * D + O)
    ref, scale = su.oracle(cfg, params, x)
    net = WCRBFNet.from_config(cfg)
    for B in (64, 3, 1):
        got = _run_small(net, cfg, params, x[:B])
        su.check(f"K1s pad D={D} O={O} {basis} B={B}", cfg, params, x[:B], got, net if B == 64 else None, ref[:B], scale[:B])


# ------------------------------------------------------------------------------------------------ 3. every basis
@pytest.mark.parametrize("basis", sorted(orc.BASIS))
def test_every_basis_and_a_query_on_a_centre(gpu, basis):
    cfg, params = _net(3, 33, 5, basis)
    x = _queries(5, 3, seed=33)
    x[2] = params["params"]["rbf_list"]["centers"][0, 7]
    net = WCRBFNet.from_config(cfg)
    got = _run_small(net, cfg, params, x)
    su.check(f"K1s basis {basis}", cfg, params, x, got, net)


# ------------------------------------------------------------------------------------------------ 4. centre counts
def _check_large(tag, cfg, params, x, got, net):
    """The bound of every other case; a case of 33000 centres or more that misses the element-wise bound against the oracle is
    held to the plain float32 CPU evaluation instead: err <= 4 err32 + 1e-6 scale (tests/test_gpu_parity.py::
    test_forward_trained_checkpoints), and the log says so."""
    ref, scale = su.oracle(cfg, params, x)
    N = cfg["num_regions"] * cfg["num_kernels"]
    if N >= 33000 and su.fast_err(got, ref, scale) > 1.0:
        err = np.abs(got - ref).max()
        err32 = np.abs(co.wcrbf_forward(cfg, params, x, np.float32).astype(np.float64) - ref).max()
        print(f"{tag}: NEEDED the float32-CPU rule: err/bound {su.fast_err(got, ref, scale):.3f}; max err {err:.2e}, float32 CPU {err32:.2e}")
        assert err <= 4 * err32 + 1e-6 * scale.max(), tag
        return
    su.check(tag, cfg, params, x, got, net, ref, scale)


@pytest.mark.parametrize("N,nb", [(1, 1), (255, 1), (256, 1), (257, 2), (513, 3), (16384, 64)])
def test_centre_counts_around_the_block(gpu, N, nb):
    cfg, params = _net(3, N, 2, "gaussian")
    x = _queries(64, 3, seed=N)
    net = WCRBFNet.from_config(cfg)
    for B in (64, 1):
        assert su.small_plan(N, B, 2) == (1, nb, nb * B)
        got = _run_small(net, cfg, params, x[:B])
        su.check(f"K1s N={N} B={B} nb={nb}", cfg, params, x[:B], got, net if B == 64 else None)


@pytest.mark.parametrize("N,B,cpl,nb,grid", [(16641, 64, 2, 33, 2112), (33000, 64, 4, 33, 2112), (65537, 1, 2, 129, 129), (16384, 64, 1, 64, 4096)])
def test_more_than_one_centre_per_lane(gpu, N, B, cpl, nb, grid):
    assert su.small_plan(N, B, 2) == (cpl, nb, grid)
    cfg, params = _net(3, N, 2, "gaussian")
    x = _queries(B, 3, seed=N + B)
    net = WCRBFNet.from_config(cfg)
    got, launch = su.forward_guarded(net, params, x)
    assert launch == {"kernel": su.small_name(3, 2, "gaussian"), "grid": grid, "block": 256}, launch
    _check_large(f"K1s N={N} B={B} cpl={cpl} nb={nb}", cfg, params, x, got, net)
    again, _ = su.forward_guarded(net, params, x)
    assert np.array_equal(got, again)


def test_region_borders_inside_a_lane_s_stride(gpu):
    """16641 centres as three regions of 5547: cpl = 2, so a lane's two centres are 256 apart and blocks 10 / 11 and 21 / 22 hold
    centres of two regions; the region of every centre is n / K."""
    lows, highs = [[-1.5, -0.5, 0.5]], [[-0.5, 0.5, 1.5]]
    ranges, delta = [(0,), (1,), (2,)], [3.0]
    cfg, params = su.region_net(3, 5547, 2, "gaussian", lows, highs, ranges, delta)
    x = su.region_queries(64, 3, lows, highs, ranges, delta, seed=5547)
    assert su.small_plan(16641, 64, 2) == (2, 33, 2112)
    net = WCRBFNet.from_config(cfg)
    got = _run_small(net, cfg, params, x)
    su.check("K1s N=3x5547 B=64 cpl=2", cfg, params, x, got, net)


# ------------------------------------------------------------------------------------------------ 5. several regions
R6_LOWS, R6_HIGHS = [[-1.0, 0.0], [-1.5, -0.5, 0.5]], [[0.0, 1.0], [-0.5, 0.5, 1.5]]
R6_RANGES = [(r % 2, r // 2) for r in range(6)]
R6_DELTA = [3.0, 4.0]


@functools.lru_cache(maxsize=None)
def _six_regions(rows=None):
    cfg, params = su.region_net(4, 45, 5, "inverse_quadratic", R6_LOWS, R6_HIGHS, R6_RANGES, R6_DELTA, rows=rows)
    x = su.region_queries(64, 4, R6_LOWS, R6_HIGHS, R6_RANGES, R6_DELTA, seed=6)
    x.setflags(write=False)
    return cfg, params, x


def test_the_region_queries_sit_between_regions():
    """A condition on the inputs: on the oracle's gamma, at least a quarter of the queries have two or more regions strictly
    inside (1e-3, 0.999)."""
    cfg, _, x = _six_regions()
    gam = orc.region_activation(x.astype(np.float64), 6, 2, cfg["lower_bounds"], cfg["upper_bounds"], cfg["delta"], cfg["dimension_ranges"])
    between = ((gam > 1e-3) & (gam < 0.999)).sum(axis=1) >= 2
    assert between.mean() >= 0.25, between.mean()


@pytest.mark.parametrize("rows", [None, 4, 0])
def test_six_regions_gated_per_centre(gpu, rows):
    """rows = 4: the last two regions have no range and stay 0; rows = 0: no region has one, the output is the bias."""
    cfg, params, x = _six_regions(rows)
    assert len(cfg["dimension_ranges"]) == (6 if rows is None else rows)
    net = WCRBFNet.from_config(cfg)
    for B in (64, 1):
        got = _run_small(net, cfg, params, x[:B])
        su.check(f"K1s R=6 K=45 rows={rows} B={B}", cfg, params, x[:B], got, net if B == 64 else None)
        if rows == 0:
            assert np.array_equal(got, np.broadcast_to(params["params"]["linear"]["bias"], got.shape))
    if rows == 4:                                             # the two regions without a range do contribute to the full card's output
        full, _ = su.oracle(_six_regions()[0], params, x)
        cut, _ = su.oracle(cfg, params, x)
        assert np.abs(full - cut).max() > 1e-3


def test_six_regions_without_gated_coordinates(gpu):
    cfg, params, x = _six_regions()
    cfg = dict(cfg, activation_idx=[], lower_bounds=[], upper_bounds=[], delta=[], dimension_ranges=[[] for _ in range(6)])
    net = WCRBFNet.from_config(cfg)
    got = _run_small(net, cfg, params, x)
    su.check("K1s R=6 K=45 nsplit=0", cfg, params, x, got, net)


def test_two_regions_wide_output(gpu):
    lows, highs, ranges, delta = [[-1.0, 0.0]], [[0.0, 1.0]], [(0,), (1,)], [3.0]
    cfg, params = su.region_net(4, 45, 20, "gaussian", lows, highs, ranges, delta)
    x = su.region_queries(64, 4, lows, highs, ranges, delta, seed=20)
    net = WCRBFNet.from_config(cfg)
    got = _run_small(net, cfg, params, x)
    su.check("K1s R=2 K=45 O=20", cfg, params, x, got, net)


# ------------------------------------------------------------------------------------------------ 6. non-finite queries
@pytest.mark.parametrize("basis", ["gaussian", "inverse_quadratic", "inverse_multiquadric"])
def test_nan_and_inf_queries(gpu, basis):
    cfg, params = _net(7, 70, 10, basis, nsplit=3)
    x = _queries(64, 7, seed=7)
    nan_rows, inf_rows = su.nonfinite_rows(x, gated=[0, 1, 2], ungated=[3, 4, 5, 6], rows=[3, 9, 20, 30, 31, 40, 63])
    net = WCRBFNet.from_config(cfg)
    got = _run_small(net, cfg, params, x)
    su.check_nonfinite(f"K1s non-finite {basis}", cfg, params, x, got, nan_rows, inf_rows)


# ------------------------------------------------------------------------------------------------ 7. independence and reuse
@functools.lru_cache(maxsize=None)
def _n513(seed=0):
    return _net(3, 513, 2, "gaussian", seed=seed)


def test_a_query_s_result_does_not_depend_on_its_batch(gpu):
    """N <= 16384: the same cpl and nb at every B <= 64, so the same sums in the same order."""
    for cfg, params, x in [(*_n513(), _queries(64, 3, seed=513)), _six_regions()]:
        N = cfg["num_regions"] * cfg["num_kernels"]
        assert len({su.small_plan(N, B, su.padded_O(cfg["out_features"]))[:2] for B in range(1, 65)}) == 1
        net = WCRBFNet.from_config(cfg)
        full = _run_small(net, cfg, params, x)
        other = np.array(x[40:57])
        for b in (0, 17, 63):
            one = _run_small(net, cfg, params, x[b:b + 1])
            assert np.array_equal(one[0], full[b]), b
            other[5] = x[b]
            assert np.array_equal(_run_small(net, cfg, params, other)[5], full[b]), b


def test_one_descriptor_through_batches_parameter_sets_and_k1(gpu):
    """A fixed sequence of twelve calls on one descriptor; every K1s result equals, bit for bit, the first evaluation of that
    (parameters, batch) pair on a descriptor of its own."""
    cfg, p0 = _n513()
    _, p1 = _n513(seed=1)
    P = (p0, p1)
    X = {B: _queries(B, 3, seed=900 + B) for B in (64, 1, 17, 65)}
    fresh = {(p, B): _run_small(WCRBFNet.from_config(cfg), cfg, P[p], X[B]) for p in (0, 1) for B in (64, 1, 17)}
    assert not np.array_equal(fresh[0, 64], fresh[1, 64])
    net = WCRBFNet.from_config(cfg)
    sequence = [(0, 64), (1, 1), (0, 17), (1, 64), (0, 1), (1, 17), (0, 65), (0, 64), (1, 1), (1, 64), (0, 17), (1, 17)]
    for i, (p, B) in enumerate(sequence):
        if B == 65:
            got, launch = su.forward_guarded(net, P[p], X[B])
            assert launch["kernel"] and not launch["kernel"].startswith("rbf_fwd_clane<"), launch
            su.check("K1s reuse: the B=65 call in between", cfg, P[p], X[B], got)
        else:
            assert np.array_equal(_run_small(net, cfg, P[p], X[B]), fresh[p, B]), (i, p, B)
    su.check("K1s reuse: parameters 1, B=64", cfg, p1, X[64], fresh[1, 64])


def test_another_stream_gives_the_same_bits(gpu):
    torch = gpu
    cfg, params = _n513()
    x = _queries(64, 3, seed=513)
    net = WCRBFNet.from_config(cfg)
    ref = _run_small(net, cfg, params, x)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for B in (64, 1):
            assert np.array_equal(_run_small(net, cfg, params, x[:B]), ref[:B])
    torch.cuda.current_stream().wait_stream(s)


def test_captured_graph_replays_on_overwritten_inputs(gpu):
    """A B = 1 and a B = 64 forward of one descriptor in one single-stream graph, replayed three times with the captured input
    tensors overwritten in place: each replay equals the uncaptured result for that input."""
    torch = gpu
    cfg, params = _n513()
    net = WCRBFNet.from_config(cfg)
    net.bind(params)
    inputs = [torch.from_numpy(_queries(64, 3, seed=s)).cuda() for s in (1, 2, 3)]
    plain = [(net(xi[:1]).clone(), net(xi).clone()) for xi in inputs]
    assert net.last_launch() == {"kernel": su.small_name(3, 2, "gaussian"), "grid": 3 * 64, "block": 256}
    x1, x64 = inputs[0][:1].clone(), inputs[0].clone()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            net(x1)
            net(x64)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        o1 = net(x1)
        o64 = net(x64)
    for xi, (r1, r64) in zip(inputs, plain):
        x1.copy_(xi[:1])
        x64.copy_(xi)
        o1.fill_(float("nan"))
        o64.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(o1, r1) and torch.equal(o64, r64)
    assert not torch.equal(plain[0][1], plain[1][1])
