"""GPU tests of K1m, the forward with Phi x W on the f32 matrix cores (`rbf_fwd_mfma`, irbfn_amd/csrc/rbf_forward_mfma.hip), forced
with fwd_kernel = FWD_K1M so that it also runs at B <= 64.  tests/test_gpu_f16.py and tests/test_gpu_gram.py hold their wide kernels
to a multiple of K1m's own error, so K1m is tested here against the float64 oracle by itself:
  1. every compiled D = 2 .. 8, NT = 1, 2, 3, 4, 7, 8 and both tile forms (QJ = 4 up to O = 16, QJ = 2 above) at batches that end
     inside and on the 16-row MFMA tile;
  2. centre counts around the 16-centre chunk, a wave with an empty chunk range;
  3. 1, 2, 8 and 16 waves per block;
  4. gates on 0, 1 and D coordinates, a card without ranges;
  5. NaN and +-Inf queries in different 16-row tiles of one block;
  6. the nets it does not take: refused when forced, another kernel under AUTO;
  7. a wide net of 1000 centres at B = 777: the reduction tile of sixteen waves does not fit the LDS and the planner halves the waves
     per block until it does (plan_mfma used to refuse the net instead).
Every case states the kernel name, grid and block it expects (tests/_small_util.py restates the planner's rule) and launches into a
buffer with NaN rows behind row B.  Bounds: tests/_small_util.py."""
import numpy as np
import pytest

import _small_util as su
from test_gpu_gram_launch import _net, _queries
from irbfn_amd import _lib
from irbfn_amd.model import WCRBFNet

pytestmark = pytest.mark.gpu


def _run_mfma(net, cfg, params, x):
    """Forward of x forced onto K1m, asserted to be `rbf_fwd_mfma` with the planner's geometry -> (out, waves per block)."""
    D, K, O = cfg["in_features"], cfg["num_kernels"], cfg["out_features"]
    NT, QJ, nw, tiles = su.mfma_plan(D, K, x.shape[0], O)
    got, launch = su.forward_guarded(net, params, x, _lib.FWD_K1M)
    assert launch == {"kernel": su.mfma_name(D, O, cfg["basis_func"]), "grid": tiles, "block": 64 * nw}, (launch, NT, QJ, nw)
    return got, nw


# ------------------------------------------------------------------------------------------------ 1. instances
@pytest.mark.parametrize("D,O,K,basis", [(2, 3, 50, "gaussian"), (3, 16, 17, "inverse_quadratic"), (4, 17, 64, "inverse_multiquadric"),
                                         (5, 33, 33, "gaussian"), (6, 48, 100, "inverse_quadratic"), (7, 64, 96, "inverse_multiquadric"),
                                         (8, 100, 70, "gaussian"), (7, 128, 300, "gaussian"), (8, 1, 16, "gaussian")])
def test_every_instance_at_batch_tails_inside_a_tile(gpu, D, O, K, basis):
    cfg, params = _net(D, K, O, basis)
    x = _queries(200, D, seed=10 * D + O)
    ref, scale = su.oracle(cfg, params, x)
    net = WCRBFNet.from_config(cfg)
    name = su.mfma_name(D, O, basis)
    assert f"NT={-(-O // 16)}," in name and f"QJ={4 if O <= 16 else 2}," in name
    for B in (1, 15, 16, 17, 63, 64, 65, 200):
        got, nw = _run_mfma(net, cfg, params, x[:B])
        su.check(f"K1m D={D} O={O} K={K} {basis} B={B} nw={nw}", cfg, params, x[:B], got, net if B == 200 else None, ref[:B], scale[:B])


# ------------------------------------------------------------------------------------------------ 2. chunk edges
@pytest.mark.parametrize("K", [1, 15, 16, 17, 31, 33, 130])
def test_centre_counts_around_the_chunk(gpu, K):
    cfg, params = _net(7, K, 10, "gaussian")
    x = _queries(100, 7, seed=K)
    if K == 130:                                              # Npad = 144: 9 chunks on 4 waves of 3 -- the fourth wave's range is empty
        assert su.mfma_plan(7, K, 100, 10) == (1, 4, 4, 2)
    net = WCRBFNet.from_config(cfg)
    got, nw = _run_mfma(net, cfg, params, x)
    su.check(f"K1m K={K} B=100 nw={nw}", cfg, params, x, got, net)


# ------------------------------------------------------------------------------------------------ 3. waves per block
def _inbox(B, D, seed):
    """Vectorised queries for the large batches: a third of them outside the gate's box [-1, 1]^D in some coordinate."""
    return np.random.default_rng(seed).uniform(-1.15, 1.15, size=(B, D)).astype(np.float32)


@pytest.mark.parametrize("O,B,nw", [(10, 100, 16), (10, 262144 + 3, 2), (10, 524288 + 3, 1), (40, 8192 + 5, 8), (40, 65536 + 3, 1)])
def test_waves_per_block(gpu, O, B, nw):
    """K = 512 is 32 chunks, so the chunk count does not cap the waves per block.  The large batches are compared with the oracle
    on their first 200 rows, their last 200 rows and every 997th row."""
    assert su.mfma_plan(7, 512, B, O)[2] == nw
    cfg, params = _net(7, 512, O, "gaussian")
    x = _queries(B, 7, seed=B) if B <= 10000 else _inbox(B, 7, seed=B)
    net = WCRBFNet.from_config(cfg)
    got, nw_run = _run_mfma(net, cfg, params, x)
    assert nw_run == nw
    rows = np.arange(B) if B <= 10000 else np.unique(np.r_[0:200, B - 200:B, 0:B:997])
    assert np.isfinite(got).all()
    su.check(f"K1m O={O} B={B} nw={nw} ({len(rows)} rows)", cfg, params, x[rows], got[rows])
    again, _ = _run_mfma(net, cfg, params, x)
    assert np.array_equal(got, again)


# ------------------------------------------------------------------------------------------------ 4. gate forms
@pytest.mark.parametrize("gate", ["nsplit=0", "nsplit=1", "nsplit=D", "no_ranges"])
@pytest.mark.parametrize("D,O", [(4, 10), (7, 40)])
def test_gate_forms(gpu, D, O, gate):
    cfg, params = _net(D, 50, O, "gaussian", nsplit={"nsplit=0": 0, "nsplit=1": 1}.get(gate, D))
    if gate == "no_ranges":
        cfg = dict(cfg, dimension_ranges=[])
    x = _queries(100, D, seed=D + len(gate))
    net = WCRBFNet.from_config(cfg)
    got, _ = _run_mfma(net, cfg, params, x)
    su.check(f"K1m D={D} O={O} {gate}", cfg, params, x, got, net)
    if gate == "no_ranges":                                   # model.py:70: no range, no activation
        assert np.array_equal(got, np.broadcast_to(params["params"]["linear"]["bias"], got.shape))


# ------------------------------------------------------------------------------------------------ 5. non-finite queries
@pytest.mark.parametrize("O", [10, 40])
def test_nan_and_inf_queries_in_different_tiles(gpu, O):
    """One block of 16 QJ rows (B = 64 narrow, B = 32 wide); the rows lie in different 16-row tiles of it."""
    B, rows = (64, [3, 9, 20, 30, 37, 50, 63]) if O <= 16 else (32, [1, 5, 9, 14, 17, 23, 31])
    cfg, params = _net(7, 70, O, "gaussian", nsplit=3)
    x = _queries(B, 7, seed=O)
    nan_rows, inf_rows = su.nonfinite_rows(x, gated=[0, 1, 2], ungated=[3, 4, 5, 6], rows=rows)
    assert su.mfma_plan(7, 70, B, O)[3] == 1 and len({r // 16 for r in nan_rows + inf_rows}) == B // 16
    net = WCRBFNet.from_config(cfg)
    got, _ = _run_mfma(net, cfg, params, x)
    su.check_nonfinite(f"K1m non-finite O={O}", cfg, params, x, got, nan_rows, inf_rows)


# ------------------------------------------------------------------------------------------------ 6. refusals
def _two_regions():
    lows, highs, ranges, delta = [[-1.0, 0.0]], [[0.0, 1.0]], [(0,), (1,)], [3.0]
    cfg, params = su.region_net(7, 40, 10, "gaussian", lows, highs, ranges, delta)
    return cfg, params, su.region_queries(100, 7, lows, highs, ranges, delta, seed=2)


def _one_region(D, K, O, basis):
    cfg, params = _net(D, K, O, basis)
    return cfg, params, _queries(100, D, seed=O)


REFUSED = {"R=2": (_two_regions, "rbf_fwd_qlane<"),
           "generic basis": (lambda: _one_region(7, 64, 10, "matern32"), "rbf_fwd_qlane<"),
           "D=1": (lambda: _one_region(1, 64, 3, "gaussian"), "rbf_fwd_f16mfma<"),
           "O=80": (lambda: _one_region(7, 64, 80, "gaussian"), "rbf_fwd_f16mfma_wide")}      # NT = 5 is not compiled for K1m


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_nets_k1m_does_not_take(gpu, what):
    make, other = REFUSED[what]
    cfg, params, x = make()
    net = WCRBFNet.from_config(cfg)
    buf = su.nan_buffer(100 + su.GUARD, cfg["out_features"])
    with pytest.raises(ValueError):
        su.forward_into(net, params, x, buf, _lib.FWD_K1M)
    gpu.cuda.synchronize()
    assert net.last_launch()["kernel"] == "" and bool(gpu.isnan(buf).all())            # nothing ran
    got, launch = su.forward_guarded(net, params, x)
    assert launch["kernel"].startswith(other), launch
    su.check(f"K1m refuses {what}; AUTO {launch['kernel'].split('<')[0]}", cfg, params, x, got)


# ------------------------------------------------------------------------------------------------ 7. the reduction tile and the LDS
def test_wide_net_whose_sixteen_wave_reduction_tile_does_not_fit(gpu):
    """D = 7, O = 100 (NT = 7), K = 1000, B = 777: 25 tiles ask for sixteen waves per block, whose reduction tile
    16 x 32 x (16 NT + 1) x 4 bytes = 231 KB is more than the 160 KB of LDS; eight waves (116 KB) fit."""
    assert su.mfma_lds_bytes(7, 100, 2, 16) > 160 * 1024 >= su.mfma_lds_bytes(7, 100, 2, 8)
    assert su.mfma_plan(7, 1000, 777, 100) == (7, 2, 8, 25)
    cfg, params = _net(7, 1000, 100, "gaussian")
    x = _queries(777, 7, seed=777)
    net = WCRBFNet.from_config(cfg)
    got, nw = _run_mfma(net, cfg, params, x)
    assert net.last_launch()["block"] == 512
    su.check("K1m D=7 O=100 K=1000 B=777 nw=8", cfg, params, x, got, net)
    again, _ = _run_mfma(net, cfg, params, x)
    assert np.array_equal(got, again)
