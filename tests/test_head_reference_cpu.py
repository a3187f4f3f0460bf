"""CPU checks of tests/_head_util.py, the float64 reference the GPU head tests (tests/test_gpu_mlp_head.py) compare with: the
hand-written adjoint against torch.autograd; relu'(0) = 0 (torch.relu, jax.nn.relu) and not clamp(min=0)'s 1; and the
conditions the input generators of those tests rely on."""
import numpy as np
import pytest
import torch

import _head_util as hu
from conftest import load_deeper_fixture
from oracle import irbfn_oracle as orc

GRADS = ("gh1", "gw2", "gb2", "gw3", "gb3")


def _autograd(c, relu):
    t = {k: torch.tensor(np.asarray(c[k], np.float64), requires_grad=k != "g") for k in ("h1", "W2", "b2", "W3", "b3", "g")}
    out = relu(relu(t["h1"]) @ t["W2"] + t["b2"]) @ t["W3"] + t["b3"]
    gh1, gw2, gb2, gw3, gb3 = torch.autograd.grad((out * t["g"]).sum(), [t[k] for k in ("h1", "W2", "b2", "W3", "b3")])
    return out.detach().numpy(), dict(gh1=gh1.numpy(), gw2=gw2.numpy(), gb2=gb2.numpy(), gw3=gw3.numpy(), gb3=gb3.numpy())


@pytest.mark.parametrize("B,O", [(1, 1), (33, 2), (257, 10), (1000, 16), (64, 100)])
def test_hand_adjoint_equals_autograd(B, O):
    c, _ = hu.real_case(B, O, seed=B + O)
    f = hu.forward64(c["h1"], c["W2"], c["b2"], c["W3"], c["b3"])
    assert (c["h1"] != 0).all() and (f["z2"] != 0).all()               # no pre-activation at the kink
    r = hu.backward64(c["h1"], c["W2"], c["b2"], c["W3"], c["g"])
    out, ref = _autograd(c, torch.relu)
    assert np.abs(f["out"] - out).max() <= 1e-12 * np.abs(out).max()
    for k in GRADS:
        assert np.abs(r[k] - ref[k]).max() <= 1e-12 * max(np.abs(ref[k]).max(), 1.0), k


def test_relu_derivative_at_zero_is_zero():
    """Pre-activations of exactly 0 in h1 and in z2: the hand adjoint is torch.relu's (= jax.nn.relu's: 0 at 0), and
    clamp(min=0), whose gradient at 0 is 1, gives something else."""
    c = hu.lattice_case(500, 10, seed=3)
    f = hu.forward64(c["h1"], c["W2"], c["b2"], c["W3"], c["b3"])
    assert (c["h1"] == 0).mean() > 0.25 and (f["z2"] == 0).mean() > 0.03
    r = hu.backward64(c["h1"], c["W2"], c["b2"], c["W3"], c["g"])
    out, ref = _autograd(c, torch.relu)
    assert np.array_equal(f["out"], out)
    for k in GRADS:
        assert np.array_equal(r[k], ref[k]), k                                                    # integers: exact
    _, clamp = _autograd(c, lambda t: t.clamp(min=0))
    assert not np.array_equal(r["gh1"], clamp["gh1"]) and not np.array_equal(r["gw2"], clamp["gw2"])
    assert not np.array_equal(r["gb2"], clamp["gb2"])


def test_oracle_torch_branch_has_relu_derivative_zero_at_zero():
    """oracle.deeper_wcrbfnet_apply (torch branch) on a net whose stage output is exactly 0 in places: a zero linear_pre1
    kernel and a bias with zeros give h1 = bias; the gradient of the bias is 0 where it is 0."""
    cfg, P, x, _ = load_deeper_fixture()
    p = {g: {n: torch.tensor(np.asarray(v, np.float64)) for n, v in d.items()} for g, d in P["params"].items()}
    p["linear_pre1"]["kernel"] = torch.zeros_like(p["linear_pre1"]["kernel"])
    bias = np.tile([0.0, 1.0, -1.0, 0.5], 16)
    p["linear_pre1"]["bias"] = torch.tensor(bias, requires_grad=True)
    out = orc.deeper_wcrbfnet_apply(cfg, {"params": p}, torch.tensor(np.asarray(x[:8], np.float64)))
    out.abs().sum().backward()
    g = p["linear_pre1"]["bias"].grad.numpy()
    assert (g[bias <= 0] == 0).all() and (g[bias > 0] != 0).any()


def test_nan_propagates_through_the_reference():
    c, _ = hu.real_case(5, 10, seed=1)
    c["h1"][2, 7] = np.nan
    f = hu.forward64(c["h1"], c["W2"], c["b2"], c["W3"], c["b3"])
    assert np.isnan(f["out"][2]).all() and np.isfinite(np.delete(f["out"], 2, axis=0)).all()


@pytest.mark.parametrize("B,O", [(200000, 16), (80000, 10), (4099, 1)])
def test_lattice_sums_stay_below_2_24(B, O):
    c = hu.lattice_case(B, O, seed=B + O)
    f = hu.forward64(c["h1"], c["W2"], c["b2"], c["W3"], c["b3"])
    largest = hu.lattice_largest_sum(c)
    print(f"lattice B={B} O={O}: largest sum of absolute terms <= {largest:.3g} (2^24 = {2.0 ** 24:.3g}); "
          f"z2 == 0: {(f['z2'] == 0).mean():.3f}, h1 == 0: {(c['h1'] == 0).mean():.3f}")
    assert hu.lattice_is_exact(c) and largest < 2.0 ** 24 / 4
    assert (f["z2"] == 0).mean() > 0.03 and (c["h1"] == 0).mean() > 0.3          # the case sits on the kink in both layers


@pytest.mark.parametrize("B,O,spread", [(80000, 10, False), (4099, 16, False), (33, 2, False), (32769, 10, True)])
def test_redraw_share_stays_under_its_cap(B, O, spread):
    c, share = hu.real_case(B, O, seed=B + O, w3_col_spread=spread)
    print(f"real B={B} O={O}: {100 * share:.2f} % of the rows redrawn")
    assert share <= hu.REDRAW_CAP
    assert not hu.near_kink_rows(c["h1"], c["W2"], c["b2"]).any()
    for k, v in c.items():
        assert v.dtype == np.float32 and np.isfinite(v).all(), k


def test_redraw_share_on_the_golden_head():
    """The golden checkpoint's head on h1 from its own stage (the float64 oracle's, rounded to float32)."""
    cfg, P, _, _ = load_deeper_fixture()
    p = P["params"]
    rng = np.random.default_rng(0)
    ns = len(cfg["activation_idx"])
    lo = np.array([min(cfg["lower_bounds"][d]) for d in range(ns)]); hi = np.array([max(cfg["upper_bounds"][d]) for d in range(ns)])
    x = rng.uniform(lo, hi, size=(4200, 8))
    h1 = orc.wcrbfnet_apply(dict(cfg, out_features=64), {"params": {"rbf_list": p["rbf_list"], "linear": p["linear_pre1"]}}, x)
    h1 = np.asarray(h1, np.float32)
    rows, share = hu.keep_clear_rows(h1, p["linear_pre2"]["kernel"], p["linear_pre2"]["bias"], 4099)
    print(f"golden head B=4099: {100 * share:.2f} % of the rows passed over")
    assert share <= hu.REDRAW_CAP and rows.size == 4099
